/*
 * selftest_main.cpp -- stand-alone run of the reference driver on the stand-in, for sanitizer builds.
 *
 * TEST INFRASTRUCTURE ONLY.  `make -C oracle ref-asan` compiles the reference's two sources, the stand-in, the entry
 * wrapper, the oracle and this file with -fsanitize=address,undefined into one program (no Python, no LD_PRELOAD) and
 * runs it: one small hill through horizon_gridded (three searches), horizon_locations with distances, and
 * Terrain.shadow / sw_dir_cor with refraction; then a guard case under a small ray budget, which must end with the
 * budget error and leave nothing allocated.  Exit status 0 and no sanitizer report is the result.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
const char *hzref_last_error(void);
void hzref_set_ray_budget(int64_t max_rays);
int64_t hzref_rays_cast(void);
int hzref_horizon_gridded(float *, int, int, float *, float *, int, int, float *, int, int, int, float, float, char *, char *,
                          float *, int, int *, int, float, uint8_t *, float, float);
int hzref_horizon_locations(float *, int, int, float *, float *, float *, float *, float *, int, int, float, float, char *,
                            char *, float, float *, int);
void *hzref_terrain_new(void);
int hzref_terrain_initialise(void *, float *, int, int, int, int, float *, float *, int, int, float *, float *,
                             unsigned char *, char *, float, float, int);
int hzref_terrain_shadow(void *, float *, unsigned char *);
int hzref_terrain_sw_dir_cor(void *, float *, float *);
void hzref_terrain_delete(void *);
}

static std::vector<float> hill(int n, float dx, float height, float sigma) {
    std::vector<float> v((size_t)3 * n * n + 16, 0.0f);
    const float mid = 0.5f * (n - 1) * dx;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const float x = j * dx, y = (n - 1 - i) * dx;
            float *p = &v[3 * ((size_t)i * n + j)];
            p[0] = x; p[1] = y;
            p[2] = height * std::exp(-((x - mid) * (x - mid) + (y - mid) * (y - mid)) / (2.0f * sigma * sigma));
        }
    return v;
}

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, hzref_last_error()); return 1; } } while (0)

int main() {
    const int n = 40, off = 12, in = n - 2 * off, azim = 12;
    std::vector<float> vert = hill(n, 50.0f, 150.0f, 350.0f);
    std::vector<float> norm((size_t)3 * in * in), north(norm.size()), tilt(norm.size());
    for (int c = 0; c < in * in; c++) {
        norm[3 * c + 2] = 1.0f; north[3 * c + 1] = 1.0f;
        tilt[3 * c] = 0.06f; tilt[3 * c + 1] = -0.08f; tilt[3 * c + 2] = 0.995f;
    }
    std::vector<uint8_t> mask((size_t)in * in, 1);
    mask[5] = 0;
    std::vector<float> hori((size_t)in * in * azim), simp(4, 0.0f);
    std::vector<int> tri(4, 0);
    char triangle[] = "triangle";
    char algs[3][24] = {"guess_constant", "binary_search", "discrete_sampling"};
    for (auto &alg : algs) {
        hzref_set_ray_budget(4000000);
        CHECK(hzref_horizon_gridded(vert.data(), n, n, norm.data(), north.data(), off, off, hori.data(), in, in, azim, 1.0f,
                                    0.25f, alg, triangle, simp.data(), 1, tri.data(), 1, -15.0f, mask.data(), -1.0f,
                                    0.1f) == 0);
        double sum = 0.0;
        for (float h : hori) sum += h;
        printf("%-18s rays %lld  sum(hori) %.9g\n", alg, (long long)hzref_rays_cast(), sum);
    }
    /* locations with distances */
    const int nloc = 3;
    float coords[nloc * 3] = {1000.0f, 1000.0f, 200.0f, 925.0f, 1010.0f, 0.0f, 5000.0f, 5000.0f, 10.0f};
    float lnorm[nloc * 3] = {0, 0, 1, 0, 0, 1, 0, 0, 1}, lnorth[nloc * 3] = {0, 1, 0, 0, 1, 0, 0, 1, 0};
    float roe[nloc] = {0.5f, 0.01f, 1.0f};
    std::vector<float> lh((size_t)nloc * azim, NAN), ld((size_t)nloc * azim, NAN);
    hzref_set_ray_budget(1000000);
    CHECK(hzref_horizon_locations(vert.data(), n, n, coords, lnorm, lnorth, lh.data(), ld.data(), nloc, azim, 1.0f, 0.25f,
                                  algs[1], triangle, -30.0f, roe, 1) == 0);
    CHECK(std::isnan(lh[2 * azim]) && !std::isnan(lh[0]));
    /* terrain with refraction */
    std::vector<float> enl((size_t)in * in, 1.01f), elev((size_t)in * in, 730.0f), cor((size_t)in * in);
    std::vector<unsigned char> sh((size_t)in * in);
    float sun[3] = {1000.0f + 9.0e7f, 1000.0f - 3.0e7f, 1.2e7f};
    void *t = hzref_terrain_new();
    CHECK(t != nullptr);
    CHECK(hzref_terrain_initialise(t, vert.data(), n, n, off, off, tilt.data(), norm.data(), in, in, enl.data(), elev.data(),
                                   mask.data(), triangle, -9.0f, 89.0f, 1) == 0);
    hzref_set_ray_budget(in * in);
    CHECK(hzref_terrain_shadow(t, sun, sh.data()) == 0);
    hzref_set_ray_budget(in * in);
    CHECK(hzref_terrain_sw_dir_cor(t, sun, cor.data()) == 0);
    CHECK(sh[5] == 3 && cor[5] == -9.0f);
    hzref_terrain_delete(t);
    /* a guard case: steep hill, narrow ring -- must stop at the budget and free what the reference left behind */
    std::vector<float> steep = hill(n, 50.0f, 900.0f, 400.0f);
    hzref_set_ray_budget(200000);
    CHECK(hzref_horizon_gridded(steep.data(), n, n, norm.data(), north.data(), off, off, hori.data(), in, in, azim, 5.0f, 0.25f,
                                algs[0], triangle, simp.data(), 1, tri.data(), 1, -15.0f, mask.data(), -1.0f, 0.1f) == 1);
    printf("guard case ended with: %s\nselftest ok\n", hzref_last_error());
    return 0;
}
