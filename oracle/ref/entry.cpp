/*
 * entry.cpp -- C entry points of oracle/_ref/libhz_ref.so -- TEST INFRASTRUCTURE ONLY.
 *
 * Forwards to the reference's own horizon_gridded_comp, horizon_locations_comp and shapes::CppTerrain, which
 * oracle/Makefile compiles unmodified from the reference tree (named on the compiler's command line only) against
 * the stand-in headers of this directory.  The arguments are the reference's, in its order; the checks its Cython
 * layer makes before calling down (known algorithm name, no guess_constant with distances) are repeated here
 * because the C++ below them would call through an unset function pointer.
 *
 * Return codes: 0 done; 1 the ray budget was exceeded (the reference's search does not end on this input);
 * 2 the stand-in refused (hzref_last_error() says why); 3 invalid argument.
 */
#include <cstdint>

#include "horizon_comp.h"
#include "shadow_comp.h"

#include <cstring>
#include <string>

#include "standin.h"

namespace {

std::string g_last_error;

template <typename F>
int guarded(F &&f) {
    g_last_error.clear();
    try {
        f();
        return 0;
    } catch (const hzref::budget_exceeded &e) {
        g_last_error = e.what();
        return 1;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return 2;
    }
}

bool known_algorithm(const char *a) {
    return !strcmp(a, "discrete_sampling") || !strcmp(a, "binary_search") || !strcmp(a, "guess_constant");
}

bool known_geometry(const char *g) { return !strcmp(g, "triangle") || !strcmp(g, "quad") || !strcmp(g, "grid"); }

struct terrain {
    shapes::CppTerrain *t;
    bool initialised;
};

}  // namespace

extern "C" {

const char *hzref_last_error(void) { return g_last_error.c_str(); }

int hzref_horizon_gridded(float *vert_grid, int dem_dim_0, int dem_dim_1, float *vec_norm, float *vec_north,
                          int offset_0, int offset_1, float *hori_buffer, int dim_in_0, int dim_in_1, int azim_num,
                          float dist_search, float hori_acc, char *ray_algorithm, char *geom_type, float *vert_simp,
                          int num_vert_simp, int *tri_ind_simp, int num_tri_simp, float elev_ang_low_lim,
                          uint8_t *mask, float hori_fill, float ray_org_elev) {
    if (!known_algorithm(ray_algorithm) || !known_geometry(geom_type) || azim_num < 1) return 3;
    const int rc = guarded([&] {
        horizon_gridded_comp(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1, hori_buffer,
                             dim_in_0, dim_in_1, azim_num, dist_search, hori_acc, ray_algorithm, geom_type, vert_simp,
                             num_vert_simp, tri_ind_simp, num_tri_simp, elev_ang_low_lim, mask, hori_fill,
                             ray_org_elev);
    });
    if (rc) hzref::release_leftovers();
    return rc;
}

int hzref_horizon_locations(float *vert_grid, int dem_dim_0, int dem_dim_1, float *coords, float *vec_norm,
                            float *vec_north, float *hori_buffer, float *hori_dist_buffer, int num_loc, int azim_num,
                            float dist_search, float hori_acc, char *ray_algorithm, char *geom_type,
                            float elev_ang_low_lim, float *ray_org_elev, int hori_dist_out) {
    if (!known_algorithm(ray_algorithm) || !known_geometry(geom_type) || azim_num < 1) return 3;
    if (hori_dist_out && !strcmp(ray_algorithm, "guess_constant")) return 3;
    const int rc = guarded([&] {
        horizon_locations_comp(vert_grid, dem_dim_0, dem_dim_1, coords, vec_norm, vec_north, hori_buffer,
                               hori_dist_buffer, num_loc, azim_num, dist_search, hori_acc, ray_algorithm, geom_type,
                               elev_ang_low_lim, ray_org_elev, hori_dist_out);
    });
    if (rc) hzref::release_leftovers();
    return rc;
}

void *hzref_terrain_new(void) {
    terrain *h = new terrain{nullptr, false};
    if (guarded([&] { h->t = new shapes::CppTerrain(); })) { delete h; return nullptr; }
    h->t->scene = nullptr;                  /* its constructor leaves the handle unset; its destructor releases it */
    hzref::forget_device(h->t->device);     /* owned by the object from here on */
    return h;
}

/* the arrays are kept by pointer (as the reference's class keeps them): the caller holds them until _delete */
int hzref_terrain_initialise(void *handle, float *vert_grid, int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
                             float *vec_tilt, float *vec_norm, int dim_in_0, int dim_in_1, float *surf_enl_fac,
                             float *elevation, unsigned char *mask, char *geom_type, float sw_dir_cor_fill,
                             float ang_max, int refrac_cor) {
    terrain *h = (terrain *)handle;
    if (!h || h->initialised || !known_geometry(geom_type)) return 3;
    const int rc = guarded([&] {
        h->t->initialise(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_tilt, vec_norm, dim_in_0, dim_in_1,
                         surf_enl_fac, elevation, mask, geom_type, sw_dir_cor_fill, ang_max, refrac_cor);
    });
    if (rc) { hzref::release_leftovers(); return rc; }
    hzref::forget_scene(h->t->scene);
    h->initialised = true;
    return 0;
}

int hzref_terrain_shadow(void *handle, float *sun_position, unsigned char *shadow_buffer) {
    terrain *h = (terrain *)handle;
    if (!h || !h->initialised) return 3;
    return guarded([&] { h->t->shadow(sun_position, shadow_buffer); });
}

int hzref_terrain_sw_dir_cor(void *handle, float *sun_position, float *sw_dir_cor_buffer) {
    terrain *h = (terrain *)handle;
    if (!h || !h->initialised) return 3;
    return guarded([&] { h->t->sw_dir_cor(sun_position, sw_dir_cor_buffer); });
}

void hzref_terrain_delete(void *handle) {
    terrain *h = (terrain *)handle;
    if (!h) return;
    delete h->t;
    delete h;
}

}
