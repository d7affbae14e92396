// hz_horisun.hip -- HorizonTerrain (hz_horizon_terrain_*): shadow mask and direct-shortwave correction from a stored
// horizon instead of a ray (clause 10).
//
// One lane owns one cell of the inner domain and walks the sun positions of a launch in its inner loop: the cell's frame,
// tilt, vertex and surface enlargement factor are loaded once and stay in registers, and so do the two float64 sums of
// `accumulate`.  Per position: the float32 set-up of shadow_setup (hz_shadow.hip; written again here in the same order of
// operations -- that file's machine code must not move), then, for the cells that pass the self-shading test, the sun's
// azimuth and elevation in the cell's frame in float64 and two loads from the cell's horizon row.  A lane's row is 4 A bytes
// from its neighbour's, so those two loads are uncoalesced; the per-position outputs out[s][cell] are coalesced.  The horizon's
// element type is a template parameter: float, or the 16-bit codes of clause 15, decoded to float32 as they are loaded.
#include "hz_internal.h"
#include "hz_horisun_plan.h"
#include "hz_horisun_refrac.h"
#include "hz_q16.h"

namespace hz {

std::atomic<int> g_horisun_chunk{0};

// shadow_comp.cpp:96-106, as vec_unit of hz_shadow.hip
__device__ __forceinline__ void horisun_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// terrain-shaded: the sun's elevation against the horizon row interpolated at the sun's azimuth, float64, every
// product and sum rounded on its own (the library is built with -ffp-contract=off).  H: float, or uint16_t for a row of
// 16-bit codes, each decoded to float32 and widened (hori_value, hz_q16.h)
template <typename H>
__device__ __forceinline__ bool horisun_shaded(const H *__restrict__ row, int azim_num, double per_rad,
                                               float sx, float sy, float sz, float nx, float ny, float nz,
                                               float hx, float hy, float hz_, double ex, double ey, double ez) {
    const double cn = ((double)sx * (double)hx + (double)sy * (double)hy) + (double)sz * (double)hz_;
    const double ce = ((double)sx * ex + (double)sy * ey) + (double)sz * ez;
    const double cu = ((double)sx * (double)nx + (double)sy * (double)ny) + (double)sz * (double)nz;
    double phi = atan2(ce, cn);
    if (phi < 0.0) phi += 6.283185307179586;
    const double u = phi * per_rad;
    // u is in [0, A] for finite inputs; the clamp keeps the two loads inside the row whatever the inputs are (NaN: 0)
    const double kf = fmin(fmax(floor(u), 0.0), (double)azim_num);
    const double t = u - kf;
    const int k = (int)kf;
    const int k0 = k % azim_num, k1 = (k + 1) % azim_num;
    const double h = (1.0 - t) * hori_value(row[k0]) + t * hori_value(row[k1]);
    const double alpha = asin(fmin(fmax(cu, -1.0), 1.0));
    return alpha < h;                                   // NaN horizon: false, the cell counts as lit
}

// REFRAC: the sun direction is bent by the atmospheric refraction first (clause 13; p.refrac_fac is not null)
// H: the element type of p.hori (float; uint16_t: the codes of clause 15)
template <bool REFRAC, typename H>
__global__ __launch_bounds__(HZ_HORISUN_TPB) void k_horisun(HorisunArgs p) {
    const size_t c = (size_t)blockIdx.x * HZ_HORISUN_TPB + threadIdx.x;
    if (c >= p.cells) return;
    const size_t n = p.cells;
    const bool want_code = p.out_u8 != nullptr || p.sum_lit != nullptr;     // the same in every lane
    if (p.mask[c] != 1) {
        for (int s = 0; s < p.num_sun; s++) {
            if (p.out_u8) p.out_u8[(size_t)s * n + c] = 3;
            if (p.out_f32) p.out_f32[(size_t)s * n + c] = p.fill;
        }
        if (p.last) {
            if (p.sum_sw) p.sum_sw[c] = p.fill;
            if (p.sum_lit) p.sum_lit[c] = p.fill;
        }
        return;
    }
    const float tilt_x = p.vec_tilt[3 * c], tilt_y = p.vec_tilt[3 * c + 1], tilt_z = p.vec_tilt[3 * c + 2];
    const float norm_x = p.vec_norm[3 * c], norm_y = p.vec_norm[3 * c + 1], norm_z = p.vec_norm[3 * c + 2];
    const float north_x = p.vec_north[3 * c], north_y = p.vec_north[3 * c + 1], north_z = p.vec_north[3 * c + 2];
    const float enl = p.surf_enl_fac[c];
    const float ray_org_elev = 0.05f;                              // shadow_comp.cpp:388, :497
    const float ox = p.vert[3 * c] + norm_x * ray_org_elev;
    const float oy = p.vert[3 * c + 1] + norm_y * ray_org_elev;
    const float oz = p.vert[3 * c + 2] + norm_z * ray_org_elev;
    // east = north x norm: products of two floats are exact in float64, each difference is rounded once
    const double ex = (double)north_y * (double)norm_z - (double)north_z * (double)norm_y;
    const double ey = (double)north_z * (double)norm_x - (double)north_x * (double)norm_z;
    const double ez = (double)north_x * (double)norm_y - (double)north_y * (double)norm_x;
    const double per_rad = (double)p.azim_num / 6.283185307179586;
    const H *row = reinterpret_cast<const H *>(p.hori) + c * (size_t)p.azim_num;
    double a_sw = (p.sum_sw && !p.first) ? p.acc_sw[c] : 0.0;
    double a_lit = (p.sum_lit && !p.first) ? p.acc_lit[c] : 0.0;
    double fac = 0.0;
    if (REFRAC) fac = p.refrac_fac[c];
    for (int s = 0; s < p.num_sun; s++) {
        float sun_x = p.suns[3 * s] - ox, sun_y = p.suns[3 * s + 1] - oy, sun_z = p.suns[3 * s + 2] - oz;   // :422-425
        horisun_unit(sun_x, sun_y, sun_z);
        float dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
        if (REFRAC) horisun_refract(fac, tilt_x, tilt_y, tilt_z, norm_x, norm_y, norm_z, sun_x, sun_y, sun_z, dot_prod_ns);
        const float dot_prod_ts = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
        int code = 1;                                   // self-shaded (shadow: !(dot_ts > 0))
        float val = 0.0f;                               // sw_dir_cor: 0 outside ang_max (!(dot_ts > dot_prod_min)) and in shadow
        // the look-up decides the code of every cell with dot_ts > 0, and the value of those with dot_ts > dot_prod_min (> 0)
        if (dot_prod_ts > (want_code ? 0.0f : p.dot_prod_min)) {
            const bool shaded = horisun_shaded(row, p.azim_num, per_rad, sun_x, sun_y, sun_z, norm_x, norm_y, norm_z,
                                               north_x, north_y, north_z, ex, ey, ez);
            code = shaded ? 2 : 0;
            if (!shaded && dot_prod_ts > p.dot_prod_min) {         // shadow_result
                float d = dot_prod_ns;
                if (d < p.dot_prod_min) d = p.dot_prod_min;
                val = (dot_prod_ts / d) * enl;
            }
        }
        if (p.out_u8) p.out_u8[(size_t)s * n + c] = (uint8_t)code;
        if (p.out_f32) p.out_f32[(size_t)s * n + c] = val;
        // clause 9: acc += (double)w * (double)value, ascending s
        const double w = p.weights ? (double)p.weights[s] : 1.0;
        if (p.sum_sw) a_sw += w * (double)val;
        if (p.sum_lit) a_lit += w * (code == 0 ? 1.0 : 0.0);
    }
    if (p.last) {                                       // one rounding
        if (p.sum_sw) p.sum_sw[c] = (float)a_sw;
        if (p.sum_lit) p.sum_lit[c] = (float)a_lit;
    } else {
        if (p.sum_sw) p.acc_sw[c] = a_sw;
        if (p.sum_lit) p.acc_lit[c] = a_lit;
    }
}

int horisun_launch(const HorisunArgs &a, unsigned blocks, hipStream_t st, bool q16) {
    if (a.cells == 0 || a.num_sun <= 0 || blocks == 0) return HZ_OK;
    const dim3 grid(blocks), block(HZ_HORISUN_TPB);
    if (q16) {
        if (a.refrac_fac) hipLaunchKernelGGL((k_horisun<true, uint16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_horisun<false, uint16_t>), grid, block, 0, st, a);
    } else {
        if (a.refrac_fac) hipLaunchKernelGGL((k_horisun<true, float>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_horisun<false, float>), grid, block, 0, st, a);
    }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
