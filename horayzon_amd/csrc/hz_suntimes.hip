// hz_suntimes.hip -- HorizonTerrain.sun_times (hz_horizon_terrain_sun_times): sunrise, sunset, sunshine duration and the
// number of sunlit spells of every cell over a sun track, from a stored horizon (clause 14).
//
// k_horisun's shape: one lane owns one cell of the inner domain and walks the positions of a launch in its inner loop; frame,
// tilt, vertex and refraction factor are loaded once.  Per position the lane forms the float32 set-up of clause 10 (clause 13
// with REFRAC, without shadow_setup's early exit for back slopes: that exit moves no shadow code, but here the clearance of a
// back slope places the crossing next to it), evaluates the float64 look-up for EVERY position -- also where the surface
// faces away -- and keeps the clearance g = fmin(alpha - h, asin(dot_ts)) of the position before.  Where the lit state
// changes between two positions the crossing time is interpolated from the two clearances.  The running state (rise, set,
// dur, open, g_prev, lit_prev, n) stays in registers during a launch; between the launches of a call it lives in a struct of
// arrays f64[5][cells] + i32[cells], so every load and store of it is coalesced.  PLANES reads the horizon as
// planes[k * stride + c] (clause 11).  The arithmetic of the look-up is written again here in k_horisun's order of operations
// (hz_horisun.hip and hz_planes.hip do not move); this file is built with -ffp-contract=off like them, so `alpha < h` decides
// exactly as their kernels do.
#include "hz_internal.h"
#include "hz_horisun_plan.h"
#include "hz_horisun_refrac.h"
#include "hz_q16.h"

namespace hz {

// shadow_comp.cpp:96-106, as horisun_unit of hz_horisun.hip
__device__ __forceinline__ void suntimes_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// horisun_refract of hz_horisun_refrac.h (clause 13, steps 3 - 7) for every cell: no early exit
__device__ __forceinline__ void suntimes_refract(double fac, float norm_x, float norm_y, float norm_z, float &sun_x, float &sun_y,
                                                 float &sun_z, float &dot_prod_ns) {
    const float elev_ang_true = (float)(90.0 - (double)horisun_rad2deg_f(hz_crm_acosf(dot_prod_ns)));
    const float refrac_cor = horisun_atmos_refrac(elev_ang_true, fac);
    float k_x = sun_y * norm_z - sun_z * norm_y;
    float k_y = sun_z * norm_x - sun_x * norm_z;
    float k_z = sun_x * norm_y - sun_y * norm_x;
    suntimes_unit(k_x, k_y, k_z);
    const float theta = horisun_deg2rad_f(refrac_cor);           // vec_rot, shadow_comp.cpp:109-132
    const float ct = hz_crm_cosf(theta), st = hz_crm_sinf(theta);
    const float part = (float)((double)((k_x * sun_x + k_y * sun_y) + k_z * sun_z) * (1.0 - (double)ct));
    const float rx = (sun_x * ct + (k_y * sun_z - k_z * sun_y) * st) + k_x * part;
    const float ry = (sun_y * ct + (k_z * sun_x - k_x * sun_z) * st) + k_y * part;
    const float rz = (sun_z * ct + (k_x * sun_y - k_y * sun_x) * st) + k_z * part;
    sun_x = rx; sun_y = ry; sun_z = rz;
    dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
}

// horisun_shaded of hz_horisun.hip, returning alpha and h instead of their comparison.  `base` = the cell's first horizon
// word, `step` = the distance of its azimuths in words (1: cell-major row, the plane stride: planes).  H: float, or uint16_t
// for the codes of clause 15 (hori_value, hz_q16.h)
template <typename H>
__device__ __forceinline__ void suntimes_lookup(const H *__restrict__ base, size_t step, int azim_num, double per_rad,
                                                float sx, float sy, float sz, float nx, float ny, float nz,
                                                float hx, float hy, float hz_, double ex, double ey, double ez,
                                                double &alpha, double &h) {
    const double cn = ((double)sx * (double)hx + (double)sy * (double)hy) + (double)sz * (double)hz_;
    const double ce = ((double)sx * ex + (double)sy * ey) + (double)sz * ez;
    const double cu = ((double)sx * (double)nx + (double)sy * (double)ny) + (double)sz * (double)nz;
    double phi = atan2(ce, cn);
    if (phi < 0.0) phi += 6.283185307179586;
    const double u = phi * per_rad;
    // u is in [0, A] for finite inputs; the clamp keeps the two loads inside the horizon whatever the inputs are (NaN: 0)
    const double kf = fmin(fmax(floor(u), 0.0), (double)azim_num);
    const double t = u - kf;
    const int k = (int)kf;
    const int k0 = k % azim_num, k1 = (k + 1) % azim_num;
    h = (1.0 - t) * hori_value(base[(size_t)k0 * step]) + t * hori_value(base[(size_t)k1 * step]);
    alpha = asin(fmin(fmax(cu, -1.0), 1.0));
}

// REFRAC: p.refrac_fac is not null (clause 13); PLANES: p.hori = planes [azim_num][p.stride]; H: the element type of p.hori
template <bool REFRAC, bool PLANES, typename H>
__global__ __launch_bounds__(HZ_HORISUN_TPB) void k_suntimes(SuntimesArgs p) {
    const size_t c = (size_t)blockIdx.x * HZ_HORISUN_TPB + threadIdx.x;
    if (c >= p.cells) return;
    const size_t n_cells = p.cells;
    if (p.mask[c] != 1) {
        if (p.last) {
            if (p.sunrise) p.sunrise[c] = p.fill;
            if (p.sunset) p.sunset[c] = p.fill;
            if (p.duration) p.duration[c] = p.fill;
            if (p.intervals) p.intervals[c] = -1;
        }
        return;
    }
    const float tilt_x = p.vec_tilt[3 * c], tilt_y = p.vec_tilt[3 * c + 1], tilt_z = p.vec_tilt[3 * c + 2];
    const float norm_x = p.vec_norm[3 * c], norm_y = p.vec_norm[3 * c + 1], norm_z = p.vec_norm[3 * c + 2];
    const float north_x = p.vec_north[3 * c], north_y = p.vec_north[3 * c + 1], north_z = p.vec_north[3 * c + 2];
    const float ray_org_elev = 0.05f;                              // shadow_comp.cpp:388, :497
    const float ox = p.vert[3 * c] + norm_x * ray_org_elev;
    const float oy = p.vert[3 * c + 1] + norm_y * ray_org_elev;
    const float oz = p.vert[3 * c + 2] + norm_z * ray_org_elev;
    // east = north x norm: products of two floats are exact in float64, each difference is rounded once
    const double ex = (double)north_y * (double)norm_z - (double)north_z * (double)norm_y;
    const double ey = (double)north_z * (double)norm_x - (double)north_x * (double)norm_z;
    const double ez = (double)north_x * (double)norm_y - (double)north_y * (double)norm_x;
    const double per_rad = (double)p.azim_num / 6.283185307179586;
    const H *hori = reinterpret_cast<const H *>(p.hori);
    const H *base = PLANES ? hori + c : hori + c * (size_t)p.azim_num;
    const size_t step = PLANES ? p.stride : 1;
    double fac = 0.0;
    if (REFRAC) fac = p.refrac_fac[c];
    // the state of clause 14: before the first position nothing has happened
    double rise = 0.0, set = 0.0, dur = 0.0, open = 0.0, g_prev = 0.0, t_prev = p.t_before;
    int n = 0;
    bool lit_prev = false;
    if (!p.first) {
        rise = p.state[c]; set = p.state[n_cells + c]; dur = p.state[2 * n_cells + c]; open = p.state[3 * n_cells + c];
        g_prev = p.state[4 * n_cells + c];
        const int w = p.state_n[c];                                // the count, and the lit state in the lowest bit
        n = w >> 1; lit_prev = (w & 1) != 0;
    }
    for (int s = 0; s < p.num_sun; s++) {
        float sun_x = p.suns[3 * s] - ox, sun_y = p.suns[3 * s + 1] - oy, sun_z = p.suns[3 * s + 2] - oz;   // :422-425
        suntimes_unit(sun_x, sun_y, sun_z);
        float dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
        if (REFRAC) suntimes_refract(fac, norm_x, norm_y, norm_z, sun_x, sun_y, sun_z, dot_prod_ns);
        const float dot_prod_ts = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
        double alpha, h;
        suntimes_lookup(base, step, p.azim_num, per_rad, sun_x, sun_y, sun_z, norm_x, norm_y, norm_z, north_x, north_y, north_z,
                        ex, ey, ez, alpha, h);
        // the clearance over terrain and surface [rad]; a NaN horizon leaves the surface's
        const double beta = asin(fmin(fmax((double)dot_prod_ts, -1.0), 1.0));
        const double g = fmin(alpha - h, beta);
        const bool lit = dot_prod_ts > 0.0f && !(alpha < h);         // shadow code 0 of k_horisun
        const double t_s = p.times[s];
        if (p.first && s == 0) {
            if (lit) { open = t_s; rise = t_s; n = 1; }
        } else if (lit != lit_prev) {
            double f = g_prev / (g_prev - g);
            if (!(f >= 0.0 && f <= 1.0)) f = 0.5;
            const double tau = t_prev + f * (t_s - t_prev);
            if (lit) {
                open = tau;
                if (n == 0) rise = tau;
                n += 1;
            } else {
                dur += tau - open;
                set = tau;
            }
        }
        g_prev = g; lit_prev = lit; t_prev = t_s;
    }
    if (p.last) {
        if (lit_prev) { dur += t_prev - open; set = t_prev; }
        const float none = __builtin_nanf("");
        if (p.sunrise) p.sunrise[c] = n ? (float)rise : none;
        if (p.sunset) p.sunset[c] = n ? (float)set : none;
        if (p.duration) p.duration[c] = n ? (float)dur : 0.0f;
        if (p.intervals) p.intervals[c] = n;
    } else {
        p.state[c] = rise; p.state[n_cells + c] = set; p.state[2 * n_cells + c] = dur; p.state[3 * n_cells + c] = open;
        p.state[4 * n_cells + c] = g_prev;
        p.state_n[c] = (n << 1) | (lit_prev ? 1 : 0);
    }
}

size_t suntimes_state_bytes(size_t cells) { return cells * (5 * sizeof(double) + sizeof(int32_t)); }

template <typename H>
static void suntimes_launch_as(const SuntimesArgs &a, bool planes, dim3 grid, dim3 block, hipStream_t st) {
    if (a.refrac_fac) {
        if (planes) hipLaunchKernelGGL((k_suntimes<true, true, H>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_suntimes<true, false, H>), grid, block, 0, st, a);
    } else {
        if (planes) hipLaunchKernelGGL((k_suntimes<false, true, H>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_suntimes<false, false, H>), grid, block, 0, st, a);
    }
}

int suntimes_launch(const SuntimesArgs &a, bool planes, unsigned blocks, hipStream_t st, bool q16) {
    if (a.cells == 0 || a.num_sun <= 0 || blocks == 0) return HZ_OK;
    const dim3 grid(blocks), block(HZ_HORISUN_TPB);
    if (q16) suntimes_launch_as<uint16_t>(a, planes, grid, block, st);
    else suntimes_launch_as<float>(a, planes, grid, block, st);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
