// hz_horisun_coarse.hip -- HorizonTerrain.sw_dir_cor_coarse (hz_horizon_terrain_sw_dir_cor_coarse): per sun position, the block
// means of sw_dir_cor and of the sunlit flag over p0 x p1 cells, from a stored horizon (clause 12).
//
// k_horisun_coarse joins clause 10's look-up (k_horisun, k_horisun_planes) with clause 9's ordered block sum
// (k_coarse_reduce, hz_subgrid.hip) without a map per position in between: the look-up needs no scratch, so the values go
// from the lanes that compute them into LDS and from there into the float64 accumulators.  The launch plan -- strips, tile
// rows, positions per pass, LDS layout -- is hz_horisun_coarse_plan.h.
//
// Contract: the sum of a coarse cell is a float64 accumulator that starts at 0.0 and takes (double)sw_dir_cor of the block's
// unmasked cells one at a time, rows ascending and within a row columns ascending, so ONE lane adds all cells of a block for
// one position, in that order, tile after tile.  As in hz_subgrid.hip a masked or unlit cell contributes +0.0 instead of
// being skipped: the accumulator starts at +0.0 and a round-to-nearest sum is -0.0 only if both operands are, so it is never
// -0.0 and `x + 0.0` leaves every bit of it as it is.
//
// A lane holds one cell's frame at a time (k_horisun: 144 VGPRs; two frames kept over a workgroup's positions made 197 and
// two waves per SIMD instead of three, and lost to the two-pass route), so the frame is loaded again for every (position,
// cell) pair: 53 bytes that the other positions of the pass left in the cache.  In return the pairs of a pass are dealt to the
// threads one by one, so a tile whose width is no multiple of the workgroup idles no lane.
//
// The look-up arithmetic is k_horisun's, written again here in the same order of operations (that file's text does not
// move); the library is built with -ffp-contract=off, so the values are the same words.
#include "hz_internal.h"
#include "hz_horisun_coarse_plan.h"
#include "hz_horisun_refrac.h"

namespace hz {

std::atomic<int> g_horisun_coarse_tile{0};
std::atomic<int> g_horisun_coarse_route{-1};
// The route a call takes when the knob does not say, per layout [cell-major, planes]: 1, the two-pass route, on both.  Measured
// on the 3601^2 tile with 43 x 43 blocks and 144 positions (scripts/horisun_coarse_perf.py): kernel time
// 34.3 ms fused against 22.4 ms two-pass cell-major, 26.3 against 21.2 ms on planes.
static const int k_default_route[2] = {1, 1};

struct HorisunCoarseArgs {
    const float *hori;                   // PLANES: f32[azim_num][stride], else f32[cells][azim_num]
    size_t stride;
    const float *vert, *vec_tilt, *vec_norm, *vec_north, *surf_enl_fac;
    const uint8_t *mask;
    const unsigned *n;                   // u32[gy][gx], k_coarse_count
    const float *suns;                   // f32[num_sun][3]: the chunk
    int num_sun, azim_num;
    float fill, dot_prod_min;
    int dim_1, p0, p1, gy, gx;
    int nb, nstrips, rows, pitch, q;
    unsigned off_flags;                  // byte offset of the lit flags in dynamic LDS (the values are at 0)
    float *f_cor, *lit;                  // [num_sun][gy][gx] at the chunk's first position, or null
    const double *refrac_fac;            // REFRAC: f64[cells], shadow_refrac_factor() (clause 13)
};

// one cell's frame
struct CoarseFrame {
    float tilt_x, tilt_y, tilt_z, norm_x, norm_y, norm_z, north_x, north_y, north_z, ox, oy, oz, enl;
    double ex, ey, ez;
};

// shadow_comp.cpp:96-106, as horisun_unit of hz_horisun.hip
__device__ __forceinline__ void coarse_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// horisun_shaded of hz_horisun.hip / planes_shaded of hz_planes.hip: the cell's horizon at azimuth k is
// hori[cell * A + k] or planes[k * stride + cell]
template <bool PLANES>
__device__ __forceinline__ bool coarse_shaded(const float *__restrict__ hori, size_t cell, size_t stride, int azim_num,
                                              double per_rad, float sx, float sy, float sz, const CoarseFrame &f) {
    const double cn = ((double)sx * (double)f.north_x + (double)sy * (double)f.north_y) + (double)sz * (double)f.north_z;
    const double ce = ((double)sx * f.ex + (double)sy * f.ey) + (double)sz * f.ez;
    const double cu = ((double)sx * (double)f.norm_x + (double)sy * (double)f.norm_y) + (double)sz * (double)f.norm_z;
    double phi = atan2(ce, cn);
    if (phi < 0.0) phi += 6.283185307179586;
    const double u = phi * per_rad;
    // u is in [0, A] for finite inputs; the clamp keeps the two loads inside the horizon whatever the inputs are (NaN: 0)
    const double kf = fmin(fmax(floor(u), 0.0), (double)azim_num);
    const double t = u - kf;
    const int k = (int)kf;
    const int k0 = k % azim_num, k1 = (k + 1) % azim_num;
    const double h0 = (double)(PLANES ? hori[(size_t)k0 * stride + cell] : hori[cell * (size_t)azim_num + (size_t)k0]);
    const double h1 = (double)(PLANES ? hori[(size_t)k1 * stride + cell] : hori[cell * (size_t)azim_num + (size_t)k1]);
    const double h = (1.0 - t) * h0 + t * h1;
    const double alpha = asin(fmin(fmax(cu, -1.0), 1.0));
    return alpha < h;                                   // NaN horizon: false, the cell counts as lit
}

__device__ __forceinline__ void coarse_frame_load(const HorisunCoarseArgs &p, size_t cc, CoarseFrame &f) {
    f.tilt_x = p.vec_tilt[3 * cc]; f.tilt_y = p.vec_tilt[3 * cc + 1]; f.tilt_z = p.vec_tilt[3 * cc + 2];
    f.norm_x = p.vec_norm[3 * cc]; f.norm_y = p.vec_norm[3 * cc + 1]; f.norm_z = p.vec_norm[3 * cc + 2];
    f.north_x = p.vec_north[3 * cc]; f.north_y = p.vec_north[3 * cc + 1]; f.north_z = p.vec_north[3 * cc + 2];
    f.enl = p.surf_enl_fac[cc];
    const float ray_org_elev = 0.05f;                              // shadow_comp.cpp:388, :497
    f.ox = p.vert[3 * cc] + f.norm_x * ray_org_elev;
    f.oy = p.vert[3 * cc + 1] + f.norm_y * ray_org_elev;
    f.oz = p.vert[3 * cc + 2] + f.norm_z * ray_org_elev;
    // east = north x norm: products of two floats are exact in float64, each difference is rounded once
    f.ex = (double)f.north_y * (double)f.norm_z - (double)f.north_z * (double)f.norm_y;
    f.ey = (double)f.north_z * (double)f.norm_x - (double)f.north_x * (double)f.norm_z;
    f.ez = (double)f.north_x * (double)f.norm_y - (double)f.north_y * (double)f.norm_x;
}

// clause 10 for one unmasked cell and one position: sw_dir_cor, and whether the cell is lit (shadow code 0)
template <bool PLANES, bool CODES, bool REFRAC>
__device__ __forceinline__ void coarse_eval(const HorisunCoarseArgs &p, size_t cell, const float *__restrict__ sun, double per_rad,
                                            float &val, int &lit) {
    CoarseFrame f;
    coarse_frame_load(p, cell, f);
    float sun_x = sun[0] - f.ox, sun_y = sun[1] - f.oy, sun_z = sun[2] - f.oz;   // :422-425
    coarse_unit(sun_x, sun_y, sun_z);
    float dot_prod_ns = (f.norm_x * sun_x + f.norm_y * sun_y) + f.norm_z * sun_z;
    if (REFRAC)
        horisun_refract(p.refrac_fac[cell], f.tilt_x, f.tilt_y, f.tilt_z, f.norm_x, f.norm_y, f.norm_z, sun_x, sun_y, sun_z, dot_prod_ns);
    const float dot_prod_ts = (f.tilt_x * sun_x + f.tilt_y * sun_y) + f.tilt_z * sun_z;
    // the look-up decides the code of every cell with dot_ts > 0, and the value of those with dot_ts > dot_prod_min (> 0)
    if (dot_prod_ts > (CODES ? 0.0f : p.dot_prod_min)) {
        const bool shaded = coarse_shaded<PLANES>(p.hori, cell, p.stride, p.azim_num, per_rad, sun_x, sun_y, sun_z, f);
        lit = shaded ? 0 : 1;
        if (!shaded && dot_prod_ts > p.dot_prod_min) {         // shadow_result
            float d = dot_prod_ns;
            if (d < p.dot_prod_min) d = p.dot_prod_min;
            val = (dot_prod_ts / d) * f.enl;
        }
    }
}

template <bool PLANES, bool CODES, bool VALS, bool REFRAC>
__global__ __launch_bounds__(HZ_HSC_TPB) void k_horisun_coarse(HorisunCoarseArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_hsc[];
    float *const lv = reinterpret_cast<float *>(smem_hsc);
    uint8_t *const lf = smem_hsc + p.off_flags;
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)p.nstrips), strip = (int)(blockIdx.x - (unsigned)I * p.nstrips);
    const int J0 = strip * p.nb, nbc = min(p.nb, p.gx - J0);
    const int W = nbc * p.p1, Wm = p.nb * p.p1;                    // columns of this strip / pitch of a tile row
    const int sp = (int)blockIdx.y * p.q, qc = min(p.q, p.num_sun - sp);   // the pass: positions [sp, sp + qc)
    if (qc <= 0) return;                                            // the same in every lane
    const int aq = tid / p.nb, ab = tid - aq * p.nb;                // adding lane: position aq of the pass, block ab of the strip
    const bool adds = aq < qc && ab < nbc;
    const double per_rad = (double)p.azim_num / 6.283185307179586;
    const float *suns = p.suns + 3 * (size_t)sp;
    double sum = 0.0;                                               // the adding lane's: in registers across the tiles
    unsigned n_lit = 0;
    for (int r0 = 0; r0 < p.p0; r0 += p.rows) {
        const int rc = min(p.rows, p.p0 - r0);
        const int cells_t = rc * W;                                 // <= pitch <= 4096, so pairs <= 8 * 4096
        const size_t cell00 = (size_t)(I * p.p0 + r0) * (size_t)p.dim_1 + (size_t)J0 * (size_t)p.p1;
        // pair x = (position q of the pass, cell e of the tile, row-major over rc rows of W cells)
        for (int x = tid; x < qc * cells_t; x += HZ_HSC_TPB) {
            const int q = x / cells_t, e = x - q * cells_t;
            const int r = e / W, c = e - r * W;
            const size_t cell = cell00 + (size_t)r * (size_t)p.dim_1 + (size_t)c;
            float val = 0.0f;                           // sw_dir_cor: 0 outside ang_max (!(dot_ts > dot_prod_min)) and in shadow
            int lit = 0;
            if (p.mask[cell] == 1) coarse_eval<PLANES, CODES, REFRAC>(p, cell, suns + 3 * q, per_rad, val, lit);
            const int at = q * p.pitch + r * Wm + c;
            if (VALS) lv[at] = val;
            if (CODES) lf[at] = (uint8_t)lit;
        }
        __syncthreads();
        if (adds) {
            for (int r = 0; r < rc; r++) {
                const int at = aq * p.pitch + r * Wm + ab * p.p1;
                for (int dj = 0; dj < p.p1; dj++) {
                    if (VALS) sum += (double)lv[at + dj];
                    if (CODES) n_lit += lf[at + dj];
                }
            }
        }
        __syncthreads();
    }
    if (adds) {
        const int J = J0 + ab;
        const unsigned n = p.n[(size_t)I * p.gx + J];
        const size_t out = ((size_t)(sp + aq) * p.gy + I) * p.gx + J;
        if (VALS) p.f_cor[out] = n ? (float)(sum / (double)n) : p.fill;
        if (CODES) p.lit[out] = n ? (float)((double)n_lit / (double)n) : p.fill;
    }
}

int horisun_coarse_plan_for(int dim_0, int dim_1, int p0, int p1, int chunk, bool planes, bool codes, bool vals,
                            HorisunCoarsePlan *plan) {
    if (horisun_coarse_plan(dim_0, dim_1, p0, p1, chunk, g_horisun_coarse_tile.load(std::memory_order_relaxed), codes, vals, plan))
        return set_error(HZ_ERR_ARG, "too many coarse cells for one launch");
    int route = g_horisun_coarse_route.load(std::memory_order_relaxed);
    if (route < 0) route = k_default_route[planes ? 1 : 0];
    if (route == 1) plan->fallback = 1;
    return HZ_OK;
}

int horisun_coarse_launch(const HorisunArgs &a, bool planes, size_t plane_stride, const HorisunCoarsePlan &plan,
                          const unsigned *n, int dim_1, int p0, int p1, float *f_cor, float *lit, hipStream_t st) {
    if (a.num_sun <= 0) return HZ_OK;
    if (plan.fallback || (!f_cor && !lit) || plan.lds_bytes > 65536)
        return set_error(HZ_ERR_ARG, "horisun_coarse_launch: the plan does not fit the call");
    HorisunCoarseArgs p;
    p.hori = a.hori; p.stride = plane_stride;
    p.vert = a.vert; p.vec_tilt = a.vec_tilt; p.vec_norm = a.vec_norm; p.vec_north = a.vec_north; p.surf_enl_fac = a.surf_enl_fac;
    p.mask = a.mask; p.n = n; p.suns = a.suns; p.num_sun = a.num_sun; p.azim_num = a.azim_num;
    p.fill = a.fill; p.dot_prod_min = a.dot_prod_min;
    p.dim_1 = dim_1; p.p0 = p0; p.p1 = p1; p.gy = plan.gy; p.gx = plan.gx;
    p.nb = plan.nb; p.nstrips = plan.nstrips; p.rows = plan.rows; p.pitch = plan.pitch; p.q = plan.q;
    p.off_flags = plan.off_flags;
    p.f_cor = f_cor; p.lit = lit; p.refrac_fac = a.refrac_fac;
    const dim3 grid(plan.grid_x, horisun_coarse_groups(plan, a.num_sun));
    const size_t lds = plan.lds_bytes;
#define HZ_LAUNCH_HSC(PL, C, V)                                                                                         \
    do {                                                                                                                \
        if (p.refrac_fac) hipLaunchKernelGGL((k_horisun_coarse<PL, C, V, true>), grid, dim3(HZ_HSC_TPB), lds, st, p);   \
        else hipLaunchKernelGGL((k_horisun_coarse<PL, C, V, false>), grid, dim3(HZ_HSC_TPB), lds, st, p);               \
    } while (0)
#define HZ_LAUNCH_HSC_OUT(PL)                                                                                           \
    do {                                                                                                                \
        if (lit && f_cor) HZ_LAUNCH_HSC(PL, true, true);                                                                \
        else if (lit) HZ_LAUNCH_HSC(PL, true, false);                                                                   \
        else HZ_LAUNCH_HSC(PL, false, true);                                                                            \
    } while (0)
    if (planes) HZ_LAUNCH_HSC_OUT(true);
    else HZ_LAUNCH_HSC_OUT(false);
#undef HZ_LAUNCH_HSC_OUT
#undef HZ_LAUNCH_HSC
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
