// hz_shadow.hip -- shadow mask / direct-shortwave correction kernels for gfx950.
//
// Replaces CppTerrain::shadow and CppTerrain::sw_dir_cor (shadow_comp.cpp:386-491,
// :495-605): one lane per inner-domain cell, at most one any-hit ray with
// tfar = infinity towards the sun (optionally bent by atmospheric refraction,
// shadow_comp.cpp:430-446).  Same tile / XCD mapping and LDS staging as the horizon
// kernel; the BVH is persistent in the Terrain handle (built once, :318-380).
#include "hz_internal.h"
#include "hz_shadow.h"
#include "hz_crmath.h"
#include <cstdlib>

namespace hz {

#define HZ_TPB 256
// The float libm calls of the reference's refraction branch (acos / tan / pow / cos / sin on float arguments
// resolve to the float overloads, shadow_comp.cpp:19): self-contained correctly rounded versions shared with
// the CPU oracle (hz_crmath.h): with refraction, shadow codes and sw_dir_cor are bit-identical TO THAT CONTRACT (the
// correctly rounded float), not to the reference's glibc calls -- tests/test_gpu_parity.py::
// test_refraction_against_platform_libm measures the distance to the platform libm (a tolerance, not equality).
__device__ __forceinline__ float f_acos(float x) { return hz_crm_acosf(x); }
__device__ __forceinline__ float f_tan(float x) { return hz_crm_tanf(x); }
__device__ __forceinline__ float f_cos(float x) { return hz_crm_cosf(x); }
__device__ __forceinline__ float f_sin(float x) { return hz_crm_sinf(x); }
__device__ __forceinline__ float f_pow(float x, float y) { return hz_crm_powf(x, y); }

// shadow_comp.cpp:43-62: float in, double arithmetic, float out.  The divisions by the two constants are the correctly rounded
// quotients in four instructions each (hz_crmath.h: hz_crm_div_const)
__device__ __forceinline__ float deg2rad_f(float a) {
    return (float)(hz_crm_div_const((double)a, 180.0, 1.0 / 180.0) * 3.14159265358979323846);
}
__device__ __forceinline__ float rad2deg_f(float a) {
    return (float)(hz_crm_div_const((double)a, 3.14159265358979323846, 1.0 / 3.14159265358979323846) * 180.0);
}

// shadow_comp.cpp:135-159 (Saemundsson), float/double promotions as there.  `fac` = the factor that depends on the cell's
// pressure and temperature only: ((double)pressure / 101.0) * (283.0 / (273.0 + (double)temp)) (:156), formed once per cell
// at Terrain::initialise (k_refrac_factor) -- the same float64 value the expression yields here
__device__ __forceinline__ float atmos_refrac(float elev_ang_true, double fac) {
    elev_ang_true = __builtin_fmaxf(-1.0f, __builtin_fminf(elev_ang_true, 90.0f));
    float refrac_cor = (float)(1.02 / (double)f_tan(deg2rad_f(
        (float)((double)elev_ang_true + 10.3 / ((double)elev_ang_true + 5.11)))));
    refrac_cor = (float)((double)refrac_cor + 0.0019279);
    refrac_cor = (float)((double)refrac_cor * fac);
    return (float)((double)refrac_cor * (1.0 / 60.0));
}

// :438-441 and the pressure / temperature factor of :156, per cell
__global__ __launch_bounds__(256) void k_refrac_factor(const float *__restrict__ elevation, size_t n, double *__restrict__ out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const float temperature_ref = 283.15f, pressure_ref = 101.0f, lapse_rate = 0.0065f;
    const float g = 9.81f, R_d = 287.0f;
    const float expo = g / (R_d * lapse_rate);                 // :353-354
    const float temperature = temperature_ref - (lapse_rate * elevation[c]);
    const float pressure = pressure_ref * f_pow(temperature / temperature_ref, expo);
    const float temp = (float)((double)temperature - 273.15);  // K2degC, :146-148
    out[c] = ((double)pressure / 101.0) * (283.0 / (273.0 + (double)temp));
}

int shadow_refrac_factor(const float *elevation, size_t n, double *out, hipStream_t st) {
    if (n == 0) return HZ_OK;
    hipLaunchKernelGGL(k_refrac_factor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, elevation, n, out);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

// Per-cell set-up shared by both kernels: classification without a ray (masked / self-shaded / outside ang_max) is
// written at once; otherwise the ray (origin, direction) and the two dot products come back and 1 is returned.
struct ShadowRay { float ox, oy, oz, dx, dy, dz, dot_ts, dot_ns; };

__device__ __forceinline__ int shadow_setup(const ShadowParams &p, int i, int j, float p_sun_x, float p_sun_y, float p_sun_z,
                                            uint8_t *out_u8, float *out_f32, ShadowRay &r) {
    const size_t cell = (size_t)i * p.dim_in_1 + j;
    if (p.mask[cell] != 1) {                                       // shadow_comp.cpp:480-484 / :594-598
        if (p.which == 0) out_u8[cell] = 3; else out_f32[cell] = p.fill;
        return 0;
    }
    const float tilt_x = p.vec_tilt[3 * cell], tilt_y = p.vec_tilt[3 * cell + 1], tilt_z = p.vec_tilt[3 * cell + 2];
    const float norm_x = p.vec_norm[3 * cell], norm_y = p.vec_norm[3 * cell + 1], norm_z = p.vec_norm[3 * cell + 2];
    const float ray_org_elev = 0.05f;                              // :388, :497
    const float *v = p.sv.verts + 3 * ((size_t)(i + p.offset_0) * p.sv.d1 + (size_t)(j + p.offset_1));
    const float ox = v[0] + norm_x * ray_org_elev;
    const float oy = v[1] + norm_y * ray_org_elev;
    const float oz = v[2] + norm_z * ray_org_elev;
    float sun_x = p_sun_x - ox, sun_y = p_sun_y - oy, sun_z = p_sun_z - oz;   // :422-425
    vec_unit(sun_x, sun_y, sun_z);
    float dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
    if (p.refrac == 1) {                                           // :430-446
        const double fac = p.refrac_fac[cell];
        // The refraction turns the sun direction about an axis normal to it by theta <= 38.81' * fac (the formula's value at
        // the clamp -1 deg, where it is largest) = 0.01129 * fac rad: tilt . sun changes by less than |tilt| * theta.  A cell
        // whose tilted surface faces away from the unrefracted sun by more than that is self-shaded (`!(dot > 0)` below,
        // and `!(dot > dot_prod_min)` with dot_prod_min > 0) whatever the refraction is: night positions and back slopes
        // skip the five libm calls.  (NaN factor: the comparison is false, the full path runs.)
        {
            const float dot0 = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
            const float tl = __builtin_fmaxf((tilt_x * tilt_x + tilt_y * tilt_y) + tilt_z * tilt_z, 1.0f);     // >= |tilt|
            const float bound = (0.0114f * __builtin_fabsf((float)fac)) * tl * 1.01f + 1.0e-5f;
            if (dot0 < -bound) {
                if (p.which == 0) out_u8[cell] = 1; else out_f32[cell] = 0.0f;
                return 0;
            }
        }
        const float elev_ang_true = (float)(90.0 - (double)rad2deg_f(f_acos(dot_prod_ns)));
        const float refrac_cor = atmos_refrac(elev_ang_true, fac);
        float k_x = sun_y * norm_z - sun_z * norm_y;
        float k_y = sun_z * norm_x - sun_x * norm_z;
        float k_z = sun_x * norm_y - sun_y * norm_x;
        vec_unit(k_x, k_y, k_z);
        const float theta = deg2rad_f(refrac_cor);                // vec_rot, :109-132
        const float ct = f_cos(theta), st = f_sin(theta);
        const float part = (float)((double)((k_x * sun_x + k_y * sun_y) + k_z * sun_z) * (1.0 - (double)ct));
        const float rx = (sun_x * ct + (k_y * sun_z - k_z * sun_y) * st) + k_x * part;
        const float ry = (sun_y * ct + (k_z * sun_x - k_x * sun_z) * st) + k_y * part;
        const float rz = (sun_z * ct + (k_x * sun_y - k_y * sun_x) * st) + k_z * part;
        sun_x = rx; sun_y = ry; sun_z = rz;
        dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
    }
    const float dot_prod_ts = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
    if (p.which == 0) {                                            // :451-478
        if (!(dot_prod_ts > 0.0f)) { out_u8[cell] = 1; return 0; }
    } else {                                                       // :561-592
        if (!(dot_prod_ts > p.dot_prod_min)) { out_f32[cell] = 0.0f; return 0; }
    }
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = sun_x; r.dy = sun_y; r.dz = sun_z;
    r.dot_ts = dot_prod_ts; r.dot_ns = dot_prod_ns;
    return 1;
}

__device__ __forceinline__ void shadow_result(const ShadowParams &p, size_t cell, bool hit, const ShadowRay &r,
                                              uint8_t *out_u8, float *out_f32) {
    if (p.which == 0) { out_u8[cell] = hit ? 2 : 0; return; }
    if (hit) { out_f32[cell] = 0.0f; return; }
    float dot_prod_ns = r.dot_ns;
    if (dot_prod_ns < p.dot_prod_min) dot_prod_ns = p.dot_prod_min;
    out_f32[cell] = (r.dot_ts / dot_prod_ns) * p.surf_enl_fac[cell];
}


#ifndef HZ_SHADOW_FAST_CAP_DEFAULT
#define HZ_SHADOW_FAST_CAP_DEFAULT 19   // 21 KiB of LDS per workgroup: 7 resident; round 4: level stack 1.074 -> fast stack 0.964 ms per position at 5 workgroups (profiles/r04/ab_shadow_fast_stack.log)
#endif
// k_shadow_refill: the refill loop (hz_refill_loop.inc: the scheme, COUNT and FAST) with at most one ray per cell towards the
// sun, tfar = infinity.
template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_SHADOW_WG) void k_shadow_refill(ShadowParams p) {
#define HZ_REFILL_OUTPUTS uint8_t *const out_u8 = HZ_REFILL_OUT_AT(p.out_u8); float *const out_f32 = HZ_REFILL_OUT_AT(p.out_f32);
#define HZ_REFILL_LANE \
    bool ray_active = false; \
    ShadowRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.dot_ts = r.dot_ns = 0.0f; \
    size_t cell = 0;
#define HZ_REFILL_PASS
#define HZ_REFILL_BUSY ray_active
#define HZ_REFILL_TAKE(i, j) \
    if (shadow_setup(p, i, j, pos_x, pos_y, pos_z, out_u8, out_f32, r)) { cell = (size_t)i * p.dim_in_1 + j; HZ_REFILL_START_RAY(r); ray_active = true; }
#define HZ_REFILL_PREPARE
#define HZ_REFILL_TFAR __builtin_inff()
#define HZ_REFILL_TFAR_BOX __builtin_inff()
#define HZ_REFILL_REGROUP ((next < total) ? HZ_SHADOW_REGROUP : 0)      // while cells are left
#define HZ_REFILL_DECIDED(res) shadow_result(p, cell, res == 1, r, out_u8, out_f32); ray_active = false;
#define HZ_REFILL_END
#include "hz_refill_loop.inc"
}

std::atomic<int> g_shadow_fast_cap{HZ_SHADOW_FAST_CAP_DEFAULT};      // hz_debug_set (hz_internal.h)
std::atomic<int> g_topo_wide{0};
std::atomic<int> g_accum_chunk{0};

// Launch configuration of the refill kernels (hz_shadow.h)
int shadow_config(const Scene *sc, const ShadowArgs &a, ShadowParams &p, size_t &lds, dim3 &grid, bool &fast) {
    p.sv = scene_view(sc);
    p.vec_tilt = a.vec_tilt; p.vec_norm = a.vec_norm; p.surf_enl_fac = a.surf_enl_fac; p.elevation = a.elevation;
    p.mask = a.mask;
    p.offset_0 = a.offset_0; p.offset_1 = a.offset_1; p.dim_in_0 = a.dim_in_0; p.dim_in_1 = a.dim_in_1;
    if (a.dim_in_0 <= 0 || a.dim_in_1 <= 0) return 0;
    const int tiles_i = (a.dim_in_0 + 15) / 16;
    p.tm = make_tile_map(tiles_i, (a.dim_in_1 + 15) / 16);
    p.suns = a.suns; p.out_stride = (size_t)a.dim_in_0 * (size_t)a.dim_in_1;
    if (a.num_sun <= 0) return 0;
    p.fill = a.sw_dir_cor_fill; p.dot_prod_min = a.dot_prod_min;
    p.refrac = (a.refrac_cor && a.refrac_fac != nullptr) ? 1 : 0; p.which = a.which; p.refrac_fac = a.refrac_fac;
    p.out_u8 = a.out_u8; p.out_f32 = a.out_f32;
    // LDS stack: one entry per tree level (hz_common.h): 12 - 14 KB per workgroup, so the VGPRs decide the residency
    p.stack_bytes = std::max(sc->hdr.height, 1) * HZ_TPB * 4;
    p.top_nodes = 0;
    p.counters = a.counters;
    // fast stack (k_shadow_refill<.., true>): HZ_SHADOW_FAST_CAP entries (0: off) behind two padding rows, if the level
    // stack of the in-kernel retry fits into them
    const int fast_cap_env = g_shadow_fast_cap.load(std::memory_order_relaxed);      // (hz_debug_set("shadow_fast_cap", n): tests)
    const int height = std::max(sc->hdr.height, 1);
    const int fast_cap = std::min(fast_cap_env, 3 * height + 1);
    fast = fast_cap >= 5 && fast_cap >= height;
    p.stack_cap = fast ? fast_cap : 0;
    lds = fast ? (size_t)(fast_cap + 2) * HZ_TPB * 4 : (size_t)p.stack_bytes;
    // blocks per wave: as many as leave >= ~48 workgroups per CU over the whole launch (measured on the 3601^2 tile, 144
    // positions per launch: 2 / 4 / 8 / 16 / 32 / 64 blocks -> 1.64 / 1.49 / 1.42 / 1.36 / 1.29 / 1.51 ms per position; a single
    // position: 1 / 2 / 4 / 8 / 16 blocks -> 2.49 / 1.77 / 1.67 / 1.65 / 1.79 ms, k_shadow 2.52 ms)
    {
        const int tiles_j = (a.dim_in_1 + 15) / 16;
        const double wgs = (double)tiles_i * tiles_j * (double)a.num_sun;
        int nb = (int)(wgs / (48.0 * 256.0));
        nb = std::max(1, std::min(std::min(nb, 32), tiles_j));
        // a count that cuts the tile row without a ragged last super tile if there is one nearby (224 tiles: 24 blocks per
        // wave measured 1.41 ms, 32 blocks 1.29 ms per position)
        for (int c = nb; c >= std::max(1, (nb * 3) / 4); c--)
            if (tiles_j % c == 0) { nb = c; break; }
        p.nb = nb;
        p.tm = make_tile_map(tiles_i, (tiles_j + nb - 1) / nb);
    }
    // grid.x is a multiple of 8, so the workgroup -> XCD assignment (flat id % 8) is the same for every grid.y row
    grid = dim3((unsigned)(p.tm.per_xcd * 8), (unsigned)a.num_sun);
    return 1;
}

int shadow_launch(const Scene *sc, const ShadowArgs &a, hipStream_t st) {
    static void (*const kernels[2][2])(ShadowParams) = HZ_REFILL_KERNELS(k_shadow_refill);
    ShadowParams p;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (!shadow_config(sc, a, p, lds, grid, fast)) return HZ_OK;
    return refill_launch(kernels, p, a.count_work, fast, grid, lds, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Terrain.accumulate (hz_terrain_accumulate): weighted sums over many sun positions without a map per position.
//
// Positions go in chunks of K.  k_accum_refill traces one chunk into scratch [K][cells] -- with the sunlit sum wanted, the
// shadow code (u8; which = 0: one ray per cell with dot_ts > 0, the shadow_batch ray set) and, if the correction sum is also
// wanted, the correction factor of the lit cells (f32); with the correction sum alone, the correction factor (which = 1:
// one ray per cell with dot_ts > dot_prod_min, the sw_dir_cor_batch ray set).  Because dot_prod_min > 0 (ang_max <= 89.99)
// the second ray set is a subset of the first and one ray serves both sums.  k_accum_add then adds the chunk to per-cell
// float64 accumulators in ascending position order, and k_accum_final rounds them to float32 once and writes the fill
// value to masked cells.
//
// k_accum_refill is a __global__ of its own on the shared loop, k_shadow_refill's hooks with another result step (why the
// loop is shared as text, not as a template parameter of k_shadow_refill: hz_refill_loop.inc).
struct AccumParams {
    ShadowParams s;          // s.which = 0: shadow codes to s.out_u8 (+ correction of the lit cells to s.out_f32); 1: correction only
    int want_sw;             // s.which == 0: also write the correction factor
};

// result of a traced ray: the code and value Terrain.shadow / Terrain.sw_dir_cor give for the cell (shadow_result)
__device__ __forceinline__ void accum_result(const AccumParams &p, size_t cell, bool hit, const ShadowRay &r,
                                             uint8_t *out_u8, float *out_f32) {
    if (p.s.which != 0) { shadow_result(p.s, cell, hit, r, out_u8, out_f32); return; }
    out_u8[cell] = hit ? 2 : 0;
    if (!p.want_sw || hit) return;        // (k_accum_add reads the correction of code-0 cells only)
    float v = 0.0f;                       // a lit cell with dot_ts <= dot_prod_min: shadow_setup's which = 1 branch
    if (r.dot_ts > p.s.dot_prod_min) {
        float dot_prod_ns = r.dot_ns;
        if (dot_prod_ns < p.s.dot_prod_min) dot_prod_ns = p.s.dot_prod_min;
        v = (r.dot_ts / dot_prod_ns) * p.s.surf_enl_fac[cell];
    }
    out_f32[cell] = v;
}

template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_SHADOW_WG) void k_accum_refill(AccumParams ap) {
    const ShadowParams &p = ap.s;
#define HZ_REFILL_OUTPUTS uint8_t *const out_u8 = HZ_REFILL_OUT_AT(p.out_u8); float *const out_f32 = HZ_REFILL_OUT_AT(p.out_f32);
#define HZ_REFILL_LANE \
    bool ray_active = false; \
    ShadowRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.dot_ts = r.dot_ns = 0.0f; \
    size_t cell = 0;
#define HZ_REFILL_PASS
#define HZ_REFILL_BUSY ray_active
#define HZ_REFILL_TAKE(i, j) \
    if (shadow_setup(p, i, j, pos_x, pos_y, pos_z, out_u8, out_f32, r)) { cell = (size_t)i * p.dim_in_1 + j; HZ_REFILL_START_RAY(r); ray_active = true; }
#define HZ_REFILL_PREPARE
#define HZ_REFILL_TFAR __builtin_inff()
#define HZ_REFILL_TFAR_BOX __builtin_inff()
#define HZ_REFILL_REGROUP ((next < total) ? HZ_SHADOW_REGROUP : 0)
#define HZ_REFILL_DECIDED(res) accum_result(ap, cell, res == 1, r, out_u8, out_f32); ray_active = false;
#define HZ_REFILL_END
#include "hz_refill_loop.inc"
}

int accum_trace_launch(const Scene *sc, const ShadowArgs &a, int want_sw, hipStream_t st) {
    static void (*const kernels[2][2])(AccumParams) = HZ_REFILL_KERNELS(k_accum_refill);
    AccumParams ap;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (!shadow_config(sc, a, ap.s, lds, grid, fast)) return HZ_OK;
    ap.want_sw = want_sw;
    return refill_launch(kernels, ap, a.count_work, fast, grid, lds, st);
}

// One chunk of k positions into the accumulators, ascending in the position: acc += (double)w * (double)value, the product of
// two floats exact in float64.  codes != null: the sunlit sum adds w * [code == 0], the correction sum w * (code == 0 ?
// value : 0) (the value is written for lit cells only); codes == null: the correction sum adds w * value.  w == null: 1.
__global__ __launch_bounds__(256) void k_accum_add(const uint8_t *__restrict__ codes, const float *__restrict__ vals, size_t n,
                                                   int k, const float *__restrict__ w, double *__restrict__ acc_sw,
                                                   double *__restrict__ acc_lit) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    double s = acc_sw ? acc_sw[c] : 0.0, l = acc_lit ? acc_lit[c] : 0.0;
    for (int q = 0; q < k; q++) {
        const double wq = w ? (double)w[q] : 1.0;
        const size_t at = (size_t)q * n + c;
        if (codes) {
            const bool lit = codes[at] == 0;
            if (acc_lit) l += wq * (lit ? 1.0 : 0.0);
            if (acc_sw) s += wq * (double)(lit ? vals[at] : 0.0f);
        } else {
            s += wq * (double)vals[at];
        }
    }
    if (acc_sw) acc_sw[c] = s;
    if (acc_lit) acc_lit[c] = l;
}

// float32 once at the end; masked cells (mask != 1) get the fill value whatever was accumulated there
__global__ __launch_bounds__(256) void k_accum_final(const uint8_t *__restrict__ mask, size_t n, float fill,
                                                     const double *__restrict__ acc_sw, const double *__restrict__ acc_lit,
                                                     float *__restrict__ out_sw, float *__restrict__ out_lit) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool on = mask[c] == 1;
    if (out_sw) out_sw[c] = on ? (float)acc_sw[c] : fill;
    if (out_lit) out_lit[c] = on ? (float)acc_lit[c] : fill;
}

int accum_add_launch(const uint8_t *codes, const float *vals, size_t n, int k, const float *w, double *acc_sw, double *acc_lit,
                     hipStream_t st) {
    if (n == 0 || k <= 0) return HZ_OK;
    hipLaunchKernelGGL(k_accum_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, codes, vals, n, k, w, acc_sw, acc_lit);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int accum_final_launch(const uint8_t *mask, size_t n, float fill, const double *acc_sw, const double *acc_lit, float *out_sw,
                       float *out_lit, hipStream_t st) {
    if (n == 0) return HZ_OK;
    hipLaunchKernelGGL(k_accum_final, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mask, n, fill, acc_sw, acc_lit, out_sw, out_lit);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
