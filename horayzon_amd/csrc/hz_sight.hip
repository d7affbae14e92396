// hz_sight.hip -- Terrain.sight_height (hz_terrain_sight_height): how high above a cell a target must be to have a free line
// of sight to an observer point, out of a caller's table of heights.
//
// DESIGN.md section 4 clause 19.  One lane per inner-domain cell and observer.  visible(k) is the viewshed's question
// (clause 18, hz_viewshed.hip) for the point H[k] above the surface, without the facing test: one any-hit ray from that
// point to the observer, tfar = the distance.  The lane asks it for the top of the table, then for its bottom, then bisects
// (hz_sight_search.h): up to 2 + ceil(log2(n - 1)) rays per cell.  Refraction is never applied.
//
// k_sight_refill is a __global__ of its own on the shared refill loop (as text, not a template: hz_refill_loop.inc), with one
// difference to k_viewshed_refill: a lane whose ray is decided advances its search and sets up the next ray of the SAME
// cell; only a finished cell frees the lane for the hand-out.
#include "hz_internal.h"
#include "hz_shadow.h"
#include "hz_sight_search.h"

namespace hz {

#define HZ_TPB 256
// resident workgroups per CU the register allocation is held to: k_shadow_refill's bound (hz_shadow.h).  Beyond the viewshed's
// lane a searching lane carries its cell as (i, j), lo | hi << 16, the phase and the index of the next ray.
#ifndef HZ_SIGHT_WG
#define HZ_SIGHT_WG HZ_SHADOW_WG
#endif
// hz_trace is left for a refill when fewer lanes than this still traverse.  Unlike the shadow kernels' lanes a decided lane
// nearly always has a next ray (of its own cell), so the threshold also holds after the last cell is handed out.
#ifndef HZ_SIGHT_REGROUP
#define HZ_SIGHT_REGROUP HZ_SHADOW_REGROUP
#endif

struct SightParams {
    ShadowParams s;          // s.suns = the observers of the launch, s.out_f32 = `height` at the launch's first observer (or null)
    const float *heights;    // f32[n]: finite, strictly increasing, heights[0] >= 0.005 (the driver checked)
    int n;                   // 1 ... 65535
    float max_dist;          // has_max: cells whose lowest target point is farther than this from the observer get +inf
    int has_max;
    unsigned *lowest;        // bits of f32[cells] or null: atomicMin of the finite results (they are positive floats)
    unsigned long long *cells_reached;   // u64[observers of the launch] or null: += the cells with a finite result
};

struct SightRay { float ox, oy, oz, dx, dy, dz, tfar; };

#define HZ_SIGHT_NONE (-2)      // (hz_sight_search.h: SIGHT_DONE, the one value sight_advance never returns)
#define HZ_SIGHT_NAN_BITS 0x7fc00000u
#define HZ_SIGHT_INF_BITS 0x7f800000u

// The ray of visible(k) for cell (i, j) and observer P in `r`: T_k = v + norm * H[k], d = P - T_k, mag, u = d / mag, tfar = mag.
// False when !(mag > 0): visible without a ray.  Every product, sum and quotient is rounded on its own (-ffp-contract=off),
// associated as in viewshed_setup.  The one table load per ray is this function's first line.
__device__ __forceinline__ bool sight_ray(const SightParams &vp, int i, int j, int k, float px, float py, float pz, SightRay &r) {
    const ShadowParams &p = vp.s;
    const float h = vp.heights[k];
    const size_t cell = (size_t)i * p.dim_in_1 + j;
    const float norm_x = p.vec_norm[3 * cell], norm_y = p.vec_norm[3 * cell + 1], norm_z = p.vec_norm[3 * cell + 2];
    const float *v = p.sv.verts + 3 * ((size_t)(i + p.offset_0) * p.sv.d1 + (size_t)(j + p.offset_1));
    const float ox = v[0] + norm_x * h;
    const float oy = v[1] + norm_y * h;
    const float oz = v[2] + norm_z * h;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const float mag = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx / mag; r.dy = dy / mag; r.dz = dz / mag; r.tfar = mag;
    return mag > 0.0f;
}

// A finished cell (k: SIGHT_UNREACHED or a result index as sight_advance packs it): its height to the observer's map, a finite
// one to the minimum over observers; `reached` marks the lane for the wave's tally of cells with a finite result.
__device__ __forceinline__ void sight_result(const SightParams &vp, float *out, size_t cell, int k, bool &reached) {
    const bool finite = k != SIGHT_UNREACHED;
    const float h = vp.heights[finite ? sight_result_index(k) : 0];
    const unsigned bits = finite ? __float_as_uint(h) : HZ_SIGHT_INF_BITS;
    if (out) out[cell] = __uint_as_float(bits);
    if (finite) {
        if (vp.lowest) atomicMin(&vp.lowest[cell], bits);
        reached = true;
    }
}

// COUNT, FAST: hz_refill_loop.inc.  The traversal is the non-LEAN hz_trace with tfar and tfar_box per lane, as in
// k_viewshed_refill.
template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_SIGHT_WG) void k_sight_refill(SightParams vp) {
    const ShadowParams &p = vp.s;
#define HZ_REFILL_OUTPUTS float *const out = HZ_REFILL_OUT_AT(p.out_f32); const int n = vp.n;
#define HZ_REFILL_LANE \
    unsigned tally = 0;                             /* cells with a finite result so far (wave uniform: a scalar register) */ \
    bool reached = false;                           /* this lane finished a cell with a finite result since the last tally */ \
    int ci = 0, cj = 0;                             /* the lane's cell */ \
    int phase = SIGHT_IDLE;                         /* SIGHT_IDLE: the lane has no cell; else a ray of its cell is set up or wanted */ \
    unsigned lohi = 0;                              /* the search bracket (hz_sight_search.h) */ \
    int k = HZ_SIGHT_NONE;                          /* the table index the lane's next ray aims at (>= 0) while it is not set up yet */ \
    SightRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.tfar = 0.0f;
// the lanes marked since the last pass, counted where the whole wave is here (not live across hz_trace)
#define HZ_REFILL_PASS tally += (unsigned)__popcll(__ballot(reached)); reached = false;
#define HZ_REFILL_BUSY (phase != SIGHT_IDLE)
// a masked cell is written at once; the range is judged at the lowest target point
#define HZ_REFILL_TAKE(i, j) \
    const size_t cell = (size_t)i * p.dim_in_1 + j; \
    if (p.mask[cell] != 1) { \
        if (out) out[cell] = __uint_as_float(HZ_SIGHT_NAN_BITS); \
    } else { \
        ci = i; cj = j; \
        bool far = false; \
        if (vp.has_max) { \
            SightRay r0; \
            (void)sight_ray(vp, i, j, 0, pos_x, pos_y, pos_z, r0); \
            far = r0.tfar > vp.max_dist; \
        } \
        k = far ? SIGHT_UNREACHED : sight_begin(phase, lohi, n); \
    }
// The next ray of every lane that wants one: of a cell just taken, or of the cell whose last ray was decided.  A target point
// that is the observer is visible without a ray: the search moves on at once.  Then the lanes that finished without a
// (further) ray: out of range, or the observer is a target point.
#define HZ_REFILL_PREPARE \
    while (sight_is_index(k)) { \
        if (sight_ray(vp, ci, cj, k, pos_x, pos_y, pos_z, r)) { HZ_REFILL_START_RAY(r); k = HZ_SIGHT_NONE; break; } \
        k = sight_advance(phase, lohi, n, true); \
    } \
    if (k != HZ_SIGHT_NONE) { sight_result(vp, out, (size_t)ci * p.dim_in_1 + cj, k, reached); k = HZ_SIGHT_NONE; }
#define HZ_REFILL_TFAR r.tfar
#define HZ_REFILL_TFAR_BOX (r.tfar + 2.0f * p.sv.tau)
#define HZ_REFILL_REGROUP HZ_SIGHT_REGROUP
#define HZ_REFILL_DECIDED(res) \
    k = sight_advance(phase, lohi, n, res != 1); \
    if (!sight_is_index(k)) { sight_result(vp, out, (size_t)ci * p.dim_in_1 + cj, k, reached); k = HZ_SIGHT_NONE; }
#define HZ_REFILL_END \
    tally += (unsigned)__popcll(__ballot(reached)); \
    if (lane == 0 && tally && vp.cells_reached) atomicAdd(&vp.cells_reached[pos], (unsigned long long)tally);
#include "hz_refill_loop.inc"
}

int sight_launch(const Scene *sc, const ShadowArgs &a, const SightArgs &v, hipStream_t st) {
    static void (*const kernels[2][2])(SightParams) = HZ_REFILL_KERNELS(k_sight_refill);
    SightParams vp;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (v.num_heights < 1 || v.num_heights > 65535 || !v.heights) return set_error(HZ_ERR_ARG, "sight_launch: bad height table");
    if (!shadow_config(sc, a, vp.s, lds, grid, fast)) return HZ_OK;
    vp.heights = v.heights; vp.n = v.num_heights;
    vp.max_dist = v.max_dist; vp.has_max = v.has_max;
    vp.lowest = reinterpret_cast<unsigned *>(v.lowest);
    vp.cells_reached = reinterpret_cast<unsigned long long *>(v.cells_reached);
    return refill_launch(kernels, vp, a.count_work, fast, grid, lds, st);
}

// before the first launch of a call: every cell of `lowest` holds the bits of +inf, the neutral element of the minimum
__global__ __launch_bounds__(256) void k_sight_lowest_init(size_t n, unsigned *__restrict__ lowest) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) lowest[c] = HZ_SIGHT_INF_BITS;
}

// after the last launch of a call: masked cells (mask != 1) hold NaN, whatever was there (+inf: no lane took a minimum)
__global__ __launch_bounds__(256) void k_sight_masked(const uint8_t *__restrict__ mask, size_t n, unsigned *__restrict__ lowest) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    if (mask[c] != 1) lowest[c] = HZ_SIGHT_NAN_BITS;
}

int sight_lowest_init_launch(size_t n, float *lowest, hipStream_t st) {
    if (n == 0 || !lowest) return HZ_OK;
    hipLaunchKernelGGL(k_sight_lowest_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, reinterpret_cast<unsigned *>(lowest));
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int sight_masked_launch(const uint8_t *mask, size_t n, float *lowest, hipStream_t st) {
    if (n == 0 || !lowest) return HZ_OK;
    hipLaunchKernelGGL(k_sight_masked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mask, n, reinterpret_cast<unsigned *>(lowest));
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
