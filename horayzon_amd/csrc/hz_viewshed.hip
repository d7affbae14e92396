// hz_viewshed.hip -- Terrain.viewshed (hz_terrain_viewshed): which cells have a free line of sight to an observer point.
//
// DESIGN.md section 4 clause 18.  One lane per inner-domain cell and observer, at most one any-hit ray from the cell's
// target point (the ray origin of the shadow kernels, `target_elev` above the surface) towards the observer, with
// tfar = the distance to it: unlike a sun position the observer is a point of the scene's frame, and terrain behind it
// blocks nothing.  Refraction is never applied.
//
// k_viewshed_refill is a __global__ of its own on the shared refill loop, with a set-up and a result step of its own and a
// tfar per lane (why the loop is shared as text and not as a template: hz_refill_loop.inc).
#include "hz_internal.h"
#include "hz_shadow.h"

namespace hz {

#define HZ_TPB 256
// resident workgroups per CU the register allocation is held to: k_shadow_refill's bound (hz_shadow.h).  The ray carries one
// value more than a shadow ray (tfar) and two fewer (the dot products of sw_dir_cor).
#ifndef HZ_VIEWSHED_WG
#define HZ_VIEWSHED_WG HZ_SHADOW_WG
#endif

struct ViewshedParams {
    ShadowParams s;          // s.suns = the observers of the launch, s.out_u8 = `visible` at the launch's first observer (or null)
    float target_elev;
    float max_dist;          // has_max: cells farther than this from the observer get code 4
    int has_max, facing;
    int *seen_count;         // i32[cells] or null: += 1 per observer with code 0
    unsigned long long *cells_seen;      // u64[observers of the launch] or null: += the cells with code 0
};

struct ViewRay { float ox, oy, oz, dx, dy, dz, tfar; };

#define HZ_VIEW_RAY (-1)
// Steps 1 - 6 of the clause for cell (i, j) and observer P: the code of a cell that needs no ray (3 masked, 4 out of range,
// 0 the observer is the target point, 1 the surface faces away), or HZ_VIEW_RAY with the ray in `r`.  Every product, sum and
// quotient is rounded on its own (-ffp-contract=off), associated as in shadow_setup / vec_unit.
__device__ __forceinline__ int viewshed_setup(const ViewshedParams &vp, int i, int j, float px, float py, float pz, ViewRay &r) {
    const ShadowParams &p = vp.s;
    const size_t cell = (size_t)i * p.dim_in_1 + j;
    if (p.mask[cell] != 1) return 3;
    const float norm_x = p.vec_norm[3 * cell], norm_y = p.vec_norm[3 * cell + 1], norm_z = p.vec_norm[3 * cell + 2];
    const float *v = p.sv.verts + 3 * ((size_t)(i + p.offset_0) * p.sv.d1 + (size_t)(j + p.offset_1));
    const float ox = v[0] + norm_x * vp.target_elev;
    const float oy = v[1] + norm_y * vp.target_elev;
    const float oz = v[2] + norm_z * vp.target_elev;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const float mag = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    if (vp.has_max && mag > vp.max_dist) return 4;
    if (!(mag > 0.0f)) return 0;
    const float ux = dx / mag, uy = dy / mag, uz = dz / mag;
    if (vp.facing) {
        const float tilt_x = p.vec_tilt[3 * cell], tilt_y = p.vec_tilt[3 * cell + 1], tilt_z = p.vec_tilt[3 * cell + 2];
        if (!((tilt_x * ux + tilt_y * uy) + tilt_z * uz > 0.0f)) return 1;
    }
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = ux; r.dy = uy; r.dz = uz; r.tfar = mag;
    return HZ_VIEW_RAY;
}

// A decided cell: its code to the observer's map, a visible one to the per-cell count; `seen` marks the lane for the wave's
// tally of visible cells.
__device__ __forceinline__ void viewshed_result(const ViewshedParams &vp, uint8_t *out_u8, size_t cell, int code, bool &seen) {
    if (out_u8) out_u8[cell] = (uint8_t)code;
    if (code == 0) {
        if (vp.seen_count) atomicAdd(&vp.seen_count[cell], 1);
        seen = true;
    }
}

// COUNT, FAST: hz_refill_loop.inc.  The traversal is the non-LEAN hz_trace, which reads tfar and tfar_box per lane (only the
// LEAN form keeps tfar in a scalar register, hz_min_uniform): a wave's 64 rays end at 64 different distances.
template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_VIEWSHED_WG) void k_viewshed_refill(ViewshedParams vp) {
    const ShadowParams &p = vp.s;
#define HZ_REFILL_OUTPUTS uint8_t *const out_u8 = HZ_REFILL_OUT_AT(p.out_u8);
#define HZ_REFILL_LANE \
    unsigned tally = 0;                             /* cells with code 0 so far (wave uniform: a scalar register) */ \
    bool seen = false;                              /* this lane decided a code 0 since the last tally */ \
    bool ray_active = false; \
    ViewRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.tfar = 0.0f; \
    size_t cell = 0;
// the lanes marked since the last pass, counted where the whole wave is here (not live across hz_trace)
#define HZ_REFILL_PASS tally += (unsigned)__popcll(__ballot(seen)); seen = false;
#define HZ_REFILL_BUSY ray_active
#define HZ_REFILL_TAKE(i, j) \
    const int code = viewshed_setup(vp, i, j, pos_x, pos_y, pos_z, r); \
    if (code == HZ_VIEW_RAY) { cell = (size_t)i * p.dim_in_1 + j; HZ_REFILL_START_RAY(r); ray_active = true; } \
    else viewshed_result(vp, out_u8, (size_t)i * p.dim_in_1 + j, code, seen);
#define HZ_REFILL_PREPARE
#define HZ_REFILL_TFAR r.tfar
#define HZ_REFILL_TFAR_BOX (r.tfar + 2.0f * p.sv.tau)
#define HZ_REFILL_REGROUP ((next < total) ? HZ_SHADOW_REGROUP : 0)
#define HZ_REFILL_DECIDED(res) viewshed_result(vp, out_u8, cell, res == 1 ? 2 : 0, seen); ray_active = false;
#define HZ_REFILL_END \
    tally += (unsigned)__popcll(__ballot(seen)); \
    if (lane == 0 && tally && vp.cells_seen) atomicAdd(&vp.cells_seen[pos], (unsigned long long)tally);
#include "hz_refill_loop.inc"
}

int viewshed_launch(const Scene *sc, const ShadowArgs &a, const ViewshedArgs &v, hipStream_t st) {
    static void (*const kernels[2][2])(ViewshedParams) = HZ_REFILL_KERNELS(k_viewshed_refill);
    ViewshedParams vp;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (!shadow_config(sc, a, vp.s, lds, grid, fast)) return HZ_OK;
    vp.target_elev = v.target_elev; vp.max_dist = v.max_dist; vp.has_max = v.has_max; vp.facing = v.facing;
    vp.seen_count = v.seen_count;
    vp.cells_seen = reinterpret_cast<unsigned long long *>(v.cells_seen);
    return refill_launch(kernels, vp, a.count_work, fast, grid, lds, st);
}

// after the last launch of a call: masked cells (mask != 1) count -1 observers, whatever was added there (nothing)
__global__ __launch_bounds__(256) void k_viewshed_masked(const uint8_t *__restrict__ mask, size_t n, int *__restrict__ seen_count) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    if (mask[c] != 1) seen_count[c] = -1;
}

int viewshed_masked_launch(const uint8_t *mask, size_t n, int32_t *seen_count, hipStream_t st) {
    if (n == 0 || !seen_count) return HZ_OK;
    hipLaunchKernelGGL(k_viewshed_masked, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mask, n, seen_count);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
