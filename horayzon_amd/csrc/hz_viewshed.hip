// hz_viewshed.hip -- Terrain.viewshed (hz_terrain_viewshed): which cells have a free line of sight to an observer point.
//
// DESIGN.md section 4 clause 18.  One lane per inner-domain cell and observer, at most one any-hit ray from the cell's
// target point (the ray origin of the shadow kernels, `target_elev` above the surface) towards the observer, with
// tfar = the distance to it: unlike a sun position the observer is a point of the scene's frame, and terrain behind it
// blocks nothing.  Refraction is never applied.
//
// k_viewshed_refill is k_shadow_refill's loop (hz_shadow.hip) with a set-up and a result step of its own and a tfar per
// lane.  It is a kernel of its own, as k_accum_refill is: k_shadow_refill<false, true> stamps profiles/*.json and its machine
// code must not move.
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

// COUNT, FAST: as k_shadow_refill.  The traversal is the non-LEAN hz_trace, which reads tfar and tfar_box per lane (only the
// LEAN form keeps tfar in a scalar register, hz_min_uniform): a wave's 64 rays end at 64 different distances.
template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_VIEWSHED_WG) void k_viewshed_refill(ViewshedParams vp) {
    const ShadowParams &p = vp.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem + (FAST ? 2 * HZ_TPB * 4 : 0));
    const int tid = threadIdx.x;
    int ti = 0, tj = 0;
    const bool has_tile = hz_tile_of_block(p.tm, blockIdx.x, &ti, &tj);
    const int wave = tid >> 6, lane = tid & 63;
    const int obs_idx = blockIdx.y;
    const float p_x = p.suns[3 * obs_idx], p_y = p.suns[3 * obs_idx + 1], p_z = p.suns[3 * obs_idx + 2];
    uint8_t *const out_u8 = p.out_u8 ? p.out_u8 + (size_t)obs_idx * p.out_stride : nullptr;
    unsigned rays = 0;
    TravCounters tc; tc.nodes = 0; tc.tris = 0; tc.w_nodes = 0; tc.w_leaves = 0;
    const int i_base = ti * 16 + (wave >> 1) * 8, j_base = tj * (16 * p.nb) + (wave & 1) * 8;
    const int total = has_tile ? 64 * p.nb : 0;
    int next = 0;                                   // cells handed out so far (wave uniform)
    unsigned tally = 0;                             // cells with code 0 so far (wave uniform: a scalar register)
    bool seen = false;                              // this lane decided a code 0 since the last tally
    bool ray_active = false;
    ViewRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.tfar = 0.0f;
    size_t cell = 0;
    RayBox rb = hz_raybox(0, 0, 0, 0, 0, 1);
    TravState ts; hz_trav_reset(ts);
    bool overflow = false;
    for (;;) {
        // the lanes marked since the last pass, counted where the whole wave is here (not live across hz_trace)
        tally += (unsigned)__popcll(__ballot(seen));
        seen = false;
        if (next < total) {
            const unsigned long long need = __ballot(!ray_active);
            if (need != 0ull) {
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                const int my = next + rank;
                next += __popcll(need);
                if (!ray_active && my < total) {
                    const int i = i_base + ((my & 63) >> 3), j = j_base + (my >> 6) * 16 + (my & 7);
                    if (i < p.dim_in_0 && j < p.dim_in_1) {
                        const int code = viewshed_setup(vp, i, j, p_x, p_y, p_z, r);
                        if (code == HZ_VIEW_RAY) {
                            cell = (size_t)i * p.dim_in_1 + j;
                            // (box tests start at -tau and end at tfar + tau: hz_common.h)
                            rb = hz_raybox((r.ox - p.sv.cx) - p.sv.tau * r.dx, (r.oy - p.sv.cy) - p.sv.tau * r.dy, (r.oz - p.sv.cz) - p.sv.tau * r.dz,
                                           r.dx, r.dy, r.dz);
                            hz_trav_reset(ts);
                            overflow = false;
                            ray_active = true;
                            rays++;
                        } else {
                            viewshed_result(vp, out_u8, (size_t)i * p.dim_in_1 + j, code, seen);
                        }
                    }
                }
            }
        }
        if (__ballot(ray_active) == 0ull) {
            if (next >= total) break;
            continue;
        }
        if (ray_active) {
            const float tfar_box = r.tfar + 2.0f * p.sv.tau;
            int res = hz_trace<HZ_TPB, COUNT, 2, false, !FAST>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                    r.tfar, tfar_box, rb, ts, (next < total) ? HZ_SHADOW_REGROUP : 0, HZ_SHADOW_LEAF_BIAS, tc, p.stack_cap, overflow);
            if (FAST && res != 2 && overflow) {
                bool unused = false;
                hz_trav_reset(ts);
                res = hz_trace<HZ_TPB, COUNT, 2, false, true>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                                    r.tfar, tfar_box, rb, ts, 0, HZ_SHADOW_LEAF_BIAS, tc, 0, unused);
                if (COUNT && p.counters) atomicAdd(&p.counters[HZ_SHADOW_CNT_TWICE], 1ull);     // rays traced twice
            }
            if (res != 2) {
                viewshed_result(vp, out_u8, cell, res == 1 ? 2 : 0, seen);
                ray_active = false;
            }
        }
    }
    tally += (unsigned)__popcll(__ballot(seen));
    if (lane == 0 && tally && vp.cells_seen) atomicAdd(&vp.cells_seen[obs_idx], (unsigned long long)tally);
    shadow_counters<COUNT>(p, rays, tc, lane);
}

#define HZ_LAUNCH_REFILL(K, P) do { \
        HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(K, grid, dim3(HZ_TPB), lds, st, P); } while (0)

int viewshed_launch(const Scene *sc, const ShadowArgs &a, const ViewshedArgs &v, hipStream_t st) {
    ViewshedParams vp;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (!shadow_config(sc, a, vp.s, lds, grid, fast)) return HZ_OK;
    vp.target_elev = v.target_elev; vp.max_dist = v.max_dist; vp.has_max = v.has_max; vp.facing = v.facing;
    vp.seen_count = v.seen_count;
    vp.cells_seen = reinterpret_cast<unsigned long long *>(v.cells_seen);
    if (fast) { if (a.count_work) HZ_LAUNCH_REFILL((k_viewshed_refill<true, true>), vp); else HZ_LAUNCH_REFILL((k_viewshed_refill<false, true>), vp); }
    else { if (a.count_work) HZ_LAUNCH_REFILL((k_viewshed_refill<true, false>), vp); else HZ_LAUNCH_REFILL((k_viewshed_refill<false, false>), vp); }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}
#undef HZ_LAUNCH_REFILL

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
