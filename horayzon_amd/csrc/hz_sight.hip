// hz_sight.hip -- Terrain.sight_height (hz_terrain_sight_height): how high above a cell a target must be to have a free line
// of sight to an observer point, out of a caller's table of heights.
//
// DESIGN.md section 4 clause 19.  One lane per inner-domain cell and observer.  visible(k) is the viewshed's question
// (clause 18, hz_viewshed.hip) for the point H[k] above the surface, without the facing test: one any-hit ray from that
// point to the observer, tfar = the distance.  The lane asks it for the top of the table, then for its bottom, then bisects
// (hz_sight_search.h): up to 2 + ceil(log2(n - 1)) rays per cell.  Refraction is never applied.
//
// k_sight_refill is k_viewshed_refill's loop with one difference: a lane whose ray is decided advances its search and sets
// up the next ray of the SAME cell; only a finished cell frees the lane for the hand-out.  It is a kernel of its own, in a
// file of its own: the machine code of the other refill kernels must not move.
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

// COUNT, FAST: as k_shadow_refill.  The traversal is the non-LEAN hz_trace with tfar and tfar_box per lane, as in
// k_viewshed_refill.
template <bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB, COUNT ? 5 : HZ_SIGHT_WG) void k_sight_refill(SightParams vp) {
    const ShadowParams &p = vp.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem + (FAST ? 2 * HZ_TPB * 4 : 0));
    const int tid = threadIdx.x;
    int ti = 0, tj = 0;
    const bool has_tile = hz_tile_of_block(p.tm, blockIdx.x, &ti, &tj);
    const int wave = tid >> 6, lane = tid & 63;
    const int obs_idx = blockIdx.y;
    const float p_x = p.suns[3 * obs_idx], p_y = p.suns[3 * obs_idx + 1], p_z = p.suns[3 * obs_idx + 2];
    float *const out = p.out_f32 ? p.out_f32 + (size_t)obs_idx * p.out_stride : nullptr;
    const int n = vp.n;
    unsigned rays = 0;
    TravCounters tc; tc.nodes = 0; tc.tris = 0; tc.w_nodes = 0; tc.w_leaves = 0;
    const int i_base = ti * 16 + (wave >> 1) * 8, j_base = tj * (16 * p.nb) + (wave & 1) * 8;
    const int total = has_tile ? 64 * p.nb : 0;
    int next = 0;                                   // cells handed out so far (wave uniform)
    unsigned tally = 0;                             // cells with a finite result so far (wave uniform: a scalar register)
    bool reached = false;                           // this lane finished a cell with a finite result since the last tally
    int ci = 0, cj = 0;                             // the lane's cell
    int phase = SIGHT_IDLE;                         // SIGHT_IDLE: the lane has no cell; else a ray of its cell is set up or wanted
    unsigned lohi = 0;                              // the search bracket (hz_sight_search.h)
    int k = HZ_SIGHT_NONE;                          // the table index the lane's next ray aims at (>= 0) while it is not set up yet
    SightRay r; r.ox = r.oy = r.oz = 0.0f; r.dx = r.dy = 0.0f; r.dz = 1.0f; r.tfar = 0.0f;
    RayBox rb = hz_raybox(0, 0, 0, 0, 0, 1);
    TravState ts; hz_trav_reset(ts);
    bool overflow = false;
    for (;;) {
        // the lanes marked since the last pass, counted where the whole wave is here (not live across hz_trace)
        tally += (unsigned)__popcll(__ballot(reached));
        reached = false;
        if (next < total) {
            const unsigned long long need = __ballot(phase == SIGHT_IDLE);
            if (need != 0ull) {
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                const int my = next + rank;
                next += __popcll(need);
                if (phase == SIGHT_IDLE && my < total) {
                    const int i = i_base + ((my & 63) >> 3), j = j_base + (my >> 6) * 16 + (my & 7);
                    if (i < p.dim_in_0 && j < p.dim_in_1) {
                        const size_t cell = (size_t)i * p.dim_in_1 + j;
                        if (p.mask[cell] != 1) {
                            if (out) out[cell] = __uint_as_float(HZ_SIGHT_NAN_BITS);
                        } else {
                            ci = i; cj = j;
                            bool far = false;
                            if (vp.has_max) {               // the range is judged at the lowest target point
                                SightRay r0;
                                (void)sight_ray(vp, i, j, 0, p_x, p_y, p_z, r0);
                                far = r0.tfar > vp.max_dist;
                            }
                            k = far ? SIGHT_UNREACHED : sight_begin(phase, lohi, n);
                        }
                    }
                }
            }
        }
        // The next ray of every lane that wants one: of a cell just taken, or of the cell whose last ray was decided below.  A
        // target point that is the observer is visible without a ray: the search moves on at once.
        while (sight_is_index(k)) {
            if (sight_ray(vp, ci, cj, k, p_x, p_y, p_z, r)) {
                // (box tests start at -tau and end at tfar + tau: hz_common.h)
                rb = hz_raybox((r.ox - p.sv.cx) - p.sv.tau * r.dx, (r.oy - p.sv.cy) - p.sv.tau * r.dy, (r.oz - p.sv.cz) - p.sv.tau * r.dz,
                               r.dx, r.dy, r.dz);
                hz_trav_reset(ts);
                overflow = false;
                rays++;
                k = HZ_SIGHT_NONE;
                break;
            }
            k = sight_advance(phase, lohi, n, true);
        }
        if (k != HZ_SIGHT_NONE) {                    // finished without a (further) ray: out of range, or the observer is a target point
            sight_result(vp, out, (size_t)ci * p.dim_in_1 + cj, k, reached);
            k = HZ_SIGHT_NONE;
        }
        if (__ballot(phase != SIGHT_IDLE) == 0ull) {
            if (next >= total) break;
            continue;
        }
        if (phase != SIGHT_IDLE) {
            const float tfar_box = r.tfar + 2.0f * p.sv.tau;
            int res = hz_trace<HZ_TPB, COUNT, 2, false, !FAST>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                    r.tfar, tfar_box, rb, ts, HZ_SIGHT_REGROUP, HZ_SHADOW_LEAF_BIAS, tc, p.stack_cap, overflow);
            if (FAST && res != 2 && overflow) {
                bool unused = false;
                hz_trav_reset(ts);
                res = hz_trace<HZ_TPB, COUNT, 2, false, true>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz,
                                                                    r.tfar, tfar_box, rb, ts, 0, HZ_SHADOW_LEAF_BIAS, tc, 0, unused);
                if (COUNT && p.counters) atomicAdd(&p.counters[HZ_SHADOW_CNT_TWICE], 1ull);     // rays traced twice
            }
            if (res != 2) {
                k = sight_advance(phase, lohi, n, res != 1);
                if (!sight_is_index(k)) {
                    sight_result(vp, out, (size_t)ci * p.dim_in_1 + cj, k, reached);
                    k = HZ_SIGHT_NONE;
                }
            }
        }
    }
    tally += (unsigned)__popcll(__ballot(reached));
    if (lane == 0 && tally && vp.cells_reached) atomicAdd(&vp.cells_reached[obs_idx], (unsigned long long)tally);
    shadow_counters<COUNT>(p, rays, tc, lane);
}

#define HZ_LAUNCH_REFILL(K, P) do { \
        HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL(K, grid, dim3(HZ_TPB), lds, st, P); } while (0)

int sight_launch(const Scene *sc, const ShadowArgs &a, const SightArgs &v, hipStream_t st) {
    SightParams vp;
    size_t lds = 0; dim3 grid; bool fast = false;
    if (v.num_heights < 1 || v.num_heights > 65535 || !v.heights) return set_error(HZ_ERR_ARG, "sight_launch: bad height table");
    if (!shadow_config(sc, a, vp.s, lds, grid, fast)) return HZ_OK;
    vp.heights = v.heights; vp.n = v.num_heights;
    vp.max_dist = v.max_dist; vp.has_max = v.has_max;
    vp.lowest = reinterpret_cast<unsigned *>(v.lowest);
    vp.cells_reached = reinterpret_cast<unsigned long long *>(v.cells_reached);
    if (fast) { if (a.count_work) HZ_LAUNCH_REFILL((k_sight_refill<true, true>), vp); else HZ_LAUNCH_REFILL((k_sight_refill<false, true>), vp); }
    else { if (a.count_work) HZ_LAUNCH_REFILL((k_sight_refill<true, false>), vp); else HZ_LAUNCH_REFILL((k_sight_refill<false, false>), vp); }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}
#undef HZ_LAUNCH_REFILL

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
