// hz_cast.hip -- Terrain.cast (hz_terrain_cast): any-hit and closest-hit for rays the caller supplies (gfx950; DESIGN.md
// section 4, clause 21).
//
// A ray is an origin with a unit direction and the call's max_dist, or an origin with a target: then the direction is
// (target - origin) / |target - origin| and the ray ends at the target (clause 18's steps 2, 4 and 5); a target on its origin
// gives no ray.  Nothing is wave uniform: origin, direction and tfar are per lane.  Three kernels, all over one chunk of the
// call's rays:
//
//   k_cast_closest<WANT_POINT, SEGMENTS>  `dist` or `point` is asked.  k_panorama's organisation: one wave = one workgroup,
//       64 consecutive rays of the chunk (of its sorted order, if there is one), the front-to-back closest hit of
//       hz_closest_order.h on a stack of individual child links in LDS (3 x height x 64 x 4 B, no barrier).  `occluded` is the
//       traversal's `hit`.
//   k_cast_any<SEGMENTS, COUNT, FAST>  `occluded` alone: the early exit.  The any-hit branch of k_locations: HZ_TPB threads, a
//       wave owns a contiguous run of the chunk's rays and hands the next one to a lane whose ray is decided as soon as fewer
//       than HZ_CAST_REGROUP lanes still traverse; the fast stack of hz_trace with the in-kernel retry on the level stack for
//       a ray that runs out of entries.  The traversal is the non-LEAN hz_trace: tfar and tfar_box per lane.
//   k_cast_keys<SEGMENTS>  order = "sorted": one 32-bit key per ray -- the origin's Morton code over the scene's box in the
//       high 24 bits, a direction code in the low 8 -- and the ray's number; radix_sort_pairs_u32 sorts them, and the two
//       kernels above read ray perm[i] and write result perm[i].  The rays are read through `perm` and not gathered first: a
//       ray's 24 bytes are read once either way, and a gather would add a pass and 24 bytes of scratch per ray (DESIGN.md
//       section 5).
//
// Every result depends on its own ray alone, so neither the order nor the chunking nor the choice of kernel can change a
// word: hz_tri_hit_t accepts exactly what hz_tri_hit accepts.
#include "hz_internal.h"
#include "hz_closest_order.h"

namespace hz {

#define HZ_TPB 256
#define HZ_CAST_CLOSEST_TPB 64
#ifndef HZ_CAST_REGROUP
#define HZ_CAST_REGROUP 16        // k_cast_any: refill when fewer lanes than this still traverse (k_shadow_refill's and k_locations' value; not swept)
#endif
#ifndef HZ_CAST_RUN
#define HZ_CAST_RUN 512           // k_cast_any: rays of a wave's run, 8 per lane (not swept)
#endif
#ifndef HZ_CAST_LEAF_BIAS
#define HZ_CAST_LEAF_BIAS 24      // hz_trace: node step when 16 * n_node >= bias * n_leaf (the refill kernels' value)
#endif

std::atomic<int> g_cast_budget{0};                           // hz_debug_set("cast_budget", bytes) (hz_api_sun.hip)
std::atomic<int> g_cast_fast_cap{HZ_CAST_FAST_CAP_DEFAULT};  // hz_debug_set("cast_fast_cap", n)
std::atomic<int> g_cast_sort_only{0};                        // hz_debug_set("cast_sort_only", 1): keys and sort, no tracing (scripts/cast_perf.py)

struct CastParams {
    SceneView sv;
    const float *org;                    // f32[n][3]
    const float *ends;                   // f32[n][3]: unit directions, or (SEGMENTS) targets
    const uint32_t *perm;                // u32[n]: position i of the launch traces ray perm[i]; null: ray i
    unsigned n;                          // rays of the chunk
    float tfar;                          // !SEGMENTS: max_dist
    uint8_t *occ;                        // u8[n] or null
    float *dist;                         // f32[n] or null
    float *point;                        // f32[n][3] (WANT_POINT)
    int stack_cap;                       // k_cast_any<.., FAST>: entries of the fast stack
    int run;                             // k_cast_any: rays per wave
    unsigned long long *counters;        // the Terrain's (HZ_SHADOW_CNT_*)
};

struct CastRay { float ox, oy, oz, dx, dy, dz, tfar; };

// Ray r of the chunk.  All its loads are issued before the first use.  false: a segment whose target is its origin -- no ray.
// Every product, sum, square root and quotient is rounded on its own (-ffp-contract=off), associated as in viewshed_setup.
template <bool SEGMENTS>
__device__ __forceinline__ bool cast_ray(const CastParams &p, size_t r, CastRay &ray) {
    const float *o = p.org + 3 * r, *e = p.ends + 3 * r;
    const float ox = o[0], oy = o[1], oz = o[2];
    const float ex = e[0], ey = e[1], ez = e[2];
    ray.ox = ox; ray.oy = oy; ray.oz = oz;
    if (SEGMENTS) {
        const float dx = ex - ox, dy = ey - oy, dz = ez - oz;
        const float mag = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
        if (!(mag > 0.0f)) return false;
        ray.dx = dx / mag; ray.dy = dy / mag; ray.dz = dz / mag;
        ray.tfar = mag;
    } else {
        ray.dx = ex; ray.dy = ey; ray.dz = ez;
        ray.tfar = p.tfar;
    }
    return true;
}

// box tests start at -tau: the frame of a RayBox is the centred origin shifted back by tau (hz_common.h)
__device__ __forceinline__ RayBox cast_raybox(const SceneView &sv, const CastRay &r) {
    return hz_raybox((r.ox - sv.cx) - sv.tau * r.dx, (r.oy - sv.cy) - sv.tau * r.dy, (r.oz - sv.cz) - sv.tau * r.dz, r.dx, r.dy, r.dz);
}

template <bool WANT_POINT, bool SEGMENTS>
__global__ __launch_bounds__(HZ_CAST_CLOSEST_TPB) void k_cast_closest(CastParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem);
    const int lane = threadIdx.x;
    const unsigned i = blockIdx.x * (unsigned)HZ_CAST_CLOSEST_TPB + (unsigned)lane;
    const bool live = i < p.n;
    bool traced = false;
    if (live) {
        const size_t r = p.perm ? (size_t)p.perm[i] : (size_t)i;
        const float nan = __builtin_nanf("");
        float d = nan, hx = nan, hy = nan, hz_ = nan;
        bool hit = false;
        CastRay ray;
        traced = cast_ray<SEGMENTS>(p, r, ray);
        if (traced) {
            const RayBox rb = cast_raybox(p.sv, ray);
            float t = 0.0f;
            hit = hd_closest_near_first<HZ_CAST_CLOSEST_TPB>(p.sv.nodes, p.sv.prims, stack, lane, ray.ox, ray.oy, ray.oz,
                                                             ray.dx, ray.dy, ray.dz, ray.tfar, p.sv.tau, rb, &t);
            if (hit) {
                d = t == 0.0f ? 0.0f : t;                    // a zero minimum is written as +0.0 (clause 20 step 4)
                if (WANT_POINT) {
                    const float px = ray.dx * d, py = ray.dy * d, pz = ray.dz * d;
                    hx = ray.ox + px; hy = ray.oy + py; hz_ = ray.oz + pz;
                }
            }
        }
        if (p.occ) p.occ[r] = hit ? 1 : 0;
        if (p.dist) p.dist[r] = d;
        if (WANT_POINT) {
            float *q = p.point + 3 * r;
            q[0] = hx; q[1] = hy; q[2] = hz_;
        }
    }
    const unsigned long long m = __ballot(traced);
    if (lane == 0 && m != 0ull) atomicAdd(&p.counters[HZ_SHADOW_CNT_RAYS], (unsigned long long)__popcll(m));
}

// COUNT: also count node visits / triangle tests / wave-level steps and the rays traced twice (Terrain count_work).
// FAST: the fast stack discipline of hz_trace (`stack_cap` entries behind two padding rows); a ray that runs out of entries is
// traced again, to completion, with one entry per tree level in the same LDS column (the launcher makes sure the height fits).
template <bool SEGMENTS, bool COUNT, bool FAST>
__global__ __launch_bounds__(HZ_TPB) void k_cast_any(CastParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem + (FAST ? 2 * HZ_TPB * 4 : 0));
    const int tid = threadIdx.x, lane = tid & 63;
    // the wave's run of the chunk: [next, end)
    const unsigned long long first = ((unsigned long long)blockIdx.x * (HZ_TPB / 64) + (unsigned)(tid >> 6)) * (unsigned long long)p.run;
    const unsigned end = (unsigned)(first + (unsigned long long)p.run < (unsigned long long)p.n ? first + (unsigned long long)p.run : (unsigned long long)p.n);
    unsigned next = first < (unsigned long long)p.n ? (unsigned)first : p.n;       // rays handed out so far (wave uniform)
    unsigned rays = 0, twice = 0;
    TravCounters tc; tc.nodes = 0; tc.tris = 0; tc.w_nodes = 0; tc.w_leaves = 0;
    bool ray_active = false, overflow = false;
    CastRay ray; ray.ox = ray.oy = ray.oz = 0.0f; ray.dx = ray.dy = 0.0f; ray.dz = 1.0f; ray.tfar = 0.0f;
    size_t r = 0;
    RayBox rb = hz_raybox(0, 0, 0, 0, 0, 1);
    TravState ts; hz_trav_reset(ts);
    for (;;) {
        if (next < end) {
            const unsigned long long need = __ballot(!ray_active);
            if (need != 0ull) {
                const unsigned my = next + (unsigned)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                next += (unsigned)__popcll(need);
                if (!ray_active && my < end) {
                    r = p.perm ? (size_t)p.perm[my] : (size_t)my;
                    if (cast_ray<SEGMENTS>(p, r, ray)) {
                        rb = cast_raybox(p.sv, ray);
                        hz_trav_reset(ts);
                        overflow = false;
                        ray_active = true;
                        rays++;
                    } else {
                        p.occ[r] = 0;
                    }
                }
            }
        }
        if (__ballot(ray_active) == 0ull) {
            if (next >= end) break;
            continue;
        }
        if (ray_active) {
            const float tfar_box = ray.tfar + 2.0f * p.sv.tau;
            int res = hz_trace<HZ_TPB, COUNT, 2, false, !FAST>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, ray.ox, ray.oy, ray.oz,
                                                               ray.dx, ray.dy, ray.dz, ray.tfar, tfar_box, rb, ts,
                                                               (next < end) ? HZ_CAST_REGROUP : 0, HZ_CAST_LEAF_BIAS, tc, p.stack_cap, overflow);
            if (FAST && res != 2 && overflow) {
                bool unused = false;
                hz_trav_reset(ts);
                res = hz_trace<HZ_TPB, COUNT, 2, false, true>(p.sv.nodes, p.sv.prims, nullptr, 0, stack, tid, ray.ox, ray.oy, ray.oz,
                                                              ray.dx, ray.dy, ray.dz, ray.tfar, tfar_box, rb, ts, 0, HZ_CAST_LEAF_BIAS, tc, 0, unused);
                if (COUNT) twice++;
            }
            if (res != 2) {
                p.occ[r] = res == 1 ? 1 : 0;
                ray_active = false;
            }
        }
    }
    unsigned long long rr = rays;
    for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off);
    if (lane == 0 && rr) atomicAdd(&p.counters[HZ_SHADOW_CNT_RAYS], rr);
    if (COUNT) {
        unsigned long long nc = tc.nodes, tn = tc.tris, wn = tc.w_nodes, wl = tc.w_leaves, tw = twice;
        for (int off = 32; off > 0; off >>= 1) {
            nc += __shfl_xor(nc, off); tn += __shfl_xor(tn, off); wn += __shfl_xor(wn, off); wl += __shfl_xor(wl, off);
            tw += __shfl_xor(tw, off);
        }
        if (lane == 0) {
            atomicAdd(&p.counters[HZ_SHADOW_CNT_NODES], nc); atomicAdd(&p.counters[HZ_SHADOW_CNT_TRIS], tn);
            atomicAdd(&p.counters[HZ_SHADOW_CNT_WAVE_NODE], wn); atomicAdd(&p.counters[HZ_SHADOW_CNT_WAVE_LEAF], wl);
            if (tw) atomicAdd(&p.counters[HZ_SHADOW_CNT_TWICE], tw);
        }
    }
}

// v in [0, 1] -> its 8 bits spread to every third bit
__device__ __forceinline__ uint32_t cast_spread8(float v) {
    uint32_t q = (uint32_t)__builtin_fminf(__builtin_fmaxf(v * 256.0f, 0.0f), 255.0f);
    q = (q | (q << 8)) & 0x00f00fu;
    q = (q | (q << 4)) & 0x0c30c3u;
    q = (q | (q << 2)) & 0x249249u;
    return q;
}

// The sort key of every ray of the chunk and its number.  Free of any contract: only the permutation matters.
template <bool SEGMENTS>
__global__ __launch_bounds__(256) void k_cast_keys(const float *__restrict__ org, const float *__restrict__ ends, unsigned n,
                                                   float lo_x, float lo_y, float lo_z, float inv_x, float inv_y, float inv_z,
                                                   uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *o = org + 3 * (size_t)i, *e = ends + 3 * (size_t)i;
    const float ox = o[0], oy = o[1], oz = o[2];
    float dx = e[0], dy = e[1], dz = e[2];
    if (SEGMENTS) {
        dx -= ox; dy -= oy; dz -= oz;
        const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz));
        const float s = m > 0.0f ? 1.0f / m : 0.0f;
        dx *= s; dy *= s; dz *= s;                                    // the largest component is +-1: enough for the code below
    }
    // a point outside the scene's box is clamped onto it (NaN cannot come: the inputs are finite)
    const uint32_t morton = cast_spread8((ox - lo_x) * inv_x) | (cast_spread8((oy - lo_y) * inv_y) << 1) | (cast_spread8((oz - lo_z) * inv_z) << 2);
    // the octant, then two bits of |dx| and |dy| and one of |dz|
    const uint32_t oct = (dx < 0.0f ? 4u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 1u : 0u);
    const uint32_t qx = (uint32_t)__builtin_fminf(__builtin_fabsf(dx) * 4.0f, 3.0f);
    const uint32_t qy = (uint32_t)__builtin_fminf(__builtin_fabsf(dy) * 4.0f, 3.0f);
    const uint32_t qz = (uint32_t)__builtin_fminf(__builtin_fabsf(dz) * 2.0f, 1.0f);
    keys[i] = (morton << 8) | (oct << 5) | (qx << 3) | (qy << 1) | qz;
    vals[i] = i;
}

int cast_keys_launch(const Scene *sc, const float *org, const float *ends, int segments, unsigned n, uint32_t *keys, uint32_t *vals,
                     hipStream_t st) {
    if (n == 0) return HZ_OK;
    float inv[3];
    for (int k = 0; k < 3; k++) {
        const float ext = sc->hdr.hi[k] - sc->hdr.lo[k];
        inv[k] = ext > 0.0f ? 1.0f / ext : 0.0f;
    }
    const dim3 grid((n + 255u) / 256u);
    if (segments)
        hipLaunchKernelGGL(k_cast_keys<true>, grid, dim3(256), 0, st, org, ends, n, sc->hdr.lo[0], sc->hdr.lo[1], sc->hdr.lo[2],
                           inv[0], inv[1], inv[2], keys, vals);
    else
        hipLaunchKernelGGL(k_cast_keys<false>, grid, dim3(256), 0, st, org, ends, n, sc->hdr.lo[0], sc->hdr.lo[1], sc->hdr.lo[2],
                           inv[0], inv[1], inv[2], keys, vals);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

static int cast_launch_kernel(void (*k)(CastParams), const CastParams &p, unsigned grid, unsigned tpb, size_t lds, hipStream_t st) {
    HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(grid), dim3(tpb), lds, st, p);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int cast_launch(const Scene *sc, const CastArgs &a, hipStream_t st) {
    if (a.num_rays == 0) return HZ_OK;
    if (!a.occluded && !a.dist && !a.point) return HZ_OK;
    CastParams p;
    p.sv = scene_view(sc);
    p.org = a.origins; p.ends = a.ends; p.perm = a.perm;
    p.n = a.num_rays; p.tfar = a.max_dist;
    p.occ = a.occluded; p.dist = a.dist; p.point = a.point;
    p.stack_cap = 0; p.run = 0;
    p.counters = a.counters;
    const int height = std::max(sc->hdr.height, 1);
    if (a.dist || a.point) {
        static void (*const kernels[2][2])(CastParams) = {{k_cast_closest<false, false>, k_cast_closest<false, true>},
                                                          {k_cast_closest<true, false>, k_cast_closest<true, true>}};
        // individual child links: up to 3 per tree level
        const size_t lds = (size_t)(3 * height) * HZ_CAST_CLOSEST_TPB * 4;
        const unsigned grid = (a.num_rays + (unsigned)HZ_CAST_CLOSEST_TPB - 1u) / (unsigned)HZ_CAST_CLOSEST_TPB;
        return cast_launch_kernel(kernels[a.point ? 1 : 0][a.segments ? 1 : 0], p, grid, HZ_CAST_CLOSEST_TPB, lds, st);
    }
    static void (*const kernels[2][2][2])(CastParams) = {
        {{k_cast_any<false, false, false>, k_cast_any<false, false, true>}, {k_cast_any<false, true, false>, k_cast_any<false, true, true>}},
        {{k_cast_any<true, false, false>, k_cast_any<true, false, true>}, {k_cast_any<true, true, false>, k_cast_any<true, true, true>}}};
    // the fast stack (+ 2 padding rows) if the level stack of the in-kernel retry fits into it, else the level stack alone
    const int fast_cap = std::min(g_cast_fast_cap.load(std::memory_order_relaxed), 3 * height + 1);
    const bool fast = fast_cap >= 5 && fast_cap >= height;
    p.stack_cap = fast ? fast_cap : 0;
    const size_t lds = (size_t)(fast ? fast_cap + 2 : height) * HZ_TPB * 4;
    // a wave's run: HZ_CAST_RUN rays, fewer while that leaves the chunk less than ~8 waves per CU (256 CUs) -- but a full wave
    int run = HZ_CAST_RUN;
    while (run > 64 && (unsigned long long)a.num_rays / (unsigned)run < 2048ull) run >>= 1;
    p.run = run;
    const unsigned per_wg = (unsigned)run * (HZ_TPB / 64);
    const unsigned grid = (a.num_rays + per_wg - 1u) / per_wg;
    return cast_launch_kernel(kernels[a.segments ? 1 : 0][a.count_work ? 1 : 0][fast ? 1 : 0], p, grid, HZ_TPB, lds, st);
}

}  // namespace hz
