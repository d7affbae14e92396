// hz_shadow.h -- what the four refill kernels (k_shadow_refill, k_accum_refill: hz_shadow.hip; k_viewshed_refill:
// hz_viewshed.hip; k_sight_refill: hz_sight.hip) share beside their loop (hz_refill_loop.inc): the kernel parameters, the
// tuning constants of the loop, the launch configuration, the launch itself and two small device functions.
#pragma once
#include "hz_internal.h"

namespace hz {

#ifndef HZ_SHADOW_LEAF_BIAS
#define HZ_SHADOW_LEAF_BIAS 24   // node step when 16 * n_node >= bias * n_leaf (hz_trace); 20 until round 4 (profiles/r04/shadow_leaf_bias.log)
#endif

struct ShadowParams {
    SceneView sv;
    const float *vec_tilt, *vec_norm, *surf_enl_fac, *elevation;
    const uint8_t *mask;
    int offset_0, offset_1, dim_in_0, dim_in_1;
    TileMap tm;
    const float *suns;       // device f32[num_sun][3]; blockIdx.y selects the position
    size_t out_stride;       // cells per sun position (outputs of position s start at s * out_stride)
    float fill, dot_prod_min;
    int refrac, which;
    const double *refrac_fac;   // refrac: per cell ((double)pressure / 101.0) * (283.0 / (273.0 + (double)temperature_degC)), k_refrac_factor
    uint8_t *out_u8; float *out_f32;
    int top_nodes, stack_bytes;
    int stack_cap;                 // FAST: entries of the fast stack (hz_trace, !LEVELSTACK), sentinel included
    int nb;                  // k_shadow_refill: 8 x 8 blocks per wave
    unsigned long long *counters;
};

// shadow_comp.cpp:96-106
__device__ __forceinline__ void vec_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// the wave's ray count (and, COUNT, its traversal counters) added to the call's counters
template <bool COUNT>
__device__ __forceinline__ void shadow_counters(const ShadowParams &p, unsigned rays, const TravCounters &tc, int lane) {
    unsigned long long r = rays;
    for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off);
    if (lane == 0 && r) atomicAdd(&p.counters[HZ_SHADOW_CNT_RAYS], r);
    if (COUNT) {
        unsigned long long nc = tc.nodes, tn = tc.tris, wn = tc.w_nodes, wl = tc.w_leaves;
        for (int off = 32; off > 0; off >>= 1) {
            nc += __shfl_xor(nc, off); tn += __shfl_xor(tn, off); wn += __shfl_xor(wn, off); wl += __shfl_xor(wl, off);
        }
        if (lane == 0) {
            atomicAdd(&p.counters[HZ_SHADOW_CNT_NODES], nc); atomicAdd(&p.counters[HZ_SHADOW_CNT_TRIS], tn);
            atomicAdd(&p.counters[HZ_SHADOW_CNT_WAVE_NODE], wn); atomicAdd(&p.counters[HZ_SHADOW_CNT_WAVE_LEAF], wl);
        }
    }
}

#ifndef HZ_SHADOW_REGROUP
#define HZ_SHADOW_REGROUP 16      // refill when fewer lanes than this are still traversing (40 until round 5; re-swept 40 ... 8 after the loop rewrite:
                                  // 16 - 20 is the flat optimum, -0.5 % without and -7.7 % with refraction, profiles/r05/ab_shadow_and_locations_thresholds.log)
#endif
// resident workgroups per CU the register allocation is held to (profiles/r04/ab_shadow_fast_stack.log, ms per sun position:
// unconstrained = 86 VGPRs = 5 workgroups 0.955; 6 (80 VGPRs, no spills) 0.884; 7 (72 VGPRs, 6 spilled) 0.857; 8 (64 VGPRs, 21
// spilled) 0.957).  The counting instantiation carries ~10 more live values and is left at 5.
#ifndef HZ_SHADOW_WG
#define HZ_SHADOW_WG 7
#endif

// Launch configuration of the refill kernels for one launch of a.num_sun positions: parameters, dynamic LDS, grid, and
// whether the fast stack is used.  Returns 0 when there is nothing to launch.
int shadow_config(const Scene *sc, const ShadowArgs &a, ShadowParams &p, size_t &lds, dim3 &grid, bool &fast);

// The four instantiations of a refill kernel `template <bool COUNT, bool FAST> __global__ void K(Params)` as [count][fast],
// and the launch of the one a call asks for, with the configuration of shadow_config.
#define HZ_REFILL_KERNELS(K) {{K<false, false>, K<false, true>}, {K<true, false>, K<true, true>}}
template <class Params>
int refill_launch(void (*const (&kernels)[2][2])(Params), const Params &params, int count_work, bool fast, dim3 grid, size_t lds,
                  hipStream_t st) {
    void (*const k)(Params) = kernels[count_work ? 1 : 0][fast ? 1 : 0];
    HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(256), lds, st, params);        // (256: the kernels' HZ_TPB)
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
