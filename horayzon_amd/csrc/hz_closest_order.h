// hz_closest_order.h -- the closest-hit traversal with the children of a node visited front to back (gfx950; DESIGN.md
// section 4, clause 16).  Shared by hz_horidist.hip (the distance to the horizon) and hz_panorama.hip (depth images from
// observer points): both run it with one wave per workgroup and a stack of individual child links, up to 3 per tree level.
#pragma once
#include "hz_common.h"

namespace hz {

// hz_node_hits (hz_common.h) -- the same conservative test, instruction for instruction -- which also says in which order a ray
// meets the four quadrants: `flip` bit 0 = the column half 1 is entered before half 0, bit 1 = the row half 1 before half 0
// (the unclamped entry parameters of the two x ranges and of the two y ranges).  Slots flip, flip ^ 1, flip ^ 2, flip ^ 3
// are then front to back (the two in the middle in either order).
__device__ __forceinline__ void hd_node_hits_order(const NodeRay &n, const RayBox &r, float tfar, const uint4 &q,
                                                   bool &h0, bool &h1, bool &h2, bool &h3, int &flip) {
    const uint32_t px0 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.x, r.sel_x), px1 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.x, r.sel_x + HZ_SEL_PAIR1);
    const uint32_t py0 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.y, r.sel_y), py1 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.y, r.sel_y + HZ_SEL_PAIR1);
    const uint32_t pz0 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.z, r.sel_z), pz1 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.z, r.sel_z + HZ_SEL_PAIR1);
    const uint32_t pz2 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.w, r.sel_z), pz3 = __builtin_amdgcn_perm(HZ_HALF_MAGIC, q.w, r.sel_z + HZ_SEL_PAIR1);
    const float nx0 = hz_fma_mix_lo(px0, n.ax, n.bx), fx0 = hz_fma_mix_hi(px0, n.ax, n.bx);
    const float nx1 = hz_fma_mix_lo(px1, n.ax, n.bx), fx1 = hz_fma_mix_hi(px1, n.ax, n.bx);
    const float ny0 = hz_fma_mix_lo(py0, n.ay, n.by), fy0 = hz_fma_mix_hi(py0, n.ay, n.by);
    const float ny1 = hz_fma_mix_lo(py1, n.ay, n.by), fy1 = hz_fma_mix_hi(py1, n.ay, n.by);
    flip = (nx1 < nx0 ? 1 : 0) | (ny1 < ny0 ? 2 : 0);
    const float cx0 = __builtin_fmaxf(nx0, 0.0f), cx1 = __builtin_fmaxf(nx1, 0.0f);
    const float gx0 = __builtin_fminf(fx0, tfar), gx1 = __builtin_fminf(fx1, tfar);
#define HD_CHILD(pz, nx, fx, ny, fy, out) do { \
        const float nz_ = hz_fma_mix_lo(pz, n.az, n.bz), fz_ = hz_fma_mix_hi(pz, n.az, n.bz); \
        const float tmin_ = __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz_); \
        const float tmax_ = __builtin_fminf(__builtin_fminf(fx, fy), fz_); \
        out = tmin_ <= tmax_ * 1.000001f; } while (0)
    HD_CHILD(pz0, cx0, gx0, ny0, fy0, h0);
    HD_CHILD(pz1, cx1, gx1, ny0, fy0, h1);
    HD_CHILD(pz2, cx0, gx0, ny1, fy1, h2);
    HD_CHILD(pz3, cx1, gx1, ny1, fy1, h3);
#undef HD_CHILD
}

// hz_closest (hz_common.h) with the children of a node visited front to back: the same boxes against the same bound, the
// same triangle tests, the minimum over all accepted triangles -- only the order differs, so a near hit shrinks the bound
// before the far subtrees are looked at.  The result cannot depend on it (clause 16).
template <int TPB>
__device__ __forceinline__ bool hd_closest_near_first(const Node *__restrict__ nodes, const Prim *__restrict__ prims,
                                                      int *stack, int tid, float ox, float oy, float oz, float dx,
                                                      float dy, float dz, float tfar, float tau, const RayBox &rb, float *dist) {
    int node = 0, sp = 0;
    float best = __builtin_inff();
    bool any = false;
    while (node != HZ_EMPTY) {
        if (node >= 0) {
            float4 n0; uint4 n1;
            hz_load_node(nodes + node, n0, n1);
            const float tf = (any ? __builtin_fminf(tfar, best * 1.0001f) : tfar) + 2.0f * tau;
            const NodeRay nr = hz_node_ray(rb, n0.x, n0.y, n0.z);
            bool h0, h1, h2, h3;
            int flip;
            hd_node_hits_order(nr, rb, tf, n1, h0, h1, h2, h3, flip);
            const int first = __float_as_int(n0.w);
            const int m = (h0 ? 1 : 0) | (h1 ? 2 : 0) | (h2 ? 4 : 0) | (h3 ? 8 : 0);
            const int s0 = flip, s1 = flip ^ 1, s2 = flip ^ 2, s3 = flip ^ 3;
            int next = HZ_EMPTY;
            if ((m >> s3) & 1) next = first + s3;
            if ((m >> s2) & 1) { if (next != HZ_EMPTY) { stack[sp * TPB + tid] = next; sp++; } next = first + s2; }
            if ((m >> s1) & 1) { if (next != HZ_EMPTY) { stack[sp * TPB + tid] = next; sp++; } next = first + s1; }
            if ((m >> s0) & 1) { if (next != HZ_EMPTY) { stack[sp * TPB + tid] = next; sp++; } next = first + s0; }
            if (next != HZ_EMPTY) { node = next; continue; }
        } else {
            float4 q0, q1, q2;
            hz_load_prim(prims + HZ_LEAF_ID(node), q0, q1, q2);
            float t;
            if (hz_tri_hit_t(ox, oy, oz, dx, dy, dz, tfar, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, &t)) {
                any = true; best = __builtin_fminf(best, t);
            }
            if ((q2.y == q2.y) &&
                hz_tri_hit_t(ox, oy, oz, dx, dy, dz, tfar, q0.w, q1.x, q1.y, q2.y, q2.z, q2.w, q1.z, q1.w, q2.x, &t)) {
                any = true; best = __builtin_fminf(best, t);
            }
        }
        if (sp > 0) { sp--; node = stack[sp * TPB + tid]; } else node = HZ_EMPTY;
    }
    if (any) *dist = best;
    return any;
}

}  // namespace hz
