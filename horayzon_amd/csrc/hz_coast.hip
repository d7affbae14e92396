// hz_coast.hip -- nearest coastline vertex of every water cell, in float64 (reference: horayzon/ocean_masking.py:163-345,
// which asks a SciPy k-d tree).  Contract: for a water cell c and a vertex p
//     d2(c, p) = ((cx - px) * (cx - px) + (cy - py) * (cy - py)) + (cz - pz) * (cz - pz)
// every operation rounded once (-ffp-contract=off), the answer the minimum of d2 over all vertices.  A minimum of identically
// computed values does not depend on the order of visits, so the index below only decides which vertices are skipped:
// a box is skipped when its distance bound, monotone in every rounding, exceeds the best value so far.
//
// Index: the vertices sorted by a 30-bit Morton key of their position in their own bounding box, leaves of HZ_COAST_LEAF
// consecutive sorted vertices, and a COMPLETE binary tree of boxes over the leaves in heap order (node n has the children 2n and
// 2n + 1, leaf j is node n_leaf_pad + j, n_leaf_pad the power of two >= the number of leaves; the leaves past the last one are
// empty boxes, lo = +inf and hi = -inf, whose bound is +inf).  The order of the leaves is all the key is used for: empty key
// cells cost nothing, equal keys (one vertex, identical vertices, vertices on a line) only make neighbouring leaves overlap.
// The heap order needs no child or parent pointers, so the traversal keeps no stack: one word of "far child still to visit"
// bits, one per level, is the whole state besides the node number.
#include "hz_internal.h"

namespace hz {

#define COAST_TPB 256
#define COAST_BBOX_BLOCKS 512

struct CoastBox { double lo[3], hi[3]; };   // 48 bytes, 16-byte aligned in the node array

// ---------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }

// Bounding box of n elements: vertices f64[n][3] (in_is_box = 0) or boxes f64[n][6]; one box per workgroup to out[blockIdx.x]
__global__ __launch_bounds__(COAST_TPB) void k_coast_bbox(const double *__restrict__ in, uint32_t n, int in_is_box,
                                                        double *__restrict__ out) {
    __shared__ double s[6][COAST_TPB];
    const double inf = __builtin_inf();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (size_t i = (size_t)blockIdx.x * COAST_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * COAST_TPB) {
        const double *e = in + i * (in_is_box ? 6 : 3);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = dmin(lo[k], e[k]);
            hi[k] = dmax(hi[k], e[k + (in_is_box ? 3 : 0)]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { s[k][threadIdx.x] = lo[k]; s[k + 3][threadIdx.x] = hi[k]; }
    __syncthreads();
    for (int w = COAST_TPB / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s[k][threadIdx.x] = dmin(s[k][threadIdx.x], s[k][threadIdx.x + w]);
                s[k + 3][threadIdx.x] = dmax(s[k + 3][threadIdx.x], s[k + 3][threadIdx.x + w]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[(size_t)blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {     // 10 bits -> every third bit
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// Key of a coordinate inside [lo, hi]: 0 .. 1023.  A NaN, an empty extent or a value outside the box ends at a bound of the
// range: the key only orders the leaves, every value of it gives a correct tree.
__device__ __forceinline__ uint32_t quant10(double v, double lo, double hi) {
    const double t = (v - lo) / (hi - lo) * 1024.0;
    if (t >= 1023.0) return 1023u;
    if (t > 0.0) return (uint32_t)t;
    return 0u;
}

__global__ __launch_bounds__(COAST_TPB) void k_coast_keys(const double *__restrict__ pts, uint32_t n,
                                                        const double *__restrict__ bbox, uint32_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * COAST_TPB + threadIdx.x;
    if (i >= n) return;
    const double *p = pts + i * 3;
    keys[i] = spread10(quant10(p[0], bbox[0], bbox[3])) | (spread10(quant10(p[1], bbox[1], bbox[4])) << 1)
            | (spread10(quant10(p[2], bbox[2], bbox[5])) << 2);
    vals[i] = (uint32_t)i;
}

// The vertices in sorted order; the last leaf is filled up with copies of the last vertex (a copy changes no minimum and no box),
// so that every leaf holds exactly HZ_COAST_LEAF vertices
__global__ __launch_bounds__(COAST_TPB) void k_coast_gather(const double *__restrict__ pts, const uint32_t *__restrict__ order,
                                                          uint32_t n, uint32_t n_padded, double *__restrict__ sorted) {
    const size_t i = (size_t)blockIdx.x * COAST_TPB + threadIdx.x;
    if (i >= n_padded) return;
    const double *p = pts + (size_t)order[i < n ? i : n - 1] * 3;
    sorted[i * 3] = p[0]; sorted[i * 3 + 1] = p[1]; sorted[i * 3 + 2] = p[2];
}

// nodes[n_leaf_pad + j]: the exact minima / maxima of leaf j's vertices; empty past the last leaf
__global__ __launch_bounds__(COAST_TPB) void k_coast_leaves(const double *__restrict__ sorted, uint32_t n_leaf,
                                                          uint32_t n_leaf_pad, CoastBox *__restrict__ nodes) {
    const size_t j = (size_t)blockIdx.x * COAST_TPB + threadIdx.x;
    if (j >= n_leaf_pad) return;
    const double inf = __builtin_inf();
    CoastBox b = {{inf, inf, inf}, {-inf, -inf, -inf}};
    if (j < n_leaf) {
        const double *p = sorted + j * (HZ_COAST_LEAF * 3);
#pragma unroll
        for (int q = 0; q < HZ_COAST_LEAF; q++)
#pragma unroll
            for (int k = 0; k < 3; k++) { b.lo[k] = dmin(b.lo[k], p[q * 3 + k]); b.hi[k] = dmax(b.hi[k], p[q * 3 + k]); }
    }
    nodes[n_leaf_pad + j] = b;
}

// one level: nodes[first + i] = union of its two children, i < count
__global__ __launch_bounds__(COAST_TPB) void k_coast_merge(CoastBox *nodes, uint32_t first, uint32_t count) {
    const size_t i = (size_t)blockIdx.x * COAST_TPB + threadIdx.x;
    if (i >= count) return;
    const size_t n = (size_t)first + i;
    const CoastBox a = nodes[2 * n], b = nodes[2 * n + 1];
    CoastBox u;
#pragma unroll
    for (int k = 0; k < 3; k++) { u.lo[k] = dmin(a.lo[k], b.lo[k]); u.hi[k] = dmax(a.hi[k], b.hi[k]); }
    nodes[n] = u;
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t coast_scratch_bytes(size_t num_pts, CoastIndex *ix) {
    const size_t n_leaf = (num_pts + HZ_COAST_LEAF - 1) / HZ_COAST_LEAF;
    size_t pad = 1;
    while (pad < n_leaf) pad <<= 1;
    ix->n_pts = (uint32_t)num_pts; ix->n_leaf = (uint32_t)n_leaf; ix->n_leaf_pad = (uint32_t)pad;
    size_t off = 0;
    ix->off_counters = off; off += align256(HZ_COAST_CNT_N * sizeof(unsigned long long));
    if (num_pts == 0) return off;
    ix->off_sorted = off;   off += align256(n_leaf * HZ_COAST_LEAF * 3 * sizeof(double));
    ix->off_nodes = off;    off += align256(2 * pad * sizeof(CoastBox));
    ix->off_bbox = off;     off += align256((COAST_BBOX_BLOCKS + 1) * 6 * sizeof(double));
    ix->off_sort = off;     off += align256((4 * num_pts + sort_temp_elems(num_pts)) * sizeof(uint32_t));
    return off;
}

// pts: device f64[num_pts][3]; scratch: device, coast_scratch_bytes(num_pts, ix) bytes (that call filled *ix in)
int coast_index_build(const double *pts, void *scratch, CoastIndex *ix, hipStream_t st) {
    char *base = (char *)scratch;
    ix->counters = (unsigned long long *)(base + ix->off_counters);
    HZ_HIP(hipMemsetAsync(ix->counters, 0, HZ_COAST_CNT_N * sizeof(unsigned long long), st));
    ix->sorted = nullptr; ix->nodes = nullptr;
    const uint32_t n = ix->n_pts;
    if (n == 0) return HZ_OK;
    double *sorted = (double *)(base + ix->off_sorted);
    CoastBox *nodes = (CoastBox *)(base + ix->off_nodes);
    double *bbox_part = (double *)(base + ix->off_bbox), *bbox = bbox_part + (size_t)COAST_BBOX_BLOCKS * 6;
    uint32_t *keys_a = (uint32_t *)(base + ix->off_sort), *vals_a = keys_a + n, *keys_b = vals_a + n, *vals_b = keys_b + n,
             *sort_tmp = vals_b + n;
    const unsigned blocks_n = (unsigned)(((size_t)n + COAST_TPB - 1) / COAST_TPB);
    const unsigned bbox_blocks = std::min<unsigned>(blocks_n, COAST_BBOX_BLOCKS);
    hipLaunchKernelGGL(k_coast_bbox, dim3(bbox_blocks), dim3(COAST_TPB), 0, st, pts, n, 0, bbox_part);
    hipLaunchKernelGGL(k_coast_bbox, dim3(1), dim3(COAST_TPB), 0, st, (const double *)bbox_part, (uint32_t)bbox_blocks, 1, bbox);
    hipLaunchKernelGGL(k_coast_keys, dim3(blocks_n), dim3(COAST_TPB), 0, st, pts, n, (const double *)bbox, keys_a, vals_a);
    HZ_HIP(hipGetLastError());
    int rc = radix_sort_pairs_u32(keys_a, vals_a, keys_b, vals_b, n, sort_tmp, st, 4);   // 4 passes: sorted pairs in keys_a / vals_a
    if (rc) return rc;
    const size_t n_padded = (size_t)ix->n_leaf * HZ_COAST_LEAF;
    hipLaunchKernelGGL(k_coast_gather, dim3((unsigned)((n_padded + COAST_TPB - 1) / COAST_TPB)), dim3(COAST_TPB), 0, st, pts,
                       (const uint32_t *)vals_a, n, (uint32_t)n_padded, sorted);
    hipLaunchKernelGGL(k_coast_leaves, dim3((ix->n_leaf_pad + COAST_TPB - 1) / COAST_TPB), dim3(COAST_TPB), 0, st,
                       (const double *)sorted, ix->n_leaf, ix->n_leaf_pad, nodes);
    for (uint32_t first = ix->n_leaf_pad >> 1; first >= 1; first >>= 1)     // level by level up to the root, node 1
        hipLaunchKernelGGL(k_coast_merge, dim3((first + COAST_TPB - 1) / COAST_TPB), dim3(COAST_TPB), 0, st, nodes, first, first);
    HZ_HIP(hipGetLastError());
    ix->sorted = sorted; ix->nodes = nodes;
    return HZ_OK;
}

// ---------------------------------------------------------------------------------------
// query
// ---------------------------------------------------------------------------------------
struct CoastQuery {
    const double *x, *y, *z;        // f64[len_0][len_1]
    const uint8_t *mask_land;
    int len_0, len_1, tiles_j;
    unsigned long long n_tiles;
    const double *sorted;           // f64[n_leaf * HZ_COAST_LEAF][3]
    const CoastBox *nodes;          // [2 * n_leaf_pad], node 0 unused
    uint32_t n_pts, n_leaf, n_leaf_pad, max_iter;
    double thr, thr2;               // any-hit form: the threshold and the largest d2 whose square root is <= thr
    double *dist;                   // nearest form
    uint8_t *mask_buffer;           // any-hit form
    unsigned long long *counters;   // [0] water cells, [1] lanes that hit the iteration bound
};

__device__ __forceinline__ double coast_d2(double cx, double cy, double cz, const double *__restrict__ p) {
    const double dx = cx - p[0], dy = cy - p[1], dz = cz - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// max(lo - c, 0, c - hi) per axis, squared and summed in the order of d2: <= d2(c, p) as computed for every p inside the box,
// because each of the operations is monotone under round-to-nearest.  An empty box (lo = +inf, hi = -inf) gives +inf.
__device__ __forceinline__ double coast_box_d2(double cx, double cy, double cz, const CoastBox *__restrict__ b) {
    const double2 *q = reinterpret_cast<const double2 *>(b);
    const double2 q0 = q[0], q1 = q[1], q2 = q[2];                   // lo.x lo.y | lo.z hi.x | hi.y hi.z
    const double bx = dmax(dmax(q0.x - cx, 0.0), cx - q1.y);
    const double by = dmax(dmax(q0.y - cy, 0.0), cy - q2.x);
    const double bz = dmax(dmax(q1.x - cz, 0.0), cz - q2.y);
    return (bx * bx + by * by) + bz * bz;
}

// One lane per cell, one wave per 8 x 8 block of cells, so that the lanes of a wave walk the same part of the tree.
// ANY = false: dist[c] = sqrt(min d2).  ANY = true: mask_buffer[c] = (min d2 > thr2), decided at the first vertex within thr2.
template <bool ANY>
__global__ __launch_bounds__(COAST_TPB) void k_coast_query(const CoastQuery a) {
    const int lane = threadIdx.x & 63;
    const unsigned long long tile = (unsigned long long)blockIdx.x * (COAST_TPB / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;                                   // the whole wave
    const int i = (int)(tile / (unsigned)a.tiles_j) * 8 + (lane >> 3), j = (int)(tile % (unsigned)a.tiles_j) * 8 + (lane & 7);
    const bool inside = i < a.len_0 && j < a.len_1;
    const size_t cell = inside ? (size_t)i * a.len_1 + j : 0;
    const bool water = inside && a.mask_land[cell] == 0;
    if (inside && !water) {                                          // land cells do no work
        if (ANY) a.mask_buffer[cell] = 0; else a.dist[cell] = __builtin_nan("");
    }
    const unsigned long long wet = __ballot(water);
    if (wet == 0ull) return;
    if (lane == 0) atomicAdd(&a.counters[0], (unsigned long long)__popcll(wet));
    if (a.n_pts == 0) {                                              // an empty set is infinitely far away
        if (water) { if (ANY) a.mask_buffer[cell] = __builtin_inf() > a.thr ? 1 : 0; else a.dist[cell] = __builtin_inf(); }
        return;
    }
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (water) { cx = a.x[cell]; cy = a.y[cell]; cz = a.z[cell]; }

    // First upper bound, shared by the wave: a vertex near the block's first water cell, found by sampling 64 vertices of a
    // range of the sorted order, one per lane (land lanes help), and narrowing the range round the nearest sample.  The range
    // shrinks 32-fold per round, so 7 rounds cover 2^31 vertices.  Every index stays inside [0, n_pts) whatever the distances are.
    const int first_wet = __ffsll((long long)wet) - 1;
    const double sx = __shfl(cx, first_wet), sy = __shfl(cy, first_wet), sz = __shfl(cz, first_wet);
    uint32_t lo = 0, len = a.n_pts, seed = 0;
    for (int round = 0; round < 8; round++) {
        uint32_t idx = lo + (uint32_t)(((unsigned long long)lane * len) >> 6);
        double d = coast_d2(sx, sy, sz, a.sorted + (size_t)idx * 3);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(d, off);
            const uint32_t oi = __shfl_xor(idx, off);
            if (od < d || (od == d && oi < idx)) { d = od; idx = oi; }
        }
        seed = idx;
        if (len <= 64u) break;
        const uint32_t step = (len + 63u) >> 6, end = lo + len;
        lo = seed - lo > step ? seed - step : lo;
        len = (end - seed > step + 1u ? seed + step + 1u : end) - lo;
    }
    if (!water) return;

    double best = coast_d2(cx, cy, cz, a.sorted + (size_t)seed * 3);
    bool found = false;
    if (ANY) { found = best <= a.thr2; best = a.thr2; }

    // Stackless walk of the heap-ordered tree, nearest child first.  `visit`: node n passed its box test and is entered;
    // otherwise the walk climbs.  Bit d of `trail` = the far child of the path's node at depth d waits.  Every node is entered at
    // most once and left upwards at most twice, so 6 * n_leaf_pad steps cannot be exceeded by a correct walk.
    const uint32_t n_leaf_pad = a.n_leaf_pad;
    uint32_t n = 1, trail = 0, iter = 0;
    int depth = 0;
    bool visit = !found && coast_box_d2(cx, cy, cz, a.nodes + 1) <= best;
    bool over = false;
    while (!found && (visit || n != 1u)) {
        if (++iter > a.max_iter) { over = true; break; }
        if (visit) {
            if (n >= n_leaf_pad + a.n_leaf) {                        // an empty leaf (entered only while best is +inf)
                visit = false;
            } else if (n >= n_leaf_pad) {
                const double *p = a.sorted + (size_t)(n - n_leaf_pad) * (HZ_COAST_LEAF * 3);
                double m = coast_d2(cx, cy, cz, p);
#pragma unroll
                for (int q = 1; q < HZ_COAST_LEAF; q++) m = dmin(m, coast_d2(cx, cy, cz, p + q * 3));
                if (ANY) found = m <= best; else best = dmin(best, m);
                visit = false;
            } else {
                const double d0 = coast_box_d2(cx, cy, cz, a.nodes + 2 * (size_t)n);
                const double d1 = coast_box_d2(cx, cy, cz, a.nodes + 2 * (size_t)n + 1);
                const bool second = d1 < d0;
                const double d_near = second ? d1 : d0, d_far = second ? d0 : d1;
                if (d_near <= best) {
                    if (d_far <= best) trail |= 1u << depth;
                    n = 2 * n + (second ? 1u : 0u);
                    depth++;
                } else {
                    visit = false;
                }
            }
        } else {
            const uint32_t bit = 1u << (depth - 1);
            if (trail & bit) {                                       // the sibling waits: test it against today's best
                trail ^= bit;
                n ^= 1u;
                visit = coast_box_d2(cx, cy, cz, a.nodes + n) <= best;
            } else {
                n >>= 1;
                depth--;
            }
        }
    }
    if (over) atomicAdd(&a.counters[1], 1ull);
    if (ANY) a.mask_buffer[cell] = found ? 0 : 1;
    else a.dist[cell] = __builtin_sqrt(best);                        // correctly rounded on the device
}

int coast_query_launch(const CoastIndex &ix, const double *x, const double *y, const double *z, const uint8_t *mask_land,
                       int len_0, int len_1, int any_hit, double thr, double thr2, double *dist, uint8_t *mask_buffer,
                       hipStream_t st) {
    CoastQuery a;
    a.x = x; a.y = y; a.z = z; a.mask_land = mask_land;
    a.len_0 = len_0; a.len_1 = len_1;
    a.tiles_j = (len_1 + 7) / 8;
    a.n_tiles = (unsigned long long)((len_0 + 7) / 8) * (unsigned long long)a.tiles_j;
    a.sorted = ix.sorted; a.nodes = (const CoastBox *)ix.nodes;
    a.n_pts = ix.n_pts; a.n_leaf = ix.n_leaf; a.n_leaf_pad = ix.n_leaf_pad;
    a.max_iter = 6u * ix.n_leaf_pad + 16u;                           // n_leaf_pad <= 2^28 (hz_api.hip refuses more vertices)
    a.thr = thr; a.thr2 = thr2;
    a.dist = dist; a.mask_buffer = mask_buffer;
    a.counters = ix.counters;
    const unsigned long long blocks = (a.n_tiles + (COAST_TPB / 64) - 1) / (COAST_TPB / 64);
    if (blocks > 0x7fffffffull) return set_error(HZ_ERR_ARG, "grid of %d x %d cells is too large", len_0, len_1);
    if (any_hit) hipLaunchKernelGGL(k_coast_query<true>, dim3((unsigned)blocks), dim3(COAST_TPB), 0, st, a);
    else hipLaunchKernelGGL(k_coast_query<false>, dim3((unsigned)blocks), dim3(COAST_TPB), 0, st, a);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
