// hz_horidist.hip -- the distance to the horizon of a gridded horizon (gfx950; DESIGN.md section 4, clause 16).
//
// Input: a horizon of the inner domain -- float32 or 16-bit codes (hz_q16.h), cell-major or as planes -- and the scene it
// was computed on.  Per cell with mask == 1 and azimuth a: j = the last entry of the ascending elevation table that is
// <= the horizon value, k = max(j - 5, 0) (for guess_constant the last ray that hit), and the distance is hz_closest's for
// the ray of table entry k and azimuth a, i.e. the minimum t over all triangles accepted with tfar = dist_search.  NaN where
// that ray hits nothing, where the horizon value is NaN and where mask != 1.  The output has the layout of the input.
//
// Organisation: one wave = one workgroup owns a block of 64 cells (8 x 8; `block_w` x 64 / block_w in general) and walks the
// azimuths in order, so the 64 closest-hit rays of a step share an azimuth and start from neighbouring cells: they open the
// same nodes.  The frame (east, north, norm, origin) is set up once per cell.  The traversal is hz_closest's plain per-lane
// loop (stack of individual child links: up to 3 per tree level) with the children of a node visited front to back
// (hd_closest_near_first, hz_closest_order.h: -31 % on the 3601^2 tile, same words); hz_closest itself stays selectable for
// same-call A/Bs.
//
// LDS and occupancy: the stack is 3 x height entries x 64 lanes x 4 B per workgroup -- 9.75 KiB at the height (13) of the
// 3601^2 tile, so 16 workgroups = 16 waves fit the 160 KiB of a CU (4 per SIMD), the same residency four workgroups of 256
// threads with 39 KiB each would have; one wave per workgroup keeps the worst case (height 40: 30 KiB) far from the limit
// of a workgroup and needs no barrier.  At 4 waves per SIMD the register budget is 128 VGPRs; see DESIGN.md section 5 for
// the compiler's resource line.
//
// Memory: cell-major, a lane owns a contiguous row of azim_num values.  The row is cut at the 16-byte boundaries of the
// DISTANCE row (pieces of four values; the first and last piece of a row may be shorter: azim_num need not be a multiple
// of four and a row may start at any element).  A full piece is one 16-byte store, and one 16-byte (float32) or 8-byte
// (codes) load where the horizon address is aligned as well; everything else moves element by element.  Planes: one
// azimuth of the block is `64 / block_w` runs of block_w consecutive cells.
#include "hz_internal.h"
#include "hz_q16.h"
#include "hz_closest_order.h"

namespace hz {

#define HZ_HD_TPB 64

#define HZ_HD_TRAVERSAL_DEFAULT 1
// hz_debug_set("horidist_traversal", 0 | 1): 0 = hz_closest as it is, 1 = the children of a node front to back (same-call A/Bs)
std::atomic<int> g_horidist_traversal{HZ_HD_TRAVERSAL_DEFAULT};
std::atomic<int> g_horidist_block_w{8};      // hz_debug_set("horidist_block_w", 8 | 16 | 32 | 64) (hz_internal.h)

struct HoridistParams {
    SceneView sv;
    const float *azim_sin, *azim_cos, *elev_ang, *elev_sin, *elev_cos;
    int azim_num, elev_num;
    float up, inv_step;                  // upper table limit [radian], 1 / table step: the arithmetic guess of the table index
    const float *vec_norm, *vec_north;   // indexed by the cell of the inner domain
    const uint8_t *mask;
    const void *hori;                    // cell c (from 0 at the launch's first row), azimuth a: cell-major element c * azim_num + a,
    float *dist;                         //   planes a * stride + cell0 + c (strides and first cells per array)
    size_t hori_stride, hori_cell0, dist_stride, dist_cell0;
    int offset_0, offset_1, dim_in_1, row_begin, row_end;
    int bw_log2, tiles_j;                // block of cells: 2^bw_log2 wide, 64 >> bw_log2 high
    float ray_org_elev, tfar;
    unsigned long long *counters;        // [0] distance rays, [1] cells with mask == 1
};

__device__ __forceinline__ float hd_value(float v) { return v; }
__device__ __forceinline__ float hd_value(uint16_t q) { return q16_decode(q); }

// elements b ... b + 3 of a row of n (those outside [0, n) are left alone) as the four components of v
__device__ __forceinline__ void hd_load_piece(const float *row, int b, int n, float4 &v) {
    if (b >= 0 && b + 4 <= n && (reinterpret_cast<uintptr_t>(row + b) & 15) == 0) {
        v = *reinterpret_cast<const float4 *>(row + b);
        return;
    }
    if (b >= 0 && b < n) v.x = row[b];
    if (b + 1 >= 0 && b + 1 < n) v.y = row[b + 1];
    if (b + 2 >= 0 && b + 2 < n) v.z = row[b + 2];
    if (b + 3 >= 0 && b + 3 < n) v.w = row[b + 3];
}
__device__ __forceinline__ void hd_load_piece(const uint16_t *row, int b, int n, float4 &v) {
    if (b >= 0 && b + 4 <= n && (reinterpret_cast<uintptr_t>(row + b) & 7) == 0) {
        const uint2 w = *reinterpret_cast<const uint2 *>(row + b);
        v.x = q16_decode((uint16_t)(w.x & 0xffffu)); v.y = q16_decode((uint16_t)(w.x >> 16));
        v.z = q16_decode((uint16_t)(w.y & 0xffffu)); v.w = q16_decode((uint16_t)(w.y >> 16));
        return;
    }
    if (b >= 0 && b < n) v.x = q16_decode(row[b]);
    if (b + 1 >= 0 && b + 1 < n) v.y = q16_decode(row[b + 1]);
    if (b + 2 >= 0 && b + 2 < n) v.z = q16_decode(row[b + 2]);
    if (b + 3 >= 0 && b + 3 < n) v.w = q16_decode(row[b + 3]);
}
// (a full piece starts at a 16-byte boundary of the distance row by construction)
__device__ __forceinline__ void hd_store_piece(float *row, int b, int n, const float4 &v) {
    if (b >= 0 && b + 4 <= n) {
        *reinterpret_cast<float4 *>(row + b) = v;
        return;
    }
    if (b >= 0 && b < n) row[b] = v.x;
    if (b + 1 >= 0 && b + 1 < n) row[b + 1] = v.y;
    if (b + 2 >= 0 && b + 2 < n) row[b + 2] = v.z;
    if (b + 3 >= 0 && b + 3 < n) row[b + 3] = v.w;
}

// max{ i : elev_ang[i] <= h }, -1 if there is none (h is not NaN): an arithmetic guess -- entry n - 1 - i is up - step * i --
// and a walk to the neighbouring entries that ends at the maximum whatever the guess was (the table ascends strictly)
__device__ __forceinline__ int hd_table_index(const float *__restrict__ elev_ang, int n, float up, float inv_step, float h) {
    const float g = __builtin_fminf(__builtin_fmaxf((up - h) * inv_step, -1.0f), (float)n);
    int idx = min(max(n - 1 - (int)g, -1), n - 1);
    while (idx + 1 < n && elev_ang[idx + 1] <= h) idx++;
    while (idx >= 0 && elev_ang[idx] > h) idx--;
    return idx;
}

template <typename T, bool PLANES, int MODE>
__global__ __launch_bounds__(HZ_HD_TPB) void k_horidist(HoridistParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *stack = reinterpret_cast<int *>(smem);
    const int lane = threadIdx.x;
    const int ti = (int)(blockIdx.x / (unsigned)p.tiles_j), tj = (int)(blockIdx.x % (unsigned)p.tiles_j);
    const int i = p.row_begin + ti * (64 >> p.bw_log2) + (lane >> p.bw_log2);
    const int j = (tj << p.bw_log2) + (lane & ((1 << p.bw_log2) - 1));
    const bool in_dom = i < p.row_end && j < p.dim_in_1;
    const size_t cell = in_dom ? (size_t)i * p.dim_in_1 + j : 0;                       // of the inner domain
    const size_t c = in_dom ? (size_t)(i - p.row_begin) * p.dim_in_1 + j : 0;          // of this launch
    const bool live = in_dom && p.mask[cell] == 1;
    const int A = p.azim_num;
    // the frame, once per cell: the origin of the gridded horizon and k_locations' rotation (east = north x norm)
    float ox = 0, oy = 0, oz = 0;
    float r00 = 0, r01 = 0, r02 = 0, r10 = 0, r11 = 0, r12 = 0, r20 = 0, r21 = 0, r22 = 1;
    if (live) {
        const float norm_x = p.vec_norm[3 * cell], norm_y = p.vec_norm[3 * cell + 1], norm_z = p.vec_norm[3 * cell + 2];
        const float north_x = p.vec_north[3 * cell], north_y = p.vec_north[3 * cell + 1], north_z = p.vec_north[3 * cell + 2];
        const float *v = p.sv.verts + 3 * ((size_t)(i + p.offset_0) * p.sv.d1 + (size_t)(j + p.offset_1));
        ox = v[0] + norm_x * p.ray_org_elev;
        oy = v[1] + norm_y * p.ray_org_elev;
        oz = v[2] + norm_z * p.ray_org_elev;
        const float east_x = north_y * norm_z - north_z * norm_y;
        const float east_y = north_z * norm_x - north_x * norm_z;
        const float east_z = north_x * norm_y - north_y * norm_x;
        r00 = east_x; r01 = north_x; r02 = norm_x;
        r10 = east_y; r11 = north_y; r12 = norm_y;
        r20 = east_z; r21 = north_z; r22 = norm_z;
    }
    const float ocx = ox - p.sv.cx, ocy = oy - p.sv.cy, ocz = oz - p.sv.cz;
    const float tau = p.sv.tau;
    const T *hrow = static_cast<const T *>(p.hori) + (PLANES ? p.hori_cell0 + c : c * (size_t)A);
    float *drow = p.dist + (PLANES ? p.dist_cell0 + c : c * (size_t)A);
    const int w0 = (int)((reinterpret_cast<uintptr_t>(drow) >> 2) & 3);      // cell-major: place of element 0 in its piece
    const float nan = __builtin_nanf("");
    float4 hv = make_float4(nan, nan, nan, nan), dv = make_float4(nan, nan, nan, nan);
    unsigned rays = 0;
    for (int a = 0; a < A; a++) {
        const int q = PLANES ? 0 : ((w0 + a) & 3);
        float h = nan;
        if (PLANES) {
            if (live) h = hd_value(hrow[(size_t)a * p.hori_stride]);
        } else {
            if (live && (q == 0 || a == 0)) hd_load_piece(hrow, a - q, A, hv);
            h = q == 0 ? hv.x : (q == 1 ? hv.y : (q == 2 ? hv.z : hv.w));
        }
        float d = nan;
        if (live && h == h) {
            const int k = max(hd_table_index(p.elev_ang, p.elev_num, p.up, p.inv_step, h) - 5, 0);
            const float ec = p.elev_cos[k], es = p.elev_sin[k];
            const float rx = ec * p.azim_sin[a], ry = ec * p.azim_cos[a], rz = es;
            const float dx = (r00 * rx + r01 * ry) + r02 * rz;
            const float dy = (r10 * rx + r11 * ry) + r12 * rz;
            const float dz = (r20 * rx + r21 * ry) + r22 * rz;
            const RayBox rb = hz_raybox(ocx - tau * dx, ocy - tau * dy, ocz - tau * dz, dx, dy, dz);
            float t = 0.0f;
            const bool hit = MODE != 0
                ? hd_closest_near_first<HZ_HD_TPB>(p.sv.nodes, p.sv.prims, stack, lane, ox, oy, oz, dx, dy, dz, p.tfar, tau, rb, &t)
                : hz_closest<HZ_HD_TPB>(p.sv.nodes, p.sv.prims, stack, lane, ox, oy, oz, dx, dy, dz, p.tfar, tau, rb, &t);
            if (hit) d = t;
            rays++;
        }
        if (PLANES) {
            if (in_dom) drow[(size_t)a * p.dist_stride] = d;
        } else {
            dv.x = q == 0 ? d : dv.x; dv.y = q == 1 ? d : dv.y; dv.z = q == 2 ? d : dv.z; dv.w = q == 3 ? d : dv.w;
            if (in_dom && (q == 3 || a == A - 1)) hd_store_piece(drow, a - q, A, dv);
        }
    }
    unsigned long long r = rays, n = live ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) { r += __shfl_xor(r, off); n += __shfl_xor(n, off); }
    if (lane == 0) {
        if (r) atomicAdd(&p.counters[0], r);
        if (n) atomicAdd(&p.counters[1], n);
    }
}

template <typename T, bool PLANES, int MODE>
static int launch3(const HoridistParams &p, unsigned grid, size_t lds, hipStream_t st) {
    HZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_horidist<T, PLANES, MODE>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_horidist<T, PLANES, MODE>), dim3(grid), dim3(HZ_HD_TPB), lds, st, p);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

template <typename T, bool PLANES>
static int launch(const HoridistParams &p, unsigned grid, size_t lds, hipStream_t st) {
    int mode = g_horidist_traversal.load(std::memory_order_relaxed);
    if (mode < 0) mode = HZ_HD_TRAVERSAL_DEFAULT;
    return mode == 0 ? launch3<T, PLANES, 0>(p, grid, lds, st) : launch3<T, PLANES, 1>(p, grid, lds, st);
}

int horidist_launch(const Scene *sc, const HoridistArgs &a, hipStream_t st) {
    if (a.row_end <= a.row_begin || a.dim_in_1 <= 0 || a.azim_num <= 0) return HZ_OK;
    if (a.block_w != 8 && a.block_w != 16 && a.block_w != 32 && a.block_w != 64)
        return set_error(HZ_ERR_ARG, "horidist: block width %d (8, 16, 32 or 64)", a.block_w);
    HoridistParams p;
    p.sv = scene_view(sc);
    p.azim_sin = a.azim_sin; p.azim_cos = a.azim_cos; p.elev_ang = a.elev_ang; p.elev_sin = a.elev_sin; p.elev_cos = a.elev_cos;
    p.azim_num = a.azim_num; p.elev_num = a.elev_num;
    p.up = a.up; p.inv_step = 5.0f / a.hori_acc;
    p.vec_norm = a.vec_norm; p.vec_north = a.vec_north; p.mask = a.mask;
    p.hori = a.hori; p.dist = a.dist;
    p.hori_stride = a.hori_stride; p.hori_cell0 = a.hori_cell0; p.dist_stride = a.dist_stride; p.dist_cell0 = a.dist_cell0;
    p.offset_0 = a.offset_0; p.offset_1 = a.offset_1; p.dim_in_1 = a.dim_in_1; p.row_begin = a.row_begin; p.row_end = a.row_end;
    p.bw_log2 = a.block_w == 8 ? 3 : (a.block_w == 16 ? 4 : (a.block_w == 32 ? 5 : 6));
    const int bh = 64 / a.block_w;
    p.tiles_j = (a.dim_in_1 + a.block_w - 1) / a.block_w;
    const size_t tiles = (size_t)((a.row_end - a.row_begin + bh - 1) / bh) * (size_t)p.tiles_j;
    if (tiles > 0x7fffffffu) return set_error(HZ_ERR_ARG, "horidist: %zu blocks of cells in one launch", tiles);
    p.ray_org_elev = a.ray_org_elev; p.tfar = a.dist_m;
    p.counters = a.counters;
    // hz_closest keeps individual child links: up to 3 per tree level
    const size_t lds = (size_t)(3 * std::max(sc->hdr.height, 1)) * HZ_HD_TPB * 4;
    const unsigned grid = (unsigned)tiles;
    if (a.q16) return a.planes ? launch<uint16_t, true>(p, grid, lds, st) : launch<uint16_t, false>(p, grid, lds, st);
    return a.planes ? launch<float, true>(p, grid, lds, st) : launch<float, false>(p, grid, lds, st);
}

}  // namespace hz
