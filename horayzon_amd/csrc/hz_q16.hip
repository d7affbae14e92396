// hz_q16.hip -- the 16-bit horizon code (clause 15; hz_q16.h): the elementwise encoder and decoder and
// the transposing encoder of the horizon call.
//
// The code is elementwise, so it commutes with the transposition of clause 11: planes_q[k][y][x] and hori_q[y][x][k] hold
// the same 16-bit word.  A destination of 16-bit words is 2-byte aligned and nothing more (a view at an odd element, an odd
// plane stride, an odd first cell), so every packed store here is chosen from the address: k_hori_quantise stores 8 bytes per
// lane from the first 8-byte boundary on and single words before it and after the last full group; k_hori_quantise_planes
// shifts a row's pairs of cells by one where the row starts at an odd word.
#include "hz_internal.h"
#include "hz_q16.h"

namespace hz {

#define HZ_Q16_TPB 256
#define HZ_Q16_PER_LANE 4                // values per lane and pass of the elementwise kernels
#define HZ_Q16_MAX_BLOCKS 16384u         // grid-stride loops: any length fits a launch

// dst[i] = encode(src[i]).  Elements [0, head) and [head + 4 * groups, n) -- fewer than four each -- are single 16-bit
// stores of the first block's lanes; group g is elements head + 4 g ... + 3, one 8-byte store at an 8-byte boundary.
// src_vec: src + head is 16-byte aligned, a group is one 16-byte load.
__global__ __launch_bounds__(HZ_Q16_TPB) void k_hori_quantise(const float *__restrict__ src, size_t n, uint16_t *__restrict__ dst,
                                                              size_t head, size_t groups, int src_vec) {
    const size_t lanes = (size_t)gridDim.x * HZ_Q16_TPB;
    const size_t tid = (size_t)blockIdx.x * HZ_Q16_TPB + threadIdx.x;
    for (size_t g = tid; g < groups; g += lanes) {
        const size_t i = head + HZ_Q16_PER_LANE * g;
        float v0, v1, v2, v3;
        if (src_vec) {
            const float4 v = *reinterpret_cast<const float4 *>(src + i);
            v0 = v.x; v1 = v.y; v2 = v.z; v3 = v.w;
        } else {
            v0 = src[i]; v1 = src[i + 1]; v2 = src[i + 2]; v3 = src[i + 3];
        }
        uint2 w;
        w.x = (uint32_t)q16_encode(v0) | ((uint32_t)q16_encode(v1) << 16);
        w.y = (uint32_t)q16_encode(v2) | ((uint32_t)q16_encode(v3) << 16);
        *reinterpret_cast<uint2 *>(dst + i) = w;
    }
    const size_t body_end = head + HZ_Q16_PER_LANE * groups;
    if (tid < head + (n - body_end)) {                  // the ragged ends
        const size_t i = tid < head ? tid : body_end + (tid - head);
        dst[i] = q16_encode(src[i]);
    }
}

// dst[i] = decode(src[i]): the groups start at the first 16-byte boundary of dst and are one 16-byte store each.
// src_vec: src + head is 8-byte aligned, a group is one 8-byte load.
__global__ __launch_bounds__(HZ_Q16_TPB) void k_hori_dequantise(const uint16_t *__restrict__ src, size_t n, float *__restrict__ dst,
                                                                size_t head, size_t groups, int src_vec) {
    const size_t lanes = (size_t)gridDim.x * HZ_Q16_TPB;
    const size_t tid = (size_t)blockIdx.x * HZ_Q16_TPB + threadIdx.x;
    for (size_t g = tid; g < groups; g += lanes) {
        const size_t i = head + HZ_Q16_PER_LANE * g;
        uint16_t q0, q1, q2, q3;
        if (src_vec) {
            const uint2 w = *reinterpret_cast<const uint2 *>(src + i);
            q0 = (uint16_t)(w.x & 0xffffu); q1 = (uint16_t)(w.x >> 16); q2 = (uint16_t)(w.y & 0xffffu); q3 = (uint16_t)(w.y >> 16);
        } else {
            q0 = src[i]; q1 = src[i + 1]; q2 = src[i + 2]; q3 = src[i + 3];
        }
        float4 v;
        v.x = q16_decode(q0); v.y = q16_decode(q1); v.z = q16_decode(q2); v.w = q16_decode(q3);
        *reinterpret_cast<float4 *>(dst + i) = v;
    }
    const size_t body_end = head + HZ_Q16_PER_LANE * groups;
    if (tid < head + (n - body_end)) {
        const size_t i = tid < head ? tid : body_end + (tid - head);
        dst[i] = q16_decode(src[i]);
    }
}

// elements before the first `align`-byte boundary of p (elements of `size` bytes, p a multiple of `size`), at most n
static size_t q16_head(const void *p, size_t align, size_t size, size_t n) {
    const size_t off = (size_t)(reinterpret_cast<uintptr_t>(p) & (align - 1));
    return std::min(n, off ? (align - off) / size : 0);
}

static unsigned q16_blocks(size_t groups) {
    return (unsigned)std::min<size_t>(std::max<size_t>(1, (groups + HZ_Q16_TPB - 1) / HZ_Q16_TPB), HZ_Q16_MAX_BLOCKS);
}

int hori_quantise_launch(const float *src, size_t n, uint16_t *dst, hipStream_t st) {
    if (n == 0) return HZ_OK;
    const size_t head = q16_head(dst, 8, sizeof(uint16_t), n);
    const size_t groups = (n - head) / HZ_Q16_PER_LANE;
    const int src_vec = (reinterpret_cast<uintptr_t>(src + head) & 15) == 0;
    hipLaunchKernelGGL(k_hori_quantise, dim3(q16_blocks(groups)), dim3(HZ_Q16_TPB), 0, st, src, n, dst, head, groups, src_vec);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int hori_dequantise_launch(const uint16_t *src, size_t n, float *dst, hipStream_t st) {
    if (n == 0) return HZ_OK;
    const size_t head = q16_head(dst, 16, sizeof(float), n);
    const size_t groups = (n - head) / HZ_Q16_PER_LANE;
    const int src_vec = (reinterpret_cast<uintptr_t>(src + head) & 7) == 0;
    hipLaunchKernelGGL(k_hori_dequantise, dim3(q16_blocks(groups)), dim3(HZ_Q16_TPB), 0, st, src, n, dst, head, groups, src_vec);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

// ---- the transposing encoder: k_hori_to_planes (hz_planes.hip) with encode on the way out -------------------------------

#define HZ_Q16_TC 64                     // cells of a tile
#define HZ_Q16_TA 32                     // azimuths of a tile

struct QuantPlanesArgs {
    const uint32_t *src;                 // hori f32[cells][A], as words
    uint16_t *dst;                       // cell c of azimuth k is element k * plane_stride + cell0 + c
    size_t cells, plane_stride, cell0;
    size_t tiles;                        // tiles_c * tiles_a
    int azim_num, tiles_a;
};

// The tile is read as k_hori_to_planes reads it: a half-wave takes the 32 azimuths of one cell.  On the way out a half-wave
// takes the 64 cells of one azimuth, two cells per lane and one 32-bit store where both exist: the pairs start at the tile's
// cell 0 when that element of dst lies on a 4-byte boundary, and at cell 1 when it does not (lane 0 then stores cell 0 on
// its own, and lane 31 the tile's last cell).  The boundary is looked up per row: with an odd plane stride it alternates.
__global__ __launch_bounds__(HZ_Q16_TPB) void k_hori_quantise_planes(QuantPlanesArgs p) {
    __shared__ uint32_t tile[HZ_Q16_TA][HZ_Q16_TC + 1];
    const int t = threadIdx.x;
    const int ra = t % HZ_Q16_TA, rc = t / HZ_Q16_TA;            // cell-major side: azimuth fastest, 8 cells per pass
    const int pl = t % (HZ_Q16_TC / 2), pa = t / (HZ_Q16_TC / 2);   // plane side: pair of cells fastest, 8 azimuths per pass
    const size_t A = (size_t)p.azim_num;
    const size_t dst_word = (size_t)(reinterpret_cast<uintptr_t>(p.dst) >> 1);
    for (size_t tl = blockIdx.x; tl < p.tiles; tl += gridDim.x) {
        const size_t cb = (tl / (size_t)p.tiles_a) * HZ_Q16_TC;
        const int ab = (int)(tl % (size_t)p.tiles_a) * HZ_Q16_TA;
        for (int i = rc; i < HZ_Q16_TC; i += HZ_Q16_TPB / HZ_Q16_TA) {
            const size_t c = cb + (size_t)i;
            if (c < p.cells && ab + ra < p.azim_num) tile[ra][i] = p.src[c * A + (size_t)(ab + ra)];
        }
        __syncthreads();
        for (int k = pa; k < HZ_Q16_TA; k += HZ_Q16_TPB / (HZ_Q16_TC / 2)) {
            if (ab + k >= p.azim_num) break;
            const size_t e0 = (size_t)(ab + k) * p.plane_stride + p.cell0 + cb;      // the tile's cell 0 in dst
            const int odd = (int)((dst_word + e0) & 1);
            const int s = 2 * pl + odd;                           // the lane's first cell of the tile
            const bool v0 = s < HZ_Q16_TC && cb + (size_t)s < p.cells;
            const bool v1 = s + 1 < HZ_Q16_TC && cb + (size_t)s + 1 < p.cells;
            if (v0 && v1) {
                const uint32_t w = (uint32_t)q16_encode(__uint_as_float(tile[k][s])) |
                                   ((uint32_t)q16_encode(__uint_as_float(tile[k][s + 1])) << 16);
                *reinterpret_cast<uint32_t *>(p.dst + e0 + (size_t)s) = w;
            } else if (v0) {
                p.dst[e0 + (size_t)s] = q16_encode(__uint_as_float(tile[k][s]));
            }
            if (odd && pl == 0 && cb < p.cells) p.dst[e0] = q16_encode(__uint_as_float(tile[k][0]));
        }
        __syncthreads();                 // the tile is filled again in the next pass
    }
}

int hori_quantise_planes_launch(const float *hori, size_t cells, int azim_num, uint16_t *planes_q, size_t plane_stride,
                                size_t cell0, hipStream_t st) {
    if (cells == 0 || azim_num <= 0) return HZ_OK;
    QuantPlanesArgs p;
    p.src = reinterpret_cast<const uint32_t *>(hori); p.dst = planes_q;
    p.cells = cells; p.plane_stride = plane_stride; p.cell0 = cell0;
    p.azim_num = azim_num;
    p.tiles_a = (azim_num + HZ_Q16_TA - 1) / HZ_Q16_TA;
    p.tiles = ((cells + HZ_Q16_TC - 1) / HZ_Q16_TC) * (size_t)p.tiles_a;
    const unsigned blocks = (unsigned)std::min<size_t>(p.tiles, HZ_Q16_MAX_BLOCKS);
    hipLaunchKernelGGL(k_hori_quantise_planes, dim3(blocks), dim3(HZ_Q16_TPB), 0, st, p);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
