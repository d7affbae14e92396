// hz_subgrid.hip -- Terrain.sw_dir_cor_coarse (hz_terrain_sw_dir_cor_coarse): block means of sw_dir_cor and of the sunlit
// flag per sun position over p0 x p1 cells of the inner domain, for gfx950.
//
// The positions are traced in chunks exactly as for Terrain.accumulate (hz_shadow.hip: k_accum_refill into scratch
// [k][cells]: a u8 shadow code and / or the f32 correction factor).  k_coarse_count counts the unmasked cells n of every
// coarse cell once per call; k_coarse_reduce turns one chunk of scratch into [k][gy][gx] means.
//
// Contract (include/horayzon_hip.h): the sum of a coarse cell is a float64 accumulator that starts
// at 0.0 and takes (double)sw_dir_cor of the block's unmasked cells one at a time, rows ascending and within a row columns
// ascending.  So ONE lane adds all cells of a block, in that order.  A cell that is masked, or not lit, contributes
// +0.0 instead of being skipped: the accumulator starts at +0.0 and a round-to-nearest sum is -0.0 only if both operands
// are, so it is never -0.0 and `x + 0.0` leaves every bit of it as it is (what sw_dir_cor writes for a cell that is not
// lit is 0.0f itself).  The data-dependent part is thereby done where the cell is loaded, and the ordered part is a
// plain chain of adds.
#include "hz_internal.h"
#include <algorithm>

namespace hz {

std::atomic<int> g_coarse_tile{0};

#define HZ_COARSE_TPB 256
// Cells of one LDS tile.  4 B value + 1 B lit flag = 20 KiB per workgroup: 8 workgroups (all 32 waves) per CU of 160 KiB,
// so that the loads of some overlap the ordered adds of the others.  A row of the 3569-column tile fits (83 blocks of 43).
#define HZ_COARSE_TILE 4096

// n[I][J] = unmasked cells of coarse cell (I, J).  One lane per (row i, coarse column J) counts p1 consecutive bytes (a wave
// reads 64 * p1 consecutive bytes) and adds its count to the coarse cell: integer sums, the order does not matter.
__global__ __launch_bounds__(HZ_COARSE_TPB) void k_coarse_count(const uint8_t *__restrict__ mask, int dim_0, int dim_1, int p0,
                                                                int p1, int gx, unsigned *__restrict__ n) {
    const size_t t = (size_t)blockIdx.x * HZ_COARSE_TPB + threadIdx.x;
    if (t >= (size_t)dim_0 * gx) return;
    const int i = (int)(t / (size_t)gx), J = (int)(t - (size_t)i * gx);
    const uint8_t *row = mask + (size_t)i * dim_1 + (size_t)J * p1;
    unsigned cnt = 0;
    for (int dj = 0; dj < p1; dj++) cnt += row[dj] == 1 ? 1u : 0u;
    if (cnt) atomicAdd(&n[(size_t)(i / p0) * gx + J], cnt);
}

struct CoarseParams {
    const uint8_t *codes;    // chunk scratch u8[k][cells] or null (f_cor alone)
    const float *vals;       // chunk scratch f32[k][cells] or null (sunlit_frac alone); with codes: valid where code == 0 only
    const uint8_t *mask;     // u8[cells]: block membership
    const unsigned *n;       // u32[gy][gx], k_coarse_count
    size_t cells;
    int dim_1, p0, p1, gy, gx;
    int nb, rows, nstrips;   // k_coarse_reduce: coarse cells per strip, rows per LDS tile, strips per coarse row
    int lx;                  // log2 of the threads along a tile row (the others go over the rows)
    float fill;
    float *f_cor, *lit;      // [k][gy][gx] at the chunk's first position, or null
};

__device__ __forceinline__ void coarse_store(const CoarseParams &p, int q, int I, int J, double sum, unsigned n_lit) {
    const unsigned n = p.n[(size_t)I * p.gx + J];
    const size_t at = ((size_t)q * p.gy + I) * p.gx + J;
    if (p.f_cor) p.f_cor[at] = n ? (float)(sum / (double)n) : p.fill;
    if (p.lit) p.lit[at] = n ? (float)((double)n_lit / (double)n) : p.fill;
}

// One workgroup: position q = blockIdx.y, coarse row I, a strip of up to nb coarse cells.  The strip's p0 rows go through
// LDS `rows` at a time: every thread loads along the rows (coalesced: mask, code, value of consecutive cells), writes the
// value that the cell contributes and its lit flag, and after the barrier lane b adds block b's part of the tile in row-major
// order to its float64 accumulator, which lives in a register across the tiles.  Neighbouring lanes read LDS p1 words apart.
template <bool CODES, bool VALS>
__global__ __launch_bounds__(HZ_COARSE_TPB) void k_coarse_reduce(CoarseParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int I = (int)(blockIdx.x / (unsigned)p.nstrips), strip = (int)(blockIdx.x - (unsigned)I * p.nstrips);
    const int J0 = strip * p.nb, nbc = min(p.nb, p.gx - J0);
    const int W = nbc * p.p1, Wm = p.nb * p.p1;                    // columns of this strip / pitch of a tile row
    float *const lv = reinterpret_cast<float *>(smem);
    uint8_t *const lf = smem + (VALS ? (size_t)p.rows * Wm * sizeof(float) : 0);
    const size_t pos = (size_t)q * p.cells;
    const int tx = 1 << p.lx, c0 = tid & (tx - 1), ry = tid >> p.lx, ty = HZ_COARSE_TPB >> p.lx;
    double sum = 0.0;
    unsigned n_lit = 0;
    for (int r0 = 0; r0 < p.p0; r0 += p.rows) {
        const int rc = min(p.rows, p.p0 - r0);
        for (int r = ry; r < rc; r += ty) {
            const size_t row = (size_t)(I * p.p0 + r0 + r) * p.dim_1 + (size_t)J0 * p.p1;
#pragma unroll 4
            for (int c = c0; c < W; c += tx) {
                const size_t cell = row + c;
                bool on = p.mask[cell] == 1;
                if (CODES) on = on && p.codes[pos + cell] == 0;
                if (VALS) lv[r * Wm + c] = on ? p.vals[pos + cell] : 0.0f;
                if (CODES) lf[r * Wm + c] = on ? 1 : 0;
            }
        }
        __syncthreads();
        if (tid < nbc) {
            for (int r = 0; r < rc; r++) {
                const int at = r * Wm + tid * p.p1;
                for (int dj = 0; dj < p.p1; dj++) {
                    if (VALS) sum += (double)lv[at + dj];
                    if (CODES) n_lit += lf[at + dj];
                }
            }
        }
        __syncthreads();
    }
    if (tid < nbc) coarse_store(p, q, I, J0 + tid, sum, n_lit);
}

// Blocks wider than an LDS tile (p1 > tile cells): one lane per (position, coarse cell) walks its block in global memory.
template <bool CODES, bool VALS>
__global__ __launch_bounds__(HZ_COARSE_TPB) void k_coarse_reduce_direct(CoarseParams p) {
    const size_t t = (size_t)blockIdx.x * HZ_COARSE_TPB + threadIdx.x;
    if (t >= (size_t)p.gy * p.gx) return;
    const int q = blockIdx.y;
    const int I = (int)(t / (size_t)p.gx), J = (int)(t - (size_t)I * p.gx);
    const size_t pos = (size_t)q * p.cells;
    double sum = 0.0;
    unsigned n_lit = 0;
    for (int di = 0; di < p.p0; di++) {
        const size_t row = (size_t)(I * p.p0 + di) * p.dim_1 + (size_t)J * p.p1;
        for (int dj = 0; dj < p.p1; dj++) {
            const size_t cell = row + dj;
            bool on = p.mask[cell] == 1;
            if (CODES) on = on && p.codes[pos + cell] == 0;
            if (VALS) sum += (double)(on ? p.vals[pos + cell] : 0.0f);
            if (CODES) n_lit += on ? 1u : 0u;
        }
    }
    coarse_store(p, q, I, J, sum, n_lit);
}

int coarse_count_launch(const uint8_t *mask, int dim_0, int dim_1, int p0, int p1, unsigned *n, hipStream_t st) {
    const int gy = dim_0 / p0, gx = dim_1 / p1;
    HZ_HIP(hipMemsetAsync(n, 0, (size_t)gy * gx * sizeof(unsigned), st));
    const size_t lanes = (size_t)dim_0 * gx;
    hipLaunchKernelGGL(k_coarse_count, dim3((unsigned)((lanes + HZ_COARSE_TPB - 1) / HZ_COARSE_TPB)), dim3(HZ_COARSE_TPB), 0, st,
                       mask, dim_0, dim_1, p0, p1, gx, n);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int coarse_reduce_launch(const uint8_t *codes, const float *vals, const uint8_t *mask, const unsigned *n, int dim_0, int dim_1,
                         int p0, int p1, int k, float fill, float *f_cor, float *lit, hipStream_t st) {
    if (k <= 0) return HZ_OK;
    if ((f_cor && !vals) || (lit && !codes) || (!codes && !vals)) return set_error(HZ_ERR_ARG, "coarse_reduce_launch: scratch does not match the outputs");
    CoarseParams p;
    p.codes = codes; p.vals = vals; p.mask = mask; p.n = n;
    p.cells = (size_t)dim_0 * dim_1;
    p.dim_1 = dim_1; p.p0 = p0; p.p1 = p1; p.gy = dim_0 / p0; p.gx = dim_1 / p1;
    p.fill = fill; p.f_cor = f_cor; p.lit = lit;
    int tile = g_coarse_tile.load(std::memory_order_relaxed);
    if (tile <= 0) tile = HZ_COARSE_TILE;
    tile = std::min(tile, HZ_COARSE_TILE);
    const bool direct = p1 > tile;
    dim3 grid;
    size_t lds = 0;
    if (direct) {
        p.nb = p.rows = p.nstrips = 1; p.lx = 0;
        grid = dim3((unsigned)(((size_t)p.gy * p.gx + HZ_COARSE_TPB - 1) / HZ_COARSE_TPB), (unsigned)k);
    } else {
        const int nb_max = std::max(1, std::min(std::min(p.gx, HZ_COARSE_TPB), tile / p1));
        p.nstrips = (p.gx + nb_max - 1) / nb_max;
        p.nb = (p.gx + p.nstrips - 1) / p.nstrips;                 // strips of equal width (the last one may be shorter)
        p.nstrips = (p.gx + p.nb - 1) / p.nb;
        const int wm = p.nb * p1;
        p.rows = std::max(1, std::min(p0, tile / wm));
        p.lx = 0;
        while ((1 << p.lx) < std::min(wm, HZ_COARSE_TPB)) p.lx++;
        if ((size_t)p.gy * p.nstrips > 0x7fffffffull) return set_error(HZ_ERR_ARG, "too many coarse cells for one launch");
        grid = dim3((unsigned)((size_t)p.gy * p.nstrips), (unsigned)k);
        lds = (size_t)p.rows * wm * ((vals ? sizeof(float) : 0) + (codes ? 1 : 0));
    }
#define HZ_LAUNCH_COARSE(C, V)                                                                                          \
    do {                                                                                                                \
        if (direct) hipLaunchKernelGGL((k_coarse_reduce_direct<C, V>), grid, dim3(HZ_COARSE_TPB), 0, st, p);            \
        else hipLaunchKernelGGL((k_coarse_reduce<C, V>), grid, dim3(HZ_COARSE_TPB), lds, st, p);                        \
    } while (0)
    if (codes && vals) HZ_LAUNCH_COARSE(true, true);
    else if (codes) HZ_LAUNCH_COARSE(true, false);
    else HZ_LAUNCH_COARSE(false, true);
#undef HZ_LAUNCH_COARSE
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
