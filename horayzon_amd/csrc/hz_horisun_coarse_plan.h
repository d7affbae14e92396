// hz_horisun_coarse_plan.h -- launch plan of k_horisun_coarse (hz_horisun_coarse.hip), the fused kernel of
// hz_horizon_terrain_sw_dir_cor_coarse: plain C++, no HIP, so that the tiling arithmetic can be compiled into a stand-alone
// host program and run under a sanitizer (scripts/horisun_coarse_plan_check.cpp).
//
// One workgroup owns a coarse row I, a strip of `nb` coarse cells (nbc in the last strip) and one pass of up to `q` consecutive
// positions of the chunk (grid.y).  It walks the strip's p0 rows in tiles of `rows` rows; a tile is rows x (nb * p1) cells.
// Per tile the threads share the (position of the pass, cell of the tile) pairs evenly, whatever the tile's width, and write
// value and lit flag of each into LDS [q][rows][nb * p1]; then lane (b, position) adds block b's part of the tile in row-major
// order into its float64 sum and lit count, which stay in its registers from tile to tile.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hz {

#define HZ_HSC_TPB 256
// Cells of one LDS tile at most; "horisun_coarse_tile" lowers it.  A block wider than the tile goes the two-pass route.
#define HZ_HSC_TILE 4096
// Tiles of up to 512 cells are chosen whenever a block row fits (p1 <= 512): q = 8 positions of such a tile are 20 KiB of
// LDS, and a coarse row of the 3569-column tile is 8 strips, so a chunk of 48 positions is ~4000 workgroups of 43 tiles each.
// Wider blocks use tiles of up to HZ_HSC_TILE cells with fewer positions per pass.
#define HZ_HSC_PREF_CELLS 512
#define HZ_HSC_QMAX 8                    // positions per pass at most
#define HZ_HSC_LDS_MAPS 32768            // bytes of the [q][tile] values and flags at most (4096 cells * 5 B fit with q = 1)
#define HZ_HSC_CHUNK_MAX 4096            // positions per launch at most (grid.y <= 4096)

struct HorisunCoarsePlan {
    int fallback = 0;        // 1: the fused kernel does not take this shape (p1 > tile cells): two-pass route
    int gy = 0, gx = 0;      // coarse grid
    int nb = 0, nstrips = 0; // coarse cells per strip, strips per coarse row
    int rows = 0, ntiles = 0;// rows per tile, tiles per block
    int pitch = 0;           // cells of a tile in LDS: rows * nb * p1
    int q = 0;               // positions per pass = per workgroup
    unsigned grid_x = 0;     // gy * nstrips
    unsigned off_flags = 0;  // byte offset of the lit flags in dynamic LDS (the values are at 0)
    size_t lds_bytes = 0;
};

// grid.y for a chunk of k positions (k <= the chunk the plan was made for)
inline unsigned horisun_coarse_groups(const HorisunCoarsePlan &p, int k) { return (unsigned)((k + p.q - 1) / p.q); }

// 0: ok (p->fallback says which route); 1: an argument or a product is out of range (nothing is launched then).
// chunk = positions per launch (1 ... HZ_HSC_CHUNK_MAX), tile_knob > 0 lowers the tile (hz_debug_set("horisun_coarse_tile", n)),
// codes / vals = sunlit_frac / f_cor wanted.
inline int horisun_coarse_plan(int dim_0, int dim_1, int p0, int p1, int chunk, int tile_knob, bool codes, bool vals,
                               HorisunCoarsePlan *p) {
    *p = HorisunCoarsePlan();
    if (dim_0 <= 0 || dim_1 <= 0 || p0 < 1 || p1 < 1 || p0 > dim_0 || p1 > dim_1 || dim_0 % p0 || dim_1 % p1) return 1;
    if (chunk < 1 || chunk > HZ_HSC_CHUNK_MAX || (!codes && !vals)) return 1;
    p->gy = dim_0 / p0; p->gx = dim_1 / p1;
    int cap = tile_knob > 0 && tile_knob < HZ_HSC_TILE ? tile_knob : HZ_HSC_TILE;
    if (p1 > cap) { p->fallback = 1; return 0; }
    if (p1 <= HZ_HSC_PREF_CELLS && cap > HZ_HSC_PREF_CELLS) cap = HZ_HSC_PREF_CELLS;
    int nb_max = cap / p1;                                       // >= 1
    if (nb_max > p->gx) nb_max = p->gx;
    if (nb_max > HZ_HSC_TPB) nb_max = HZ_HSC_TPB;
    p->nstrips = (int)(((int64_t)p->gx + nb_max - 1) / nb_max);
    p->nb = (int)(((int64_t)p->gx + p->nstrips - 1) / p->nstrips);   // strips of equal width (the last one may be shorter)
    p->nstrips = (int)(((int64_t)p->gx + p->nb - 1) / p->nb);
    const int wm = p->nb * p1;                                   // <= cap
    p->rows = cap / wm;
    if (p->rows > p0) p->rows = p0;
    p->ntiles = (p0 + p->rows - 1) / p->rows;
    p->pitch = p->rows * wm;                                     // <= cap <= 4096
    const uint64_t gx64 = (uint64_t)p->gy * (uint64_t)p->nstrips;
    if (gx64 > 0x7fffffffull) return 1;                          // grid.x
    p->grid_x = (unsigned)gx64;
    const int cell_bytes = (vals ? 4 : 0) + (codes ? 1 : 0);
    int q = HZ_HSC_QMAX;
    if (q > HZ_HSC_TPB / p->nb) q = HZ_HSC_TPB / p->nb;          // one adding lane per (block, position of the pass)
    if (q > HZ_HSC_LDS_MAPS / (p->pitch * cell_bytes)) q = HZ_HSC_LDS_MAPS / (p->pitch * cell_bytes);
    if (q > chunk) q = chunk;
    p->q = q;                                                    // >= 1
    const size_t maps = (size_t)p->q * p->pitch;
    p->off_flags = (unsigned)(vals ? maps * 4 : 0);
    p->lds_bytes = p->off_flags + (codes ? maps : 0);
    return 0;
}

}  // namespace hz
