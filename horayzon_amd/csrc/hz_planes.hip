// hz_planes.hip -- the azimuth-major horizon layout planes[azim][y][x] (clause 11): the two
// transpositions between it and the cell-major hori[y][x][azim] that k_horizon writes, and the look-up kernel of
// HorizonTerrain that reads planes.
//
// The cell-major horizon is a `cells` x A matrix with the cells contiguous, so both directions are a 2-D transpose
// through an LDS tile of 64 cells x 32 azimuths.  Data moves as 32-bit words: no float arithmetic touches it, NaN
// payloads and hori_fill arrive as they left.  On the cell-major side a half-wave reads or writes the 32 azimuths of
// one cell (128 contiguous bytes), on the plane side a wave reads or writes 64 cells of one plane (256 contiguous
// bytes).  The tile's rows are padded by one word (as k_topo's): the 32 lanes of a half-wave that walk down a column
// hit banks (a * 65 + cell) mod 32 = (a + cell) mod 32, all different; the row accesses are consecutive words.
//
// k_horisun_planes is k_horisun (hz_horisun.hip) with row[k] read as planes[k * stride + c].  The sun's azimuth is
// nearly the same in every cell's frame, so the lanes of a wave ask for the same one or two planes and their loads are
// 64 consecutive words instead of 64 lines.  The arithmetic is written again here in the same order of operations
// (that file's text does not move); both files are built with -ffp-contract=off, so the results are the same words.  Like
// k_horisun it takes the horizon's element type as a template parameter: float, or the 16-bit codes of clause 15 (hz_q16.h).
#include "hz_internal.h"
#include "hz_horisun_plan.h"
#include "hz_horisun_refrac.h"
#include "hz_q16.h"

namespace hz {

#define HZ_PLANES_TC 64                  // cells of a tile
#define HZ_PLANES_TA 32                  // azimuths of a tile
#define HZ_PLANES_TPB 256
#define HZ_PLANES_MAX_BLOCKS 16384u      // the blocks walk the tiles in a grid-stride loop: any shape fits a launch

struct PlanesArgs {
    const uint32_t *src;
    uint32_t *dst;
    size_t cells, plane_stride, cell0;   // plane side: cell c is element k * plane_stride + cell0 + c
    size_t tiles_c, tiles;               // tiles along the cells, tiles in all (tiles_c * tiles_a)
    int azim_num, tiles_a;
};

// TO_PLANES: src = hori[cells][A], dst = planes; else src = planes, dst = hori[cells][A]
template <bool TO_PLANES>
__device__ __forceinline__ void planes_transpose_body(const PlanesArgs &p, uint32_t (*tile)[HZ_PLANES_TC + 1]) {
    const int t = threadIdx.x;
    const int ra = t % HZ_PLANES_TA, rc = t / HZ_PLANES_TA;      // cell-major side: azimuth fastest, 8 cells per pass
    const int pc = t % HZ_PLANES_TC, pa = t / HZ_PLANES_TC;      // plane side: cell fastest, 4 azimuths per pass
    const size_t A = (size_t)p.azim_num;
    for (size_t tl = blockIdx.x; tl < p.tiles; tl += gridDim.x) {
        // consecutive tiles share their cells and go along the azimuths: a cell's row is read or written end to end
        const size_t cb = (tl / (size_t)p.tiles_a) * HZ_PLANES_TC;
        const int ab = (int)(tl % (size_t)p.tiles_a) * HZ_PLANES_TA;
        if (TO_PLANES) {
            for (int i = rc; i < HZ_PLANES_TC; i += HZ_PLANES_TPB / HZ_PLANES_TA) {
                const size_t c = cb + (size_t)i;
                if (c < p.cells && ab + ra < p.azim_num) tile[ra][i] = p.src[c * A + (size_t)(ab + ra)];
            }
        } else {
            for (int k = pa; k < HZ_PLANES_TA; k += HZ_PLANES_TPB / HZ_PLANES_TC) {
                const size_t c = cb + (size_t)pc;
                if (c < p.cells && ab + k < p.azim_num) tile[k][pc] = p.src[(size_t)(ab + k) * p.plane_stride + p.cell0 + c];
            }
        }
        __syncthreads();
        if (TO_PLANES) {
            for (int k = pa; k < HZ_PLANES_TA; k += HZ_PLANES_TPB / HZ_PLANES_TC) {
                const size_t c = cb + (size_t)pc;
                if (c < p.cells && ab + k < p.azim_num) p.dst[(size_t)(ab + k) * p.plane_stride + p.cell0 + c] = tile[k][pc];
            }
        } else {
            for (int i = rc; i < HZ_PLANES_TC; i += HZ_PLANES_TPB / HZ_PLANES_TA) {
                const size_t c = cb + (size_t)i;
                if (c < p.cells && ab + ra < p.azim_num) p.dst[c * A + (size_t)(ab + ra)] = tile[ra][i];
            }
        }
        __syncthreads();                 // the tile is filled again in the next pass
    }
}

__global__ __launch_bounds__(HZ_PLANES_TPB) void k_hori_to_planes(PlanesArgs p) {
    __shared__ uint32_t tile[HZ_PLANES_TA][HZ_PLANES_TC + 1];
    planes_transpose_body<true>(p, tile);
}

__global__ __launch_bounds__(HZ_PLANES_TPB) void k_planes_to_hori(PlanesArgs p) {
    __shared__ uint32_t tile[HZ_PLANES_TA][HZ_PLANES_TC + 1];
    planes_transpose_body<false>(p, tile);
}

template <bool TO_PLANES>
static int planes_transpose(const float *src, float *dst, size_t cells, int azim_num, size_t plane_stride, size_t cell0,
                            hipStream_t st) {
    if (cells == 0 || azim_num <= 0) return HZ_OK;
    PlanesArgs p;
    p.src = reinterpret_cast<const uint32_t *>(src); p.dst = reinterpret_cast<uint32_t *>(dst);
    p.cells = cells; p.plane_stride = plane_stride; p.cell0 = cell0;
    p.azim_num = azim_num;
    p.tiles_a = (azim_num + HZ_PLANES_TA - 1) / HZ_PLANES_TA;
    p.tiles_c = (cells + HZ_PLANES_TC - 1) / HZ_PLANES_TC;
    p.tiles = p.tiles_c * (size_t)p.tiles_a;
    const unsigned blocks = (unsigned)std::min<size_t>(p.tiles, HZ_PLANES_MAX_BLOCKS);
    if (TO_PLANES) hipLaunchKernelGGL(k_hori_to_planes, dim3(blocks), dim3(HZ_PLANES_TPB), 0, st, p);
    else hipLaunchKernelGGL(k_planes_to_hori, dim3(blocks), dim3(HZ_PLANES_TPB), 0, st, p);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

int hori_to_planes_launch(const float *hori, size_t cells, int azim_num, float *planes, size_t plane_stride, size_t cell0,
                          hipStream_t st) {
    return planes_transpose<true>(hori, planes, cells, azim_num, plane_stride, cell0, st);
}

int planes_to_hori_launch(const float *planes, size_t plane_stride, size_t cell0, size_t cells, int azim_num, float *hori,
                          hipStream_t st) {
    return planes_transpose<false>(planes, hori, cells, azim_num, plane_stride, cell0, st);
}

// ---- k_horisun_planes: k_horisun of hz_horisun.hip, the horizon read from planes ----------------------------------

struct HorisunPlanesArgs {
    HorisunArgs a;                       // a.hori = planes f32[azim_num][stride]
    size_t stride;
};

// shadow_comp.cpp:96-106, as horisun_unit of hz_horisun.hip
__device__ __forceinline__ void planes_unit(float &x, float &y, float &z) {
    const float mag = __builtin_sqrtf((x * x + y * y) + z * z);
    x = x / mag; y = y / mag; z = z / mag;
}

// horisun_shaded of hz_horisun.hip: `col` = planes + c, the cell's horizon at azimuth k is col[k * stride]
template <typename H>
__device__ __forceinline__ bool planes_shaded(const H *__restrict__ col, size_t stride, int azim_num, double per_rad,
                                              float sx, float sy, float sz, float nx, float ny, float nz,
                                              float hx, float hy, float hz_, double ex, double ey, double ez) {
    const double cn = ((double)sx * (double)hx + (double)sy * (double)hy) + (double)sz * (double)hz_;
    const double ce = ((double)sx * ex + (double)sy * ey) + (double)sz * ez;
    const double cu = ((double)sx * (double)nx + (double)sy * (double)ny) + (double)sz * (double)nz;
    double phi = atan2(ce, cn);
    if (phi < 0.0) phi += 6.283185307179586;
    const double u = phi * per_rad;
    // u is in [0, A] for finite inputs; the clamp keeps the two loads inside the planes whatever the inputs are (NaN: 0)
    const double kf = fmin(fmax(floor(u), 0.0), (double)azim_num);
    const double t = u - kf;
    const int k = (int)kf;
    const int k0 = k % azim_num, k1 = (k + 1) % azim_num;
    const double h = (1.0 - t) * hori_value(col[(size_t)k0 * stride]) + t * hori_value(col[(size_t)k1 * stride]);
    const double alpha = asin(fmin(fmax(cu, -1.0), 1.0));
    return alpha < h;                                   // NaN horizon: false, the cell counts as lit
}

// REFRAC, H: as k_horisun's
template <bool REFRAC, typename H>
__global__ __launch_bounds__(HZ_HORISUN_TPB) void k_horisun_planes(HorisunPlanesArgs q) {
    const HorisunArgs &p = q.a;
    const size_t c = (size_t)blockIdx.x * HZ_HORISUN_TPB + threadIdx.x;
    if (c >= p.cells) return;
    const size_t n = p.cells;
    const bool want_code = p.out_u8 != nullptr || p.sum_lit != nullptr;     // the same in every lane
    if (p.mask[c] != 1) {
        for (int s = 0; s < p.num_sun; s++) {
            if (p.out_u8) p.out_u8[(size_t)s * n + c] = 3;
            if (p.out_f32) p.out_f32[(size_t)s * n + c] = p.fill;
        }
        if (p.last) {
            if (p.sum_sw) p.sum_sw[c] = p.fill;
            if (p.sum_lit) p.sum_lit[c] = p.fill;
        }
        return;
    }
    const float tilt_x = p.vec_tilt[3 * c], tilt_y = p.vec_tilt[3 * c + 1], tilt_z = p.vec_tilt[3 * c + 2];
    const float norm_x = p.vec_norm[3 * c], norm_y = p.vec_norm[3 * c + 1], norm_z = p.vec_norm[3 * c + 2];
    const float north_x = p.vec_north[3 * c], north_y = p.vec_north[3 * c + 1], north_z = p.vec_north[3 * c + 2];
    const float enl = p.surf_enl_fac[c];
    const float ray_org_elev = 0.05f;                              // shadow_comp.cpp:388, :497
    const float ox = p.vert[3 * c] + norm_x * ray_org_elev;
    const float oy = p.vert[3 * c + 1] + norm_y * ray_org_elev;
    const float oz = p.vert[3 * c + 2] + norm_z * ray_org_elev;
    // east = north x norm: products of two floats are exact in float64, each difference is rounded once
    const double ex = (double)north_y * (double)norm_z - (double)north_z * (double)norm_y;
    const double ey = (double)north_z * (double)norm_x - (double)north_x * (double)norm_z;
    const double ez = (double)north_x * (double)norm_y - (double)north_y * (double)norm_x;
    const double per_rad = (double)p.azim_num / 6.283185307179586;
    const H *col = reinterpret_cast<const H *>(p.hori) + c;
    double a_sw = (p.sum_sw && !p.first) ? p.acc_sw[c] : 0.0;
    double a_lit = (p.sum_lit && !p.first) ? p.acc_lit[c] : 0.0;
    double fac = 0.0;
    if (REFRAC) fac = p.refrac_fac[c];
    for (int s = 0; s < p.num_sun; s++) {
        float sun_x = p.suns[3 * s] - ox, sun_y = p.suns[3 * s + 1] - oy, sun_z = p.suns[3 * s + 2] - oz;   // :422-425
        planes_unit(sun_x, sun_y, sun_z);
        float dot_prod_ns = (norm_x * sun_x + norm_y * sun_y) + norm_z * sun_z;
        if (REFRAC) horisun_refract(fac, tilt_x, tilt_y, tilt_z, norm_x, norm_y, norm_z, sun_x, sun_y, sun_z, dot_prod_ns);
        const float dot_prod_ts = (tilt_x * sun_x + tilt_y * sun_y) + tilt_z * sun_z;
        int code = 1;                                   // self-shaded (shadow: !(dot_ts > 0))
        float val = 0.0f;                               // sw_dir_cor: 0 outside ang_max (!(dot_ts > dot_prod_min)) and in shadow
        // the look-up decides the code of every cell with dot_ts > 0, and the value of those with dot_ts > dot_prod_min (> 0)
        if (dot_prod_ts > (want_code ? 0.0f : p.dot_prod_min)) {
            const bool shaded = planes_shaded(col, q.stride, p.azim_num, per_rad, sun_x, sun_y, sun_z, norm_x, norm_y, norm_z,
                                              north_x, north_y, north_z, ex, ey, ez);
            code = shaded ? 2 : 0;
            if (!shaded && dot_prod_ts > p.dot_prod_min) {         // shadow_result
                float d = dot_prod_ns;
                if (d < p.dot_prod_min) d = p.dot_prod_min;
                val = (dot_prod_ts / d) * enl;
            }
        }
        if (p.out_u8) p.out_u8[(size_t)s * n + c] = (uint8_t)code;
        if (p.out_f32) p.out_f32[(size_t)s * n + c] = val;
        // clause 9: acc += (double)w * (double)value, ascending s
        const double w = p.weights ? (double)p.weights[s] : 1.0;
        if (p.sum_sw) a_sw += w * (double)val;
        if (p.sum_lit) a_lit += w * (code == 0 ? 1.0 : 0.0);
    }
    if (p.last) {                                       // one rounding
        if (p.sum_sw) p.sum_sw[c] = (float)a_sw;
        if (p.sum_lit) p.sum_lit[c] = (float)a_lit;
    } else {
        if (p.sum_sw) p.acc_sw[c] = a_sw;
        if (p.sum_lit) p.acc_lit[c] = a_lit;
    }
}

int horisun_planes_launch(const HorisunArgs &a, size_t plane_stride, unsigned blocks, hipStream_t st, bool q16) {
    if (a.cells == 0 || a.num_sun <= 0 || blocks == 0) return HZ_OK;
    HorisunPlanesArgs q;
    q.a = a; q.stride = plane_stride;
    const dim3 grid(blocks), block(HZ_HORISUN_TPB);
    if (q16) {
        if (a.refrac_fac) hipLaunchKernelGGL((k_horisun_planes<true, uint16_t>), grid, block, 0, st, q);
        else hipLaunchKernelGGL((k_horisun_planes<false, uint16_t>), grid, block, 0, st, q);
    } else {
        if (a.refrac_fac) hipLaunchKernelGGL((k_horisun_planes<true, float>), grid, block, 0, st, q);
        else hipLaunchKernelGGL((k_horisun_planes<false, float>), grid, block, 0, st, q);
    }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
