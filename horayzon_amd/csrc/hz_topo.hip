// hz_topo.hip -- the reductions over the azimuth axis of a horizon array (topo_param.pyx): sky view factor, visible sky
// fraction and topographic openness, any subset of the three from one read of `hori`.
#include "hz_internal.h"
#include "hz_q16.h"

namespace hz {

// ---------------------------------------------------------------------------------------
// reductions over the azimuth axis of a horizon array (topo_param.pyx):
//   HZ_TOPO_SVF   sky view factor        _sky_view_factor_cy        :412-460
//   HZ_TOPO_VSF   visible sky fraction   _visible_sky_fraction_cy   :499-543
//   HZ_TOPO_OPEN  topographic openness   _topographic_openness_cy   :577-603
//
// k_topo: one lane per cell for the arithmetic, one wave per 64 consecutive cells for the memory: the wave loads a
// [64 cells] x [32 azimuths] block of `hori` with 128 B contiguous per half wave into LDS (row stride 33 floats: the
// transposed reads are conflict free) and every lane then walks ITS cell's 32 values in azimuth order.  The float32
// accumulator with a float64 add per azimuth is the reference's (topo_param.pyx:446-458: the order of the additions is
// kept).  (Round 2 read `hori` with one lane per cell straight from HBM: 4 B loads at a stride of 4 A bytes, 1.7 - 3.4 x
// over-fetch and 31.5 ms per 3601^2 tile for an 18 GB read.)
//
// Trigonometry: the Cython code calls libm's float64 atan / cos / sin three times per (cell, azimuth) and adds the float64 term
// to a FLOAT32 accumulator (topo_param.pyx:446); all arguments lie in [-pi/2, pi/2].  Here ONE sine / cosine pair of the horizon
// angle gives cos^2, sin(2 h) / 2 = sin cos and -- through tan(h) >= x  <=>  sin >= x cos -- the comparison with the tilted plane's
// own horizon atan(x) without an arctangent; the arctangent is only evaluated where the plane limits.
// Round 6: the pair and the term are evaluated in FLOAT32 (fdlibm-style kernel polynomials on the halved argument + the
// double-angle formulas, |error| < 2e-7; every multiply and add rounds separately, -ffp-contract=off).  With the float64 pair of
// rounds 3 - 5 the kernel was bound by its float64 instructions (7.8e9 wave instructions at 4 cycles = 12.7 ms for 18.35 GB:
// 1.6 TB/s), not by memory.  What decides the result's accuracy is the float32 accumulator both sides share (half an ulp of a sum
// of ~100: 4e-6 per add before the division by azim_num), not the 1e-7 of a term: against a float64 evaluation of the same
// formulas the result is off by no more than the reference's own error E_ref plus 2.4e-7 (measured: E_ref + 1.2e-7 at most, over
// 2 ... 3456 azimuths, slopes up to 89.5 degrees, horizons -30 ... 85 degrees and +-pi/2: tests/test_gpu_topo_reference.py,
// DESIGN.md section 5; the older bar against the reference-made fixtures is 1e-5), and
// k_topo_wide keeps libm's float64 routines per azimuth as the Cython code has them.  Each lane prefetches its share of the next
// block into registers before it reduces the current one.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void hz_sincos_halfpi_f(float x, float &s, float &c) {
    // sin / cos for |x| <= pi/2 (+ a little): polynomials in z = y^2 on y = x / 2 (|y| <= pi/4: truncation < 2e-9), then
    // sin x = 2 sin y cos y, cos x = 1 - 2 sin^2 y
    const float y = 0.5f * x, z = y * y;
    float ps = 2.7557314e-06f;                                  //  1/9!
    ps = ps * z + -1.9841270e-04f;                              // -1/7!
    ps = ps * z + 8.3333338e-03f;                               //  1/5!
    ps = ps * z + -1.6666667e-01f;                              // -1/3!
    float pc = -2.7557314e-07f;                                 // -1/10!
    pc = pc * z + 2.4801587e-05f;                               //  1/8!
    pc = pc * z + -1.3888889e-03f;                              // -1/6!
    pc = pc * z + 4.1666668e-02f;                               //  1/4!
    const float sy = (y * z) * ps + y;
    const float cy = (z * z) * pc + (1.0f - 0.5f * z);
    s = (2.0f * sy) * cy;
    c = 1.0f - (2.0f * sy) * sy;
}

#define HZ_TOPO_CH 32      // azimuths per LDS block
#ifndef HZ_TOPO_WG
#define HZ_TOPO_WG 3      // workgroups per CU the register allocation is held to (3: 155 VGPRs; 4: see DESIGN.md section 5)
#endif
#ifndef HZ_TOPO_UNROLL
#define HZ_TOPO_UNROLL 2      // two terms in flight per lane (the float32 accumulation stays sequential): 15.7 -> 14.8 ms; 4: 16.5 (VGPRs)
#endif

// ---------------------------------------------------------------------------------------
// One kernel for any subset WANT of {HZ_TOPO_SVF, HZ_TOPO_VSF, HZ_TOPO_OPEN}, from ONE read of each block of `hori` (the
// horizon call's per-chunk launch, hz_topo_params and the three single-output entry points; all seven subsets are
// instantiated, a single output is k_topo<1|2|4>).  Each output has its own float32 accumulator and an operation sequence that
// does not depend on which other outputs are asked for: SVF and VSF share the sine / cosine pair of the horizon angle and the
// tilted-plane test, which either of them needs as they stand; openness adds the raw hv in float64.  So a map is the same
// words whatever it is computed together with (-ffp-contract=off: no multiply-add is formed in one instantiation and not in
// another).
// ---------------------------------------------------------------------------------------
#define HZ_TOPO_SVF 1
#define HZ_TOPO_VSF 2
#define HZ_TOPO_OPEN 4
template <int WANT>
__global__ __launch_bounds__(256, HZ_TOPO_WG) void k_topo(const float *__restrict__ azim, const float *__restrict__ hori,
                                             const float *__restrict__ vec_tilt, size_t ncell, int A,
                                             float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                             float *__restrict__ out_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    extern __shared__ float topo_lds[];                 // [2 A] sin / cos of the azimuths, then 4 x [64][33] blocks
    float *az_tab = topo_lds;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tile = topo_lds + 2 * A + wave * (64 * (HZ_TOPO_CH + 1));
    if (TILT) {                                         // float32 of the float64 value, topo_param.pyx:425-426
        for (int k = threadIdx.x; k < A; k += blockDim.x) {
            az_tab[k] = (float)sin((double)azim[k]);
            az_tab[A + k] = (float)cos((double)azim[k]);
        }
    }
    const size_t cell0 = ((size_t)blockIdx.x * 4 + wave) * 64;
    const size_t c = cell0 + lane;
    const bool have = c < ncell;
    float tx = 0.0f, ty = 0.0f, tz = 1.0f;
    if (TILT && have) { tx = vec_tilt[3 * c]; ty = vec_tilt[3 * c + 1]; tz = vec_tilt[3 * c + 2]; }
    // tangent of the tilted plane's own horizon: x = -sin(az) tx / tz - cos(az) ty / tz (:441-443); the two quotients
    // are formed once per cell (the Cython expression divides per azimuth: same value to a float rounding)
    const float qx = -tx / tz, qy = -ty / tz;
    const double half_pi = 3.14159265358979323846 / 2.0;
    const float half_pi_f = 1.57079632679489661923f;
    float agg_svf = 0.0f, agg_vsf = 0.0f, agg_open = 0.0f;
    const int half = lane >> 5, col = lane & 31;
    // this lane's share of a block: rows half, half + 2, ... of column `col` (128 B contiguous per half wave and row)
    const size_t n_rows = cell0 < ncell ? min((size_t)64, ncell - cell0) : 0;
    const float *src = hori + (cell0 + half) * (size_t)A + col;
    float pre[32];
    auto fetch = [&](int k0) {
        const int n = min(HZ_TOPO_CH, A - k0);
#pragma unroll
        for (int r = 0; r < 32; r++) {
            pre[r] = 0.0f;
            if (col < n && (size_t)(2 * r + half) < n_rows) pre[r] = src[(size_t)(2 * r) * A + k0];
        }
    };
    fetch(0);
    __syncthreads();                                    // az_tab is written
    // A wave's tile is private to it: LDS instructions of one wave execute in program order, so the transposed reads
    // below see the stores above without a workgroup barrier (the waves of a workgroup drift apart and overlap each
    // other's load and arithmetic phases); the fences only keep the compiler from reordering across them.
    for (int k0 = 0; k0 < A; k0 += HZ_TOPO_CH) {
        const int n = min(HZ_TOPO_CH, A - k0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 32; r++) tile[(2 * r + half) * (HZ_TOPO_CH + 1) + col] = pre[r];
        if (k0 + HZ_TOPO_CH < A) fetch(k0 + HZ_TOPO_CH);   // the next block's loads fly while this one is reduced
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!have) continue;
        const float *row = tile + lane * (HZ_TOPO_CH + 1);
#pragma unroll HZ_TOPO_UNROLL
        for (int kk = 0; kk < n; kk++) {
            const float hv = row[kk];
            if (WANT & HZ_TOPO_OPEN) agg_open = (float)(((double)agg_open + half_pi) - (double)hv);      // :599
            if (!TILT) continue;
            const float as = az_tab[k0 + kk], ac = az_tab[A + k0 + kk];
            const float xf = as * qx + ac * qy;
            float sn, cs;
            hz_sincos_halfpi_f(hv, sn, cs);
            float he = hv;
            // hv < atan(x)  <=>  sin < x cos: the tilted plane hides the horizon (:444 takes the larger angle)
            if (!(sn >= xf * cs)) {
                const float hp = atanf(xf);
                // sine and cosine of the plane's horizon come from its tangent: cos = 1 / sqrt(1 + x^2), sin = x cos
                if (!(hv >= hp)) {
                    he = hp;
                    // (xf * xf overflows for a plane that stands upright, tz == 0: rc is 0 and xf * rc would be inf * 0;
                    //  the reference takes the sine of atan(+-inf) = +-pi/2 there)
                    const float x2 = 1.0f + xf * xf;
                    const float rc = __builtin_amdgcn_rsqf(x2);
                    cs = rc; sn = (x2 == INFINITY) ? copysignf(1.0f, xf) : xf * rc;
                }
            }
            if (WANT & HZ_TOPO_SVF) agg_svf = agg_svf + ((tx * as + ty * ac) * ((half_pi_f - he) - sn * cs) + tz * (cs * cs));      // :446-452
            if (WANT & HZ_TOPO_VSF) agg_vsf = agg_vsf + (1.0f - sn);                  // 1 - cos(pi/2 - he), :540
        }
    }
    if (!have) return;
    if (WANT & HZ_TOPO_OPEN) out_open[c] = agg_open / (float)A;                       // :601
    if (TILT) {
        const float azim_spac = azim[1] - azim[0];
        if (WANT & HZ_TOPO_SVF) out_svf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_svf);
        if (WANT & HZ_TOPO_VSF) out_vsf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_vsf);
    }
}

// fallback for azimuth counts whose sine / cosine table does not fit in LDS (or hz_debug_set("topo_wide", 1)): one lane per
// cell, libm calls as the Cython code has them (the round-2 kernel).  As in k_topo, an output's operation sequence does not
// depend on the other outputs asked for.
template <int WANT>
__global__ __launch_bounds__(256) void k_topo_wide(const float *__restrict__ azim, const float *__restrict__ hori,
                                                  const float *__restrict__ vec_tilt, size_t ncell, int A,
                                                  float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                                  float *__restrict__ out_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    float tx = 0.0f, ty = 0.0f, tz = 1.0f;
    if (TILT) { tx = vec_tilt[3 * c]; ty = vec_tilt[3 * c + 1]; tz = vec_tilt[3 * c + 2]; }
    const float *h = hori + c * (size_t)A;
    float agg_svf = 0.0f, agg_vsf = 0.0f, agg_open = 0.0f;
    for (int k = 0; k < A; k++) {
        const float hv = h[k];
        if (WANT & HZ_TOPO_OPEN) agg_open = (float)(((double)agg_open + (3.14159265358979323846 / 2.0)) - (double)hv);
        if (!TILT) continue;
        const float as = (float)sin((double)azim[k]);
        const float ac = (float)cos((double)azim[k]);
        const float hori_plane = (float)atan((double)(-as * tx / tz - ac * ty / tz));
        const float he = (hv >= hori_plane) ? hv : hori_plane;
        if (WANT & HZ_TOPO_SVF) {
            const double ce = cos((double)he);
            agg_svf = (float)((double)agg_svf + ((double)(tx * as + ty * ac)
                              * ((3.14159265358979323846 / 2.0) - (double)he - (sin(2.0 * (double)he) / 2.0))
                              + (double)tz * (ce * ce)));
        }
        if (WANT & HZ_TOPO_VSF) agg_vsf = (float)((double)agg_vsf + (1.0 - cos((3.14159265358979323846 / 2.0) - (double)he)));
    }
    if (WANT & HZ_TOPO_OPEN) out_open[c] = agg_open / (float)A;
    if (TILT) {
        const float azim_spac = azim[1] - azim[0];
        if (WANT & HZ_TOPO_SVF) out_svf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_svf);
        if (WANT & HZ_TOPO_VSF) out_vsf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_vsf);
    }
}

// ---------------------------------------------------------------------------------------
// The reductions on the 16-bit horizon code (hz_q16.h; DESIGN.md section 4, clause 17) and on an azimuth-major horizon
// without the transposition back.  The contract: a code is decoded to float32 first (q16_decode, as hori_value(uint16_t)
// does) and the operation sequence of k_topo / k_topo_wide then runs on that float32, so a map reduced from codes q is,
// word for word, the map the float kernels reduce from decode(q); 0xFFFF decodes to NaN and behaves as a NaN horizon does.
//
// The float kernels above stay as they are (their machine code is what the headline numbers were measured on); the kernels
// below are written beside them and share the per-(cell, azimuth) step among themselves: topo_term() is k_topo's loop body,
// statement for statement (-ffp-contract=off: the same source operations are the same machine operations wherever they
// are inlined), and tests/test_gpu_topo_q16.py holds every instantiation to the float kernels bit for bit.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float topo_elem(float v) { return v; }
__device__ __forceinline__ float topo_elem(uint16_t q) { return q16_decode(q); }

template <int WANT>
__device__ __forceinline__ void topo_term(float hv, float as, float ac, float qx, float qy, float tx, float ty, float tz,
                                          float &agg_svf, float &agg_vsf, float &agg_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    const double half_pi = 3.14159265358979323846 / 2.0;
    const float half_pi_f = 1.57079632679489661923f;
    if (WANT & HZ_TOPO_OPEN) agg_open = (float)(((double)agg_open + half_pi) - (double)hv);      // :599
    if (!TILT) return;
    const float xf = as * qx + ac * qy;
    float sn, cs;
    hz_sincos_halfpi_f(hv, sn, cs);
    float he = hv;
    if (!(sn >= xf * cs)) {
        const float hp = atanf(xf);
        if (!(hv >= hp)) {
            he = hp;
            const float x2 = 1.0f + xf * xf;
            const float rc = __builtin_amdgcn_rsqf(x2);
            cs = rc; sn = (x2 == INFINITY) ? copysignf(1.0f, xf) : xf * rc;
        }
    }
    if (WANT & HZ_TOPO_SVF) agg_svf = agg_svf + ((tx * as + ty * ac) * ((half_pi_f - he) - sn * cs) + tz * (cs * cs));      // :446-452
    if (WANT & HZ_TOPO_VSF) agg_vsf = agg_vsf + (1.0f - sn);                  // 1 - cos(pi/2 - he), :540
}

// the division by azim_num and the sector weight, as k_topo ends
template <int WANT>
__device__ __forceinline__ void topo_store(const float *__restrict__ azim, size_t c, int A, float agg_svf, float agg_vsf,
                                           float agg_open, float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                           float *__restrict__ out_open) {
    if (WANT & HZ_TOPO_OPEN) out_open[c] = agg_open / (float)A;                       // :601
    if (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) {
        const float azim_spac = azim[1] - azim[0];
        if (WANT & HZ_TOPO_SVF) out_svf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_svf);
        if (WANT & HZ_TOPO_VSF) out_vsf[c] = (float)(((double)azim_spac / (2.0 * 3.14159265358979323846)) * (double)agg_vsf);
    }
}

// k_topo on cell-major codes: the same wave-private [64][33] float tile, the prefetch registers hold the raw codes and the
// decode sits where they are stored into the tile, so the arithmetic loop reads the float32 words k_topo reads.  A cell's
// row of codes starts at byte 2 c A -- at 2 mod 4 for every second cell of an odd A, or for a view at an odd element -- so
// the loads are plain 2-byte loads (64 B contiguous per half wave and row).
template <int WANT>
__global__ __launch_bounds__(256, HZ_TOPO_WG) void k_topo_q16(const float *__restrict__ azim, const uint16_t *__restrict__ hori,
                                                 const float *__restrict__ vec_tilt, size_t ncell, int A,
                                                 float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                                 float *__restrict__ out_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    extern __shared__ float topo_lds[];                 // [2 A] sin / cos of the azimuths, then 4 x [64][33] blocks
    float *az_tab = topo_lds;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tile = topo_lds + 2 * A + wave * (64 * (HZ_TOPO_CH + 1));
    if (TILT) {
        for (int k = threadIdx.x; k < A; k += blockDim.x) {
            az_tab[k] = (float)sin((double)azim[k]);
            az_tab[A + k] = (float)cos((double)azim[k]);
        }
    }
    const size_t cell0 = ((size_t)blockIdx.x * 4 + wave) * 64;
    const size_t c = cell0 + lane;
    const bool have = c < ncell;
    float tx = 0.0f, ty = 0.0f, tz = 1.0f;
    if (TILT && have) { tx = vec_tilt[3 * c]; ty = vec_tilt[3 * c + 1]; tz = vec_tilt[3 * c + 2]; }
    const float qx = -tx / tz, qy = -ty / tz;
    float agg_svf = 0.0f, agg_vsf = 0.0f, agg_open = 0.0f;
    const int half = lane >> 5, col = lane & 31;
    const size_t n_rows = cell0 < ncell ? min((size_t)64, ncell - cell0) : 0;
    const uint16_t *src = hori + (cell0 + half) * (size_t)A + col;
    uint16_t pre[32];
    auto fetch = [&](int k0) {
        const int n = min(HZ_TOPO_CH, A - k0);
#pragma unroll
        for (int r = 0; r < 32; r++) {
            pre[r] = 32767;                             // (decodes to +0.0f: k_topo's filler)
            if (col < n && (size_t)(2 * r + half) < n_rows) pre[r] = src[(size_t)(2 * r) * A + k0];
        }
    };
    fetch(0);
    __syncthreads();                                    // az_tab is written
    for (int k0 = 0; k0 < A; k0 += HZ_TOPO_CH) {
        const int n = min(HZ_TOPO_CH, A - k0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 32; r++) tile[(2 * r + half) * (HZ_TOPO_CH + 1) + col] = q16_decode(pre[r]);
        if (k0 + HZ_TOPO_CH < A) fetch(k0 + HZ_TOPO_CH);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (!have) continue;
        const float *row = tile + lane * (HZ_TOPO_CH + 1);
#pragma unroll HZ_TOPO_UNROLL
        for (int kk = 0; kk < n; kk++) {
            const float as = TILT ? az_tab[k0 + kk] : 0.0f, ac = TILT ? az_tab[A + k0 + kk] : 0.0f;
            topo_term<WANT>(row[kk], as, ac, qx, qy, tx, ty, tz, agg_svf, agg_vsf, agg_open);
        }
    }
    if (!have) return;
    topo_store<WANT>(azim, c, A, agg_svf, agg_vsf, agg_open, out_svf, out_vsf, out_open);
}

// The reductions straight from an azimuth-major horizon: planes[k * stride + c] is azimuth k of cell c, so the 64 lanes of a
// wave -- one lane per cell -- read 64 consecutive words (or codes) of one plane: coalesced as they lie, no LDS tile, no
// second pass.  HZ_TOPO_PF azimuths' loads are in flight per lane while the previous HZ_TOPO_PF are reduced.  The sine /
// cosine table sits in LDS as in k_topo and the step is topo_term(): the maps are k_topo's words.
#define HZ_TOPO_PF 8
template <int WANT, typename H>
__global__ __launch_bounds__(256) void k_topo_planes(const float *__restrict__ azim, const H *__restrict__ planes, size_t stride,
                                                    const float *__restrict__ vec_tilt, size_t ncell, int A,
                                                    float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                                    float *__restrict__ out_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    extern __shared__ float topo_lds[];                 // [2 A] sin / cos of the azimuths
    float *az_tab = topo_lds;
    if (TILT) {
        for (int k = threadIdx.x; k < A; k += blockDim.x) {
            az_tab[k] = (float)sin((double)azim[k]);
            az_tab[A + k] = (float)cos((double)azim[k]);
        }
    }
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = c < ncell;
    float tx = 0.0f, ty = 0.0f, tz = 1.0f;
    if (TILT && have) { tx = vec_tilt[3 * c]; ty = vec_tilt[3 * c + 1]; tz = vec_tilt[3 * c + 2]; }
    const float qx = -tx / tz, qy = -ty / tz;
    float agg_svf = 0.0f, agg_vsf = 0.0f, agg_open = 0.0f;
    const H *src = planes + (have ? c : 0);
    H cur[HZ_TOPO_PF], nxt[HZ_TOPO_PF];
    auto fetch = [&](H (&dst)[HZ_TOPO_PF], int k0) {
#pragma unroll
        for (int j = 0; j < HZ_TOPO_PF; j++) {
            dst[j] = H(0);
            if (have && k0 + j < A) dst[j] = src[(size_t)(k0 + j) * stride];
        }
    };
    fetch(cur, 0);
    __syncthreads();                                    // az_tab is written
    if (!have) return;
    for (int k0 = 0; k0 < A; k0 += HZ_TOPO_PF) {
        if (k0 + HZ_TOPO_PF < A) fetch(nxt, k0 + HZ_TOPO_PF);
#pragma unroll
        for (int j = 0; j < HZ_TOPO_PF; j++) {
            if (k0 + j < A) {
                const float as = TILT ? az_tab[k0 + j] : 0.0f, ac = TILT ? az_tab[A + k0 + j] : 0.0f;
                topo_term<WANT>(topo_elem(cur[j]), as, ac, qx, qy, tx, ty, tz, agg_svf, agg_vsf, agg_open);
            }
        }
#pragma unroll
        for (int j = 0; j < HZ_TOPO_PF; j++) cur[j] = nxt[j];
    }
    topo_store<WANT>(azim, c, A, agg_svf, agg_vsf, agg_open, out_svf, out_vsf, out_open);
}

// k_topo_wide for either element type and either layout: element (c, k) is hori[c * cell_stride + k * azim_stride] --
// (A, 1) cell-major, (1, stride) on planes.  The operation sequence is k_topo_wide's on topo_elem() of the element.
template <int WANT, typename H>
__global__ __launch_bounds__(256) void k_topo_wide_strided(const float *__restrict__ azim, const H *__restrict__ hori,
                                                          size_t cell_stride, size_t azim_stride,
                                                          const float *__restrict__ vec_tilt, size_t ncell, int A,
                                                          float *__restrict__ out_svf, float *__restrict__ out_vsf,
                                                          float *__restrict__ out_open) {
    constexpr bool TILT = (WANT & (HZ_TOPO_SVF | HZ_TOPO_VSF)) != 0;
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    float tx = 0.0f, ty = 0.0f, tz = 1.0f;
    if (TILT) { tx = vec_tilt[3 * c]; ty = vec_tilt[3 * c + 1]; tz = vec_tilt[3 * c + 2]; }
    const H *h = hori + c * cell_stride;
    float agg_svf = 0.0f, agg_vsf = 0.0f, agg_open = 0.0f;
    for (int k = 0; k < A; k++) {
        const float hv = topo_elem(h[(size_t)k * azim_stride]);
        if (WANT & HZ_TOPO_OPEN) agg_open = (float)(((double)agg_open + (3.14159265358979323846 / 2.0)) - (double)hv);
        if (!TILT) continue;
        const float as = (float)sin((double)azim[k]);
        const float ac = (float)cos((double)azim[k]);
        const float hori_plane = (float)atan((double)(-as * tx / tz - ac * ty / tz));
        const float he = (hv >= hori_plane) ? hv : hori_plane;
        if (WANT & HZ_TOPO_SVF) {
            const double ce = cos((double)he);
            agg_svf = (float)((double)agg_svf + ((double)(tx * as + ty * ac)
                              * ((3.14159265358979323846 / 2.0) - (double)he - (sin(2.0 * (double)he) / 2.0))
                              + (double)tz * (ce * ce)));
        }
        if (WANT & HZ_TOPO_VSF) agg_vsf = (float)((double)agg_vsf + (1.0 - cos((3.14159265358979323846 / 2.0) - (double)he)));
    }
    topo_store<WANT>(azim, c, A, agg_svf, agg_vsf, agg_open, out_svf, out_vsf, out_open);
}

using TopoKernel = void (*)(const float *, const float *, const float *, size_t, int, float *, float *, float *);
static const TopoKernel topo_tiled[8] = {nullptr, k_topo<1>, k_topo<2>, k_topo<3>, k_topo<4>, k_topo<5>, k_topo<6>, k_topo<7>};
static const TopoKernel topo_wide[8] = {nullptr, k_topo_wide<1>, k_topo_wide<2>, k_topo_wide<3>, k_topo_wide<4>,
                                        k_topo_wide<5>, k_topo_wide<6>, k_topo_wide<7>};

int topo_launch(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                float *svf, float *vsf, float *openness, hipStream_t st) {
    const int want = (svf ? HZ_TOPO_SVF : 0) | (vsf ? HZ_TOPO_VSF : 0) | (openness ? HZ_TOPO_OPEN : 0);
    if (want == 0) return set_error(HZ_ERR_ARG, "no reduction requested");
    const size_t ncell = (size_t)len_0 * len_1;
    if (ncell == 0) return HZ_OK;
    const size_t lds = (2 * (size_t)len_2 + 4 * 64 * (HZ_TOPO_CH + 1)) * sizeof(float);
    // (hz_debug_set("topo_wide", 1) forces the fallback kernel -- tests compare the two paths on the same input, so that they
    //  cannot drift apart: k_topo takes the float32 arctangent only where the tilted plane limits, k_topo_wide calls libm's
    //  float64 routines per azimuth as the Cython code does; both are held to 1e-5 against the reference-made fixtures)
    const bool tiled = lds <= 60 * 1024 && g_topo_wide.load(std::memory_order_relaxed) == 0;
    const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
    const TopoKernel kernel = tiled ? topo_tiled[want] : topo_wide[want];
    hipLaunchKernelGGL(kernel, grid, block, tiled ? lds : 0, st, azim, hori, vec_tilt, ncell, len_2, svf, vsf, openness);
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

// ---- the launches of the kernels on codes and on planes ----------------------------------------
using TopoQ16Kernel = void (*)(const float *, const uint16_t *, const float *, size_t, int, float *, float *, float *);
template <typename H>
using TopoPlanesKernel = void (*)(const float *, const H *, size_t, const float *, size_t, int, float *, float *, float *);
template <typename H>
using TopoStridedKernel = void (*)(const float *, const H *, size_t, size_t, const float *, size_t, int, float *, float *, float *);

static const TopoQ16Kernel topo_tiled_q16[8] = {nullptr, k_topo_q16<1>, k_topo_q16<2>, k_topo_q16<3>, k_topo_q16<4>,
                                                k_topo_q16<5>, k_topo_q16<6>, k_topo_q16<7>};
template <typename H>
static TopoPlanesKernel<H> topo_planes_kernel(int want) {
    static const TopoPlanesKernel<H> table[8] = {nullptr, k_topo_planes<1, H>, k_topo_planes<2, H>, k_topo_planes<3, H>,
                                                 k_topo_planes<4, H>, k_topo_planes<5, H>, k_topo_planes<6, H>, k_topo_planes<7, H>};
    return table[want];
}
template <typename H>
static TopoStridedKernel<H> topo_strided_kernel(int want) {
    static const TopoStridedKernel<H> table[8] = {nullptr, k_topo_wide_strided<1, H>, k_topo_wide_strided<2, H>,
                                                  k_topo_wide_strided<3, H>, k_topo_wide_strided<4, H>, k_topo_wide_strided<5, H>,
                                                  k_topo_wide_strided<6, H>, k_topo_wide_strided<7, H>};
    return table[want];
}

// One rule for every route (topo_launch's): the tiled and the direct form while the sine / cosine table and k_topo's tiles
// fit the LDS and "topo_wide" is off, the one-lane-per-cell libm form otherwise -- so a layout or an element type never
// changes which form, and with it which error bar, an azimuth count gets.
static bool topo_use_tiled(int A) {
    const size_t lds = (2 * (size_t)A + 4 * 64 * (HZ_TOPO_CH + 1)) * sizeof(float);
    return lds <= 60 * 1024 && g_topo_wide.load(std::memory_order_relaxed) == 0;
}

int topo_launch_q16(const float *azim, const uint16_t *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                    float *svf, float *vsf, float *openness, hipStream_t st) {
    const int want = (svf ? HZ_TOPO_SVF : 0) | (vsf ? HZ_TOPO_VSF : 0) | (openness ? HZ_TOPO_OPEN : 0);
    if (want == 0) return set_error(HZ_ERR_ARG, "no reduction requested");
    const size_t ncell = (size_t)len_0 * len_1;
    if (ncell == 0) return HZ_OK;
    const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
    if (topo_use_tiled(len_2)) {
        const size_t lds = (2 * (size_t)len_2 + 4 * 64 * (HZ_TOPO_CH + 1)) * sizeof(float);
        hipLaunchKernelGGL(topo_tiled_q16[want], grid, block, lds, st, azim, hori, vec_tilt, ncell, len_2, svf, vsf, openness);
    } else {
        hipLaunchKernelGGL(topo_strided_kernel<uint16_t>(want), grid, block, 0, st, azim, hori, (size_t)len_2, (size_t)1, vec_tilt,
                           ncell, len_2, svf, vsf, openness);
    }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

template <typename H>
static int topo_launch_planes_of(const float *azim, const H *planes, size_t stride, const float *vec_tilt, size_t ncell, int A,
                                 int want, float *svf, float *vsf, float *openness, hipStream_t st) {
    const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
    if (topo_use_tiled(A)) {
        hipLaunchKernelGGL(topo_planes_kernel<H>(want), grid, block, 2 * (size_t)A * sizeof(float), st, azim, planes, stride, vec_tilt,
                           ncell, A, svf, vsf, openness);
    } else {
        hipLaunchKernelGGL(topo_strided_kernel<H>(want), grid, block, 0, st, azim, planes, (size_t)1, stride, vec_tilt, ncell, A,
                           svf, vsf, openness);
    }
    HZ_HIP(hipGetLastError());
    return HZ_OK;
}

// `planes` points at azimuth 0 of the first of `ncell` cells, azimuth k of a cell lies k * stride elements on; vec_tilt and the
// maps point at that first cell too.  q16: the elements are codes, else float32.
int topo_launch_planes_direct(const float *azim, const void *planes, bool q16, size_t stride, const float *vec_tilt, size_t ncell,
                              int A, float *svf, float *vsf, float *openness, hipStream_t st) {
    const int want = (svf ? HZ_TOPO_SVF : 0) | (vsf ? HZ_TOPO_VSF : 0) | (openness ? HZ_TOPO_OPEN : 0);
    if (want == 0) return set_error(HZ_ERR_ARG, "no reduction requested");
    if (ncell == 0) return HZ_OK;
    return q16 ? topo_launch_planes_of(azim, static_cast<const uint16_t *>(planes), stride, vec_tilt, ncell, A, want, svf, vsf, openness, st)
               : topo_launch_planes_of(azim, static_cast<const float *>(planes), stride, vec_tilt, ncell, A, want, svf, vsf, openness, st);
}

}  // namespace hz
