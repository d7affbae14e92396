// hz_search.h -- the reference's per-cell horizon search algorithms as a resumable per-lane
// state machine (ray_discrete_sampling / ray_binary_search / ray_guess_const,
// horizon_comp.cpp:302-498, and the *_hori_dist variants :519-612).  Shared by the gridded
// and the locations kernels.  The float/double promotion pattern of the reference's index
// arithmetic is reproduced exactly; tables are built on the host (hz_api_horizon.hip) and only read here.
#pragma once
#include "hz_internal.h"

namespace hz {

enum { ALG_DISCRETE = 0, ALG_BINARY = 1, ALG_GUESS = 2 };
enum { PH_NEWAZ = 0, PH_BIN = 1, PH_UP = 2, PH_DOWN = 3, PH_EMIT = 4 };

struct Tables {
    const float *azim_sin, *azim_cos, *elev_ang, *elev_sin, *elev_cos;
    const int *mid_idx;   // pairs: mid_idx[2 i] = ind_of(half_sum(elev_ang[i], elev_ang[i + 10])), [2 i + 1] = bits of elev_ang[that], built on the host
    int azim_num, elev_num;
    float hori_acc, low, up;
    double step;   // (double)hori_acc / 5.0
};

struct Search {
    int k, phase, ind, prev, pazim, count;
    float lim_up, lim_low, elev_samp;
    float ev;   // value to emit for azimuth k (phase PH_EMIT): one emit site keeps the code small
};

// (int)roundf((elev_samp - low) / (hori_acc / 5.0)), horizon_comp.cpp:351-352
__device__ __forceinline__ int ind_of(const Tables &t, float elev_samp) {
    return (int)__builtin_roundf((float)((double)(elev_samp - t.low) / t.step));
}
// (a + b) / 2.0 -> float, horizon_comp.cpp:350, :330, :462, :490
__device__ __forceinline__ float half_sum(float a, float b) {
    return (float)((double)(a + b) / 2.0);
}

// index of the table entry nearest to the midpoint of entries `a` and `b` (horizon_comp.cpp:462-464,
// :490-492).  The search steps by 10 entries, so the midpoint index comes from a host-built table
// (same float/double expressions, hz_api_horizon.hip); clamped steps at the table ends take the general path.
// *ev = elev_ang[that index], the value the search emits: the table holds (index, value bits) pairs -- one 8 B load.
__device__ __forceinline__ int mid_index(const Tables &t, int a, int b, float *ev) {
    const int lo = min(a, b);
    if (max(a, b) - lo == 10) {
        const int2 v = reinterpret_cast<const int2 *>(t.mid_idx)[lo];
        *ev = __int_as_float(v.y);
        return v.x;
    }
    const int ind = ind_of(t, half_sum(t.elev_ang[a], t.elev_ang[b]));
    *ev = t.elev_ang[ind];
    return ind;
}

// per-cell output sink
struct Sink {
    float *hori;         // &hori_buffer[cell * azim_num]
    float *dist;         // &hori_dist_buffer[cell * azim_num] or null
    float dist_hit;      // distance of the last hit ray; persists across azimuths (horizon_comp.cpp:526-527)
    float *stage;        // LDS staging of 4 consecutive azimuths of this lane (stage[j * stride]) or null
    int stride;
};

// A lane produces its azimuths one at a time; a 4 B store per lane at stride 4*A bytes costs a
// 32 B memory sector each (8x write amplification measured).  With STAGE, four consecutive
// values of a lane are collected in LDS and leave as one 16 B store (requires azim_num % 4 == 0
// and a 16 B aligned buffer; checked by the launcher).
template <bool STAGE>
__device__ __forceinline__ void emit(Sink &s, const Tables &, int k, float h) {
    if (STAGE) {
        if ((k & 3) == 3) {
            const float4 v = make_float4(s.stage[0], s.stage[s.stride], s.stage[2 * s.stride], h);
            *reinterpret_cast<float4 *>(s.hori + (k - 3)) = v;
        } else {
            s.stage[(k & 3) * s.stride] = h;
        }
    } else {
        s.hori[k] = h;
    }
    if (s.dist) s.dist[k] = s.dist_hit;   // :552, :608
}

// Consume the result of the previous ray (if any) and produce the next sample.
// Returns true with s.ind / s.k identifying the next ray, false when the cell is finished.
template <int ALG, bool STAGE>
__device__ __forceinline__ bool advance(Search &s, bool hit, const Tables &t, Sink &out,
                                        unsigned &guards) {
    const int top = t.elev_num - 1;
    for (;;) {
        if (s.phase == PH_EMIT) {                              // the only place that writes output
            emit<STAGE>(out, t, s.k, s.ev);
            s.k++; s.phase = PH_NEWAZ;
        }
        if (s.phase == PH_NEWAZ) {
            if (s.k >= t.azim_num) return false;
            const bool binary = (ALG == ALG_BINARY) || (ALG == ALG_GUESS && s.k == 0);
            if (binary) {                                   // horizon_comp.cpp:348-354 / :398-404
                s.lim_up = t.up; s.lim_low = t.low;
                s.elev_samp = half_sum(s.lim_up, s.lim_low);
                s.ind = ind_of(t, s.elev_samp);
                s.phase = PH_BIN;
                const float e = t.elev_ang[s.ind];
                if (__builtin_fmaxf(s.lim_up - e, e - s.lim_low) > t.hori_acc) return true;
                s.ev = s.elev_samp; s.pazim = s.ind; s.phase = PH_EMIT;
                continue;
            }
            // move upwards: horizon_comp.cpp:311-317 (discrete, from index 0) / :439-446
            s.ind = (ALG == ALG_DISCRETE) ? 0 : max(s.pazim - 5, 0);
            s.prev = s.ind;
            s.ind = min(s.ind + 10, top);
            s.count = 1;
            s.phase = PH_UP;
            return true;
        }
        if (s.phase == PH_BIN) {                             // :367-374 / :417-424
            const float e0 = t.elev_ang[s.ind];
            if (hit) s.lim_low = e0; else s.lim_up = e0;
            s.elev_samp = half_sum(s.lim_up, s.lim_low);
            s.ind = ind_of(t, s.elev_samp);
            const float e = t.elev_ang[s.ind];
            if (__builtin_fmaxf(s.lim_up - e, e - s.lim_low) > t.hori_acc) return true;
            s.ev = s.elev_samp; s.pazim = s.ind; s.phase = PH_EMIT;   // :376 / :428
            continue;
        }
        if (s.phase == PH_UP) {
            const bool guard = hit && (s.ind == top);        // the reference never leaves this loop
            if (hit && !guard) {
                s.prev = s.ind;
                s.ind = min(s.ind + 10, top);
                s.count++;
                return true;
            }
            if (guard) guards++;
            if (ALG == ALG_DISCRETE) {                       // :330
                s.ev = half_sum(t.elev_ang[s.prev], t.elev_ang[s.ind]); s.phase = PH_EMIT;
                s.pazim = s.prev;                            // last blocked sample (hit-cache hint only)
                continue;
            }
            if (s.count > 1) {                               // :460-467
                s.ind = mid_index(t, s.prev, s.ind, &s.ev);
                s.pazim = s.ind; s.phase = PH_EMIT;
                continue;
            }
            // move downwards: :472-477
            s.ind = min(s.pazim + 5, top);
            s.prev = s.ind;
            s.ind = max(s.ind - 10, 0);
            s.phase = PH_DOWN;
            return true;
        }
        // PH_DOWN: :474-488
        {
            const bool guard = (!hit) && (s.ind == 0);
            if (!hit && !guard) {
                s.prev = s.ind;
                s.ind = max(s.ind - 10, 0);
                return true;
            }
            if (guard) guards++;
            s.ind = mid_index(t, s.prev, s.ind, &s.ev);                       // :490-494
            s.pazim = s.ind; s.phase = PH_EMIT;
            continue;
        }
    }
}

// The search state of the flat guess_constant refill (k_horizon<..., FLAT>): Search without the four floats that only the binary
// search of azimuth 0 reads.  The two that persist from one ray to the next there, lim_up and lim_low, live in two LDS words of
// the lane (lim[0], lim[lim_stride]: the two rows below the fast stack, k_horizon) while the lane is in PH_BIN; elev_samp and ev
// never outlive the call that sets them.  Every other field means what it means in Search.
struct SearchLean {
    int k, phase, ind, prev, pazim, count;
};

// The transitions of advance<ALG_GUESS, STAGE> out of PH_NEWAZ and PH_BIN on a SearchLean: azimuth 0's binary search
// (horizon_comp.cpp:398-428) up to the first sample of azimuth 1 (:439-446).  Same states, same emitted values.
template <bool STAGE>
__device__ __forceinline__ bool advance_az0_lean(SearchLean &s, bool hit, const Tables &t, Sink &out, float *lim, int lim_stride) {
    const int top = t.elev_num - 1;
    if (s.phase == PH_NEWAZ && s.k >= t.azim_num) return false;
    if (s.phase == PH_BIN || s.k == 0) {
        float lim_up = t.up, lim_low = t.low;
        if (s.phase == PH_BIN) {                             // :417-424
            const float e0 = t.elev_ang[s.ind];
            lim_up = lim[0]; lim_low = lim[lim_stride];
            if (hit) lim_low = e0; else lim_up = e0;
        }
        const float elev_samp = half_sum(lim_up, lim_low);
        s.ind = ind_of(t, elev_samp);
        s.phase = PH_BIN;
        const float e = t.elev_ang[s.ind];
        if (__builtin_fmaxf(lim_up - e, e - lim_low) > t.hori_acc) {
            lim[0] = lim_up; lim[lim_stride] = lim_low;
            return true;
        }
        s.pazim = s.ind;                                     // :428
        emit<STAGE>(out, t, s.k, elev_samp);
        s.k++; s.phase = PH_NEWAZ;
        if (s.k >= t.azim_num) return false;
    }
    s.ind = max(s.pazim - 5, 0);                             // move upwards: :439-446
    s.prev = s.ind;
    s.ind = min(s.ind + 10, top);
    s.count = 1;
    s.phase = PH_UP;
    return true;
}

// advance<ALG_GUESS, STAGE> as one pass without a loop (k_horizon<..., FLAT>): the same transitions on the Search encoding, held in a SearchLean.
// After azimuth 0 a guess_constant lane is in PH_UP or PH_DOWN whenever a ray ends, and what happens next is one of
//   step on    UP with a hit below the top index, DOWN with a miss above index 0
//   turn round UP with a miss (or a hit at the top) on the first sample
//   finalize   everything else: the midpoint entry is emitted and azimuth k + 1 starts with its first UP sample
// The three cases are 0 / -1 words in vector registers, combined with AND / OR / bit-select (the empty asm hides them from the
// compiler's mask algebra, as in hz_trace: no scalar logic on vector compares, no exec-mask branch per case).  PH_BIN and PH_NEWAZ
// (azimuth 0) run the state machine above behind a wave-uniform branch; so does the midpoint of a step that was clamped at a table
// end.  PH_EMIT does not persist, as before.
//   issue_k(k')     called once the azimuth of the next ray is known (k' <= azim_num - 1: a lane that finishes keeps the last one)
//   issue_ind(ind') called once its table index is known
// are where the caller issues the loads of the new ray, so that they are in flight together with / right behind the midpoint pair.
#define HZ_HIDE(m) asm volatile("" : "+v"(m))
#define HZ_BSEL(m, x, y) (((m) & (x)) | (~(m) & (y)))
template <bool STAGE, class FK, class FI>
__device__ __forceinline__ bool advance_guess_flat(SearchLean &s, bool hit, const Tables &t, Sink &out, unsigned &guards,
                                                   float *lim, int lim_stride, FK &&issue_k, FI &&issue_ind) {
    const int top = t.elev_num - 1;
    int m_flat = (int)((unsigned)s.phase << 30) >> 31;       // PH_UP = 2, PH_DOWN = 3: bit 1
    HZ_HIDE(m_flat);
    if (__ballot(m_flat == 0) != 0ull) {                     // azimuth 0 only: no lane takes this after the first rays of a block
        if (m_flat == 0) (void)advance_az0_lean<STAGE>(s, hit, t, out, lim, lim_stride);      // (false: s.k == azim_num, see the return below)
    }
    // ---- decide ----  (every case mask is inside m_flat: the lanes of the branch above keep the state it left)
    int m_down = (int)((unsigned)s.phase << 31) >> 31;
    int m_hit = hit ? -1 : 0;
    int m_end = (s.ind == (top & ~m_down)) ? -1 : 0;         // at the index the phase cannot step beyond
    int m_many = (1 - s.count) >> 31;                        // count > 1
    HZ_HIDE(m_down); HZ_HIDE(m_hit); HZ_HIDE(m_end); HZ_HIDE(m_many);
    const int m_fwd = (m_hit ^ m_down) & m_flat;             // the ray says "further": blocked on the way up, free on the way down
    const int m_step = m_fwd & ~m_end;
    const int m_turn = m_flat & ~(m_step | m_down | m_many);
    const int m_fin = m_flat & ~(m_step | m_turn);
    guards += (unsigned)(m_fwd & m_end & 1);                 // the reference never leaves this loop
    // ---- the three successors ----
    const int st_ind = min(max(s.ind + 10 - (20 & m_down), 0), top);
    const int tu_prev = min(s.pazim + 5, top), tu_ind = max(tu_prev - 10, 0);
    const int lo = min(s.prev, s.ind), hi = max(s.prev, s.ind);
    const int2 pair = reinterpret_cast<const int2 *>(t.mid_idx)[min(max(lo, 0), top)];      // (all lanes: inside the table whatever the state)
    int m_gen = (hi - lo != 10) ? m_fin : 0;                 // a step clamped at a table end: the general midpoint
    HZ_HIDE(m_gen);
    const int k_new = s.k - m_fin;
    issue_k(min(k_new, t.azim_num - 1));                     // (k_new == azim_num: that was the cell's last azimuth)
    int mid = pair.x, evb = pair.y;
    if (__ballot(m_gen != 0) != 0ull) {
        if (m_gen != 0) {
            mid = ind_of(t, half_sum(t.elev_ang[s.prev], t.elev_ang[s.ind]));
            evb = __float_as_int(t.elev_ang[mid]);
        }
    }
    const int fi_prev = max(mid - 5, 0), fi_ind = min(fi_prev + 10, top);
    const int ind_new = HZ_BSEL(m_step, st_ind, HZ_BSEL(m_turn, tu_ind, HZ_BSEL(m_fin, fi_ind, s.ind)));
    issue_ind(ind_new);
    const int k_emit = s.k;
    s.prev = HZ_BSEL(m_step, s.ind, HZ_BSEL(m_turn, tu_prev, HZ_BSEL(m_fin, fi_prev, s.prev)));
    s.ind = ind_new;
    s.count = HZ_BSEL(m_fin, 1, s.count + (m_step & ~m_down & 1));
    s.phase += m_turn & 1;                                   // UP -> DOWN
    s.phase -= m_fin & m_down & 1;                           // DOWN -> UP (azimuth k + 1)
    s.pazim = HZ_BSEL(m_fin, mid, s.pazim);
    s.k = k_new;
    if (m_fin != 0) emit<STAGE>(out, t, k_emit, __int_as_float(evb));      // one exec-mask region: the lanes that finalize
    return s.k < t.azim_num;
}
#undef HZ_BSEL
#undef HZ_HIDE

}  // namespace hz
