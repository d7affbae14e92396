// hz_sight_search.h -- the per-lane search of Terrain.sight_height (DESIGN.md section 4 clause 19) as a resumable state
// machine: which entry of the height table the cell's next ray aims at, given the answer of the last one.  Top of the table
// first, then its bottom, then a bisection between the two: 1 ray for a cell nothing reaches, 2 for one seen at H[0],
// 2 + ceil(log2(n - 1)) at the most.  No arithmetic on heights, only on indices.
//
// It includes nothing and names no device type, so a host program can compile it as it stands (tests/sight_search_host.cpp
// drives it through every table length and every first visible index under ASan + UBSan).
#pragma once

#if defined(__HIPCC__)
#define HZ_SIGHT_FN __host__ __device__ __forceinline__
#else
#define HZ_SIGHT_FN inline
#endif

namespace hz {

// the phase of a lane; 0 doubles as "the lane has no cell"
enum { SIGHT_IDLE = 0, SIGHT_TOP = 1, SIGHT_BOTTOM = 2, SIGHT_BISECT = 3 };
// what sight_advance returns instead of a table index when the cell is finished with +inf; a finished cell with a finite
// result returns SIGHT_DONE - 1 - index
enum { SIGHT_UNREACHED = -1, SIGHT_DONE = -2 };

HZ_SIGHT_FN bool sight_is_index(int k) { return k >= 0; }
HZ_SIGHT_FN int sight_result_index(int k) { return SIGHT_DONE - 1 - k; }       // of a finished cell that is not SIGHT_UNREACHED

// lo in bits 0 - 15, hi in bits 16 - 31 (n <= 65535: indices <= 65534)
HZ_SIGHT_FN unsigned sight_pack(int lo, int hi) { return (unsigned)lo | ((unsigned)hi << 16); }
HZ_SIGHT_FN int sight_lo(unsigned lohi) { return (int)(lohi & 0xffffu); }
HZ_SIGHT_FN int sight_hi(unsigned lohi) { return (int)(lohi >> 16); }

// The first ray of a cell aims at the top of the table.
HZ_SIGHT_FN int sight_begin(int &phase, unsigned &lohi, int n) {
    phase = SIGHT_TOP;
    lohi = sight_pack(0, n - 1);
    return n - 1;
}

// The ray at the index the lane was given last is decided (`visible`: nothing in between, or no ray was needed).  Returns the
// next index to trace (>= 0, phase and lohi advanced), SIGHT_UNREACHED, or SIGHT_DONE - 1 - the result's index; a finished
// cell leaves the lane SIGHT_IDLE.
HZ_SIGHT_FN int sight_advance(int &phase, unsigned &lohi, int n, bool visible) {
    int lo = sight_lo(lohi), hi = sight_hi(lohi);
    if (phase == SIGHT_TOP) {
        if (!visible) { phase = SIGHT_IDLE; return SIGHT_UNREACHED; }
        if (n == 1) { phase = SIGHT_IDLE; return sight_result_index(0); }
        phase = SIGHT_BOTTOM;
        return 0;
    }
    if (phase == SIGHT_BOTTOM) {
        if (visible) { phase = SIGHT_IDLE; return sight_result_index(0); }
    } else {                                    // SIGHT_BISECT: the ray aimed at (lo + hi) >> 1
        const int mid = (lo + hi) >> 1;
        if (visible) hi = mid; else lo = mid;
        lohi = sight_pack(lo, hi);
    }
    if (hi - lo > 1) { phase = SIGHT_BISECT; return (lo + hi) >> 1; }
    phase = SIGHT_IDLE;
    return sight_result_index(hi);
}

}  // namespace hz
