/*
 * Stand-in for <tbb/parallel_for.h> -- TEST INFRASTRUCTURE ONLY (oracle/Makefile, target _ref/libhz_ref.so).
 * Serial: the body sees the whole range once, on the calling thread.  The reference's cells are independent
 * (every cell writes its own output words), so the order of execution cannot change a result.
 */
#ifndef HZ_REF_STANDIN_TBB_PARALLEL_FOR_H
#define HZ_REF_STANDIN_TBB_PARALLEL_FOR_H

#include "blocked_range.h"

namespace tbb {

template <typename Range, typename Body>
void parallel_for(const Range &range, const Body &body) {
    if (!range.empty()) body(range);
}

}  // namespace tbb

#endif
