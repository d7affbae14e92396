/*
 * Stand-in for <tbb/parallel_reduce.h> -- TEST INFRASTRUCTURE ONLY (oracle/Makefile, target _ref/libhz_ref.so).
 * Serial form of the functional overload parallel_reduce(range, identity, body, reduction).  As in oneTBB the
 * value type is the type of `identity`: the reference passes 0.0, so its ray count travels through a double
 * (exact below 2^53) whatever its body takes and returns.  With one chunk the reduction is never called.
 */
#ifndef HZ_REF_STANDIN_TBB_PARALLEL_REDUCE_H
#define HZ_REF_STANDIN_TBB_PARALLEL_REDUCE_H

#include "blocked_range.h"

namespace tbb {

template <typename Range, typename Value, typename Body, typename Reduction>
Value parallel_reduce(const Range &range, const Value &identity, const Body &body, const Reduction &) {
    if (range.empty()) return identity;
    return static_cast<Value>(body(range, identity));
}

}  // namespace tbb

#endif
