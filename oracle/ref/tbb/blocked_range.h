/*
 * Stand-in for oneTBB's blocked_range -- TEST INFRASTRUCTURE ONLY (oracle/Makefile, target _ref/libhz_ref.so).
 * A half-open index interval; the serial parallel_for / parallel_reduce of this directory never split it.
 */
#ifndef HZ_REF_STANDIN_TBB_BLOCKED_RANGE_H
#define HZ_REF_STANDIN_TBB_BLOCKED_RANGE_H

namespace tbb {

template <typename T>
class blocked_range {
public:
    blocked_range(T first, T last) : first_(first), last_(last) {}
    T begin() const { return first_; }
    T end() const { return last_; }
    bool empty() const { return !(first_ < last_); }

private:
    T first_, last_;
};

}  // namespace tbb

#endif
