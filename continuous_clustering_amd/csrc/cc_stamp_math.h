// cc_stamp_math.h — the rules of the firing-stamp log (include/cc_stamps.h) as one text for the kernels of cc_stamps.hip
// and their host twins. Integers only: nothing here rounds, so host and device agree bit for bit and no launch shape can change a result.
#ifndef CC_STAMP_MATH_H
#define CC_STAMP_MATH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCS_HD __host__ __device__ inline
#else
#define CCS_HD inline
#endif

namespace ccs
{

// What the log knows of one stream: `head` is the index the next pushed firing gets, firings below `floor` are forgotten (seek, reset).
struct Log
{
    uint64_t head, floor;
};

// The stamp of the firing whose index has the low 32 bits f, or 0 with *missing = true when the log does not hold that firing.
// ring: the stream's `capacity` slots (a power of two); the firing with index i lives in slot i & (capacity - 1).
CCS_HD uint64_t resolve(const uint64_t* ring, uint64_t capacity, Log log, uint32_t f, bool* missing)
{
    *missing = true;
    if (log.head == 0 || log.head == log.floor)
        return 0;
    const uint64_t last = log.head - 1;
    const uint64_t idx = last - (uint64_t) (uint32_t) ((uint32_t) last - f); // the newest pushed firing with these low bits
    if (last - idx >= capacity || idx < log.floor)                           // (an idx that wrapped below 0 fails the first test)
        return 0;
    *missing = false;
    return ring[idx & (capacity - 1)];
}

// ros::Time::fromNSec: seconds truncated to 32 bits, and the nanoseconds left over
CCS_HD void sec_nsec(uint64_t stamp, uint32_t* sec, uint32_t* nsec)
{
    *sec = (uint32_t) (stamp / 1000000000ull);
    *nsec = (uint32_t) (stamp % 1000000000ull);
}

// The reference's header stamp is the minimum NON-ZERO point stamp, 0 where there is none (ros_utils.cpp:51-71). With the key
// stamp - 1 (0 wraps to 2^64 - 1) that is a plain unsigned minimum: min-non-zero = min(key) + 1, and the identity 2^64 - 1 wraps back to 0.
CCS_HD uint64_t nonzero_min_key(uint64_t stamp)
{
    return stamp - 1;
}
CCS_HD uint64_t nonzero_min_from_key(uint64_t key)
{
    return key + 1;
}

// stamp_cluster of cc.cpp:1025-1028. min + (max - min) / 2, never (min + max) / 2: the sum overflows for stamps above 2^63.
CCS_HD uint64_t cluster_stamp(uint64_t min_stamp, uint64_t max_stamp, bool use_last_point)
{
    return use_last_point ? max_stamp : min_stamp + (max_stamp - min_stamp) / 2;
}

// The stream whose slice holds record i: the last s with first(s) <= i (slices abut in stream order, so the empty ones before the holder
// share its first record and the empty ones after it start above i). -1 when even first(0) > i.
template <class First>
CCS_HD int slice_of(int n, int64_t i, First first)
{
    int lo = 0, hi = n; // first(lo - 1) <= i < first(hi), with first(-1) = -inf and first(n) = +inf
    while (lo < hi)
    {
        const int mid = lo + (hi - lo) / 2;
        if (first(mid) <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

} // namespace ccs
#endif
