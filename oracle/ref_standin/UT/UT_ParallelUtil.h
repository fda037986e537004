/* Stand-in for the HDK's threading helpers (UT_ParallelUtil.h, UT_ThreadedAlgorithm.h, UT_JobInfo.h,
 * UT_Thread.h): one job, one processor.  Every body runs once, serially, over the whole range, so the
 * per-thread lists the reference concatenates are a single list in visiting order.  See SYS/SYS_Types.h. */
#ifndef REFSTANDIN_UT_PARALLELUTIL_H
#define REFSTANDIN_UT_PARALLELUTIL_H

#include <SYS/SYS_Math.h>
#include <UT/UT_Array.h>
#include <UT/UT_Interrupt.h>

template <typename T>
class UT_BlockedRange
{
public:
    UT_BlockedRange(T b, T e, size_t = 1) : myBegin(b), myEnd(e) {}
    T begin() const { return myBegin; }
    T end() const { return myEnd; }
    bool empty() const { return !(myBegin < myEnd); }

private:
    T myBegin, myEnd;
};

template <typename Range, typename Body>
inline void UTparallelFor(const Range &range, const Body &body, int = 2, int = 1)
{
    body(range);
}
template <typename Range, typename Body>
inline void UTparallelForLightItems(const Range &range, const Body &body)
{
    body(range);
}
template <typename Range, typename Body>
inline void UTparallelForHeavyItems(const Range &range, const Body &body)
{
    body(range);
}
template <typename Range, typename Body>
inline void UTserialFor(const Range &range, const Body &body)
{
    body(range);
}
template <typename IntType, typename Body>
inline void UTparallelForEachNumber(IntType n, const Body &body)
{
    body(UT_BlockedRange<IntType>(IntType(0), n));
}
template <typename It, typename Compare>
inline void UTparallelSort(It begin, It end, const Compare &less)
{
    std::sort(begin, end, less);
}

class UT_Thread
{
public:
    static int getNumProcessors() { return 1; }
};

class UT_JobInfo
{
public:
    int job() const { return 0; }
    int numJobs() const { return 1; }
    template <typename I>
    void divideWork(I units, I &start, I &end) const
    {
        start = 0;
        end = units;
    }
};

class UT_ThreadedAlgorithm
{
public:
    template <typename Body>
    void run(const Body &body)
    {
        UT_JobInfo info;
        body(info);
    }
};

#endif
