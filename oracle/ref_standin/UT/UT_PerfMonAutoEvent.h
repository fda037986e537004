/* Stand-in for the HDK's UT_PerfMonAutoSolveEvent, a scoped timing event of the performance monitor: records
 * nothing.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_UT_PERFMONAUTOEVENT_H
#define REFSTANDIN_UT_PERFMONAUTOEVENT_H

class UT_PerfMonAutoSolveEvent
{
public:
    UT_PerfMonAutoSolveEvent(const void *, const char *) {}
    ~UT_PerfMonAutoSolveEvent() {}
};

#endif
