/* Stand-in for the HDK's UT_StopWatch: wall-clock seconds between start() and stop().  See SYS/SYS_Types.h. */
#ifndef REFSTANDIN_UT_STOPWATCH_H
#define REFSTANDIN_UT_STOPWATCH_H

#include <chrono>

class UT_StopWatch
{
public:
    void start() { myStart = std::chrono::steady_clock::now(); }
    double stop() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - myStart).count(); }
    double lap() { return stop(); }
    void clear() { myStart = std::chrono::steady_clock::time_point(); }

private:
    std::chrono::steady_clock::time_point myStart;
};

#endif
