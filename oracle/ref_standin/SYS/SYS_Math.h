/* Stand-in for the HDK's SYS_Math.h: the three helpers the reference solver core uses.  See SYS_Types.h. */
#ifndef REFSTANDIN_SYS_MATH_H
#define REFSTANDIN_SYS_MATH_H

#include "SYS_Types.h"

template <typename T>
inline T SYSsqrt(T v)
{
    return std::sqrt(v);
}
template <typename T>
inline T SYSmax(T a, T b)
{
    return a > b ? a : b;
}
template <typename T>
inline T SYSmin(T a, T b)
{
    return a < b ? a : b;
}

#endif
