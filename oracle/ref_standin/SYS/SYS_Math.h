/* Stand-in for the HDK's SYS_Math.h: the helpers the reference uses.  See SYS_Types.h. */
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
// v held to [lo, hi]: lo where v < lo, hi where v > hi, v itself otherwise
template <typename T>
inline T SYSclamp(T v, T lo, T hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

#endif
