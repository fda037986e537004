/* Stand-in for the HDK's UT_Vector3T: three components, component-wise arithmetic, explicit conversion
 * between component types (a cast per component, so double -> integer truncates toward zero).  See
 * SYS/SYS_Types.h for the stand-in tree's semantics. */
#ifndef REFSTANDIN_UT_VECTOR3_H
#define REFSTANDIN_UT_VECTOR3_H

#include <SYS/SYS_Types.h>

template <typename T>
class UT_Vector3T
{
public:
    UT_Vector3T() : v{T(0), T(0), T(0)} {}
    explicit UT_Vector3T(T s) : v{s, s, s} {}
    UT_Vector3T(T x, T y, T z) : v{x, y, z} {}
    template <typename S, typename = std::enable_if_t<!std::is_same<S, T>::value>>
    explicit UT_Vector3T(const UT_Vector3T<S> &o) : v{T(o[0]), T(o[1]), T(o[2])}
    {
    }

    T &operator[](int a) { return v[a]; }
    const T &operator[](int a) const { return v[a]; }
    T x() const { return v[0]; }
    T y() const { return v[1]; }
    T z() const { return v[2]; }
    T maxComponent() const { return std::max(v[0], std::max(v[1], v[2])); }

    bool operator==(const UT_Vector3T &o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
    bool operator!=(const UT_Vector3T &o) const { return !(*this == o); }

    UT_Vector3T operator+(const UT_Vector3T &o) const { return UT_Vector3T(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
    UT_Vector3T operator-(const UT_Vector3T &o) const { return UT_Vector3T(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
    UT_Vector3T operator-() const { return UT_Vector3T(-v[0], -v[1], -v[2]); }
    UT_Vector3T &operator+=(const UT_Vector3T &o)
    {
        for (int a = 0; a < 3; ++a) v[a] += o.v[a];
        return *this;
    }
    UT_Vector3T &operator-=(const UT_Vector3T &o)
    {
        for (int a = 0; a < 3; ++a) v[a] -= o.v[a];
        return *this;
    }

private:
    T v[3];
};

template <typename T, typename S, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline UT_Vector3T<T> operator*(S s, const UT_Vector3T<T> &a)
{
    return UT_Vector3T<T>(T(s) * a[0], T(s) * a[1], T(s) * a[2]);
}
template <typename T, typename S, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline UT_Vector3T<T> operator*(const UT_Vector3T<T> &a, S s)
{
    return UT_Vector3T<T>(a[0] * T(s), a[1] * T(s), a[2] * T(s));
}
template <typename T, typename S, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline UT_Vector3T<T> operator/(const UT_Vector3T<T> &a, S s)
{
    return UT_Vector3T<T>(a[0] / T(s), a[1] / T(s), a[2] / T(s));
}

using UT_Vector3i = UT_Vector3T<int32>;
using UT_Vector3I = UT_Vector3T<int64>;
using UT_Vector3F = UT_Vector3T<fpreal32>;
using UT_Vector3D = UT_Vector3T<fpreal64>;
using UT_Vector3 = UT_Vector3T<fpreal32>;

#endif
