/* Stand-in for the HDK's UT_Array: a growable array over std::vector.  bool entries are stored as
 * bytes so that operator[] yields a real reference.  See SYS/SYS_Types.h. */
#ifndef REFSTANDIN_UT_ARRAY_H
#define REFSTANDIN_UT_ARRAY_H

#include <SYS/SYS_Types.h>

template <typename T>
class UT_Array
{
    using Stored = std::conditional_t<std::is_same<T, bool>::value, unsigned char, T>;

public:
    using iterator = typename std::vector<Stored>::iterator;
    using const_iterator = typename std::vector<Stored>::const_iterator;

    void setSize(exint n) { myData.resize(size_t(n)); }
    exint size() const { return exint(myData.size()); }
    exint entries() const { return exint(myData.size()); }
    bool isEmpty() const { return myData.empty(); }
    void clear() { myData.clear(); }
    void bumpCapacity(exint n) { myData.reserve(size_t(n)); }
    void constant(const T &v) { std::fill(myData.begin(), myData.end(), Stored(v)); }
    exint append(const T &v)
    {
        myData.push_back(Stored(v));
        return exint(myData.size()) - 1;
    }
    void concat(const UT_Array &o) { myData.insert(myData.end(), o.myData.begin(), o.myData.end()); }

    Stored &operator[](exint i) { return myData[size_t(i)]; }
    const Stored &operator[](exint i) const { return myData[size_t(i)]; }
    Stored &operator()(exint i) { return myData[size_t(i)]; }
    const Stored &operator()(exint i) const { return myData[size_t(i)]; }

    iterator begin() { return myData.begin(); }
    iterator end() { return myData.end(); }
    const_iterator begin() const { return myData.begin(); }
    const_iterator end() const { return myData.end(); }

private:
    std::vector<Stored> myData;
};

#endif
