/*
 * Stand-in for the HDK's UT_VoxelArray family, written from the HDK's documented behaviour.  See
 * SYS/SYS_Types.h for the semantics of the whole stand-in tree; the ones that live here:
 *
 *   - storage is dense, x fastest: voxel (x, y, z) is element (z * ny + y) * nx + x;
 *   - tiles are 16^3 (the last tile of an axis may be partial); linear tile number = tx + ntx * (ty + nty * tz);
 *   - UT_VoxelArrayIterator walks tiles myTileStart .. myTileEnd - 1 in that order and, inside a tile, its
 *     voxels x fastest, then y, then z.  rewind() goes to the first voxel of tile myTileStart; atEnd() is
 *     true once the tile number reaches myTileEnd; advanceTile() goes to the first voxel of the next tile;
 *     getTileVoxels(start, end) gives the tile's voxel box, end exclusive; splitByTile(info) keeps the whole
 *     tile range (one job);
 *   - nothing is ever compressed: isTileConstant() and a tile's isConstant() return false, uncompress(),
 *     collapseAllTiles() and setCompressOnExit() do nothing, constant(v) fills.  The ARRAY's isConstant(&v)
 *     answers by value: true, with the value in v, where every voxel holds the same value (what the HDK
 *     reports of an array after constant(v)); the plugin asks it of the density field only;
 *   - UT_VoxelProbe and UT_VoxelProbeCube hold only an index: getValue reads the array, setValue writes it,
 *     at once (write-through, no cached line).  A read or write outside the array throws: the reference
 *     never relies on border behaviour, and a stand-in that invented one would hide it if it did.
 */
#ifndef REFSTANDIN_UT_VOXELARRAY_H
#define REFSTANDIN_UT_VOXELARRAY_H

#include <SYS/SYS_Math.h>
#include <UT/UT_Array.h>
#include <UT/UT_ParallelUtil.h>
#include <UT/UT_Vector3.h>

constexpr int REFSTANDIN_TILE = 16;

class UT_VoxelTileStandin
{
public:
    bool isConstant() const { return false; }
    void uncompress() {}
};

template <typename T>
class UT_VoxelArrayIterator;

template <typename T>
class UT_VoxelArray
{
public:
    void size(int nx, int ny, int nz)
    {
        myRes[0] = nx;
        myRes[1] = ny;
        myRes[2] = nz;
        for (int a = 0; a < 3; ++a) myTileRes[a] = (myRes[a] + REFSTANDIN_TILE - 1) / REFSTANDIN_TILE;
        myData.assign(size_t(nx) * size_t(ny) * size_t(nz), T(0));
    }
    void constant(T v) { std::fill(myData.begin(), myData.end(), v); }

    UT_Vector3I getVoxelRes() const { return UT_Vector3I(myRes[0], myRes[1], myRes[2]); }
    int getXRes() const { return myRes[0]; }
    int getYRes() const { return myRes[1]; }
    int getZRes() const { return myRes[2]; }
    int getRes(int axis) const { return myRes[axis]; }
    exint numVoxels() const { return exint(myData.size()); }

    int numTiles() const { return myTileRes[0] * myTileRes[1] * myTileRes[2]; }
    int getTileRes(int axis) const { return myTileRes[axis]; }
    int indexToLinearTile(exint x, exint y, exint z) const
    {
        check(x, y, z);
        return int(x / REFSTANDIN_TILE) + myTileRes[0] * (int(y / REFSTANDIN_TILE) + myTileRes[1] * int(z / REFSTANDIN_TILE));
    }
    void linearTileToXYZ(int tile, int &tx, int &ty, int &tz) const
    {
        tx = tile % myTileRes[0];
        ty = (tile / myTileRes[0]) % myTileRes[1];
        tz = tile / (myTileRes[0] * myTileRes[1]);
    }
    UT_VoxelTileStandin *getLinearTile(exint) const { return &theTile(); }
    void collapseAllTiles() {}
    bool isConstant(T *value = nullptr) const
    {
        for (const T &v : myData)
            if (!(v == myData.front())) return false;
        if (value && !myData.empty()) *value = myData.front();
        return true;
    }

    T operator()(const UT_Vector3I &c) const { return myData[index(c[0], c[1], c[2])]; }
    T operator()(exint x, exint y, exint z) const { return myData[index(x, y, z)]; }
    T getValue(exint x, exint y, exint z) const { return myData[index(x, y, z)]; }
    void setValue(const UT_Vector3I &c, T v) { myData[index(c[0], c[1], c[2])] = v; }
    void setValue(exint x, exint y, exint z, T v) { myData[index(x, y, z)] = v; }

    // flat access for the driver
    T *rawData() { return myData.data(); }
    const T *rawData() const { return myData.data(); }

private:
    void check(exint x, exint y, exint z) const
    {
        if (x < 0 || y < 0 || z < 0 || x >= myRes[0] || y >= myRes[1] || z >= myRes[2])
            throw refstandin::AssertionFailed("stand-in UT_VoxelArray: access outside the array at (" + std::to_string(x) + ", " +
                                              std::to_string(y) + ", " + std::to_string(z) + ")");
    }
    size_t index(exint x, exint y, exint z) const
    {
        check(x, y, z);
        return (size_t(z) * size_t(myRes[1]) + size_t(y)) * size_t(myRes[0]) + size_t(x);
    }
    static UT_VoxelTileStandin &theTile()
    {
        static UT_VoxelTileStandin tile;
        return tile;
    }

    int myRes[3] = {0, 0, 0};
    int myTileRes[3] = {0, 0, 0};
    std::vector<T> myData;
};

// Shared by the array iterator (tiles myTileStart .. myTileEnd - 1) and the tile iterator (one tile).
template <typename T>
class UT_VoxelArrayIterator
{
public:
    UT_VoxelArrayIterator() = default;
    explicit UT_VoxelArrayIterator(UT_VoxelArray<T> *array) { setArray(array); }
    void setCompressOnExit(bool) {}
    void setArray(UT_VoxelArray<T> *array)
    {
        myArray = array;
        myTileStart = 0;
        myTileEnd = array->numTiles();
        rewind();
    }
    void setConstArray(const UT_VoxelArray<T> *array) { setArray(const_cast<UT_VoxelArray<T> *>(array)); }
    template <typename JobInfo>
    void splitByTile(const JobInfo &)
    {
        myTileStart = 0;
        myTileEnd = myArray->numTiles();
        rewind();
    }

    void rewind()
    {
        myCurTile = myTileStart;
        enterTile();
    }
    bool atEnd() const { return myCurTile >= myTileEnd; }
    void advance()
    {
        if (++myPos[0] < myEnd[0]) return;
        myPos[0] = myStart[0];
        if (++myPos[1] < myEnd[1]) return;
        myPos[1] = myStart[1];
        if (++myPos[2] < myEnd[2]) return;
        advanceTile();
    }
    void advanceTile()
    {
        ++myCurTile;
        enterTile();
    }

    int x() const { return myPos[0]; }
    int y() const { return myPos[1]; }
    int z() const { return myPos[2]; }
    T getValue() const { return (*myArray)(myPos[0], myPos[1], myPos[2]); }
    void setValue(T v) const { myArray->setValue(myPos[0], myPos[1], myPos[2], v); }

    bool isTileConstant() const { return false; }
    int getLinearTileNum() const { return myCurTile; }
    void getTileVoxels(UT_Vector3I &start, UT_Vector3I &end) const
    {
        start = UT_Vector3I(myStart[0], myStart[1], myStart[2]);
        end = UT_Vector3I(myEnd[0], myEnd[1], myEnd[2]);
    }
    UT_VoxelArray<T> *getArray() const { return myArray; }

    int myTileStart = 0, myTileEnd = 0;

private:
    void enterTile()
    {
        if (!myArray || myCurTile >= myTileEnd || myCurTile >= myArray->numTiles()) return;
        int t[3];
        myArray->linearTileToXYZ(myCurTile, t[0], t[1], t[2]);
        for (int a = 0; a < 3; ++a)
        {
            myStart[a] = t[a] * REFSTANDIN_TILE;
            myEnd[a] = std::min(myStart[a] + REFSTANDIN_TILE, myArray->getRes(a));
            myPos[a] = myStart[a];
        }
    }

    UT_VoxelArray<T> *myArray = nullptr;
    int myCurTile = 0;
    int myStart[3] = {0, 0, 0}, myEnd[3] = {0, 0, 0}, myPos[3] = {0, 0, 0};
};

template <typename T>
class UT_VoxelTileIterator
{
public:
    template <typename S>
    void setTile(const UT_VoxelArrayIterator<S> &vit)
    {
        static_assert(std::is_same<S, T>::value, "tile iterator over the array iterator's own array");
        myIt.setArray(vit.getArray());
        myIt.myTileStart = vit.getLinearTileNum();
        myIt.myTileEnd = vit.getLinearTileNum() + 1;
        myIt.rewind();
    }
    void rewind() { myIt.rewind(); }
    bool atEnd() const { return myIt.atEnd(); }
    void advance() { myIt.advance(); }
    int x() const { return myIt.x(); }
    int y() const { return myIt.y(); }
    int z() const { return myIt.z(); }
    T getValue() const { return myIt.getValue(); }
    void setValue(T v) const { myIt.setValue(v); }

private:
    UT_VoxelArrayIterator<T> myIt;
};

using UT_VoxelArrayF = UT_VoxelArray<fpreal32>;
using UT_VoxelArrayI = UT_VoxelArray<int64>;
using UT_VoxelArrayIteratorF = UT_VoxelArrayIterator<fpreal32>;
using UT_VoxelArrayIteratorI = UT_VoxelArrayIterator<int64>;
using UT_VoxelTileIteratorF = UT_VoxelTileIterator<fpreal32>;
using UT_VoxelTileIteratorI = UT_VoxelTileIterator<int64>;

// One row along x around an index; prex / postx (the cached span in the HDK) carry no meaning here.
template <typename T, bool DoRead, bool DoWrite, bool TestForWrites>
class UT_VoxelProbe
{
public:
    void setArray(UT_VoxelArray<T> *array, int = 0, int = 0) { myArray = array; }
    void setConstArray(const UT_VoxelArray<T> *array, int = 0, int = 0) { myArray = const_cast<UT_VoxelArray<T> *>(array); }

    bool setIndex(exint x, exint y, exint z)
    {
        myPos[0] = x;
        myPos[1] = y;
        myPos[2] = z;
        return true;
    }
    template <typename S>
    bool setIndex(const UT_VoxelArrayIterator<S> &vit)
    {
        return setIndex(vit.x(), vit.y(), vit.z());
    }

    T getValue() const { return (*myArray)(myPos[0], myPos[1], myPos[2]); }
    T getValue(int dx) const { return (*myArray)(myPos[0] + dx, myPos[1], myPos[2]); }
    void setValue(T v) { myArray->setValue(myPos[0], myPos[1], myPos[2], v); }

private:
    UT_VoxelArray<T> *myArray = nullptr;
    exint myPos[3] = {0, 0, 0};
};

// The 3^3 neighbourhood of an index ("plus": the six face neighbours; the cube form reads the same way).
template <typename T>
class UT_VoxelProbeCube
{
public:
    void setConstPlusArray(const UT_VoxelArray<T> *array) { myArray = array; }
    void setConstCubeArray(const UT_VoxelArray<T> *array) { myArray = array; }

    bool setIndexPlus(exint x, exint y, exint z)
    {
        myPos[0] = x;
        myPos[1] = y;
        myPos[2] = z;
        return true;
    }
    template <typename S>
    bool setIndexPlus(const UT_VoxelArrayIterator<S> &vit)
    {
        return setIndexPlus(vit.x(), vit.y(), vit.z());
    }
    bool setIndexCube(exint x, exint y, exint z) { return setIndexPlus(x, y, z); }
    template <typename S>
    bool setIndexCube(const UT_VoxelArrayIterator<S> &vit)
    {
        return setIndexPlus(vit);
    }

    T getValue() const { return (*myArray)(myPos[0], myPos[1], myPos[2]); }
    T getValue(int dx, int dy, int dz) const { return (*myArray)(myPos[0] + dx, myPos[1] + dy, myPos[2] + dz); }
    T getValue(const UT_Vector3I &offset) const
    {
        return (*myArray)(myPos[0] + offset[0], myPos[1] + offset[1], myPos[2] + offset[2]);
    }

private:
    const UT_VoxelArray<T> *myArray = nullptr;
    exint myPos[3] = {0, 0, 0};
};

#endif
