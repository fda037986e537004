/*
 * Stand-in for the HDK's SIM_RawField and SIM_RawIndexField, written from the HDK's documented behaviour for
 * the one purpose of compiling the reference's plugin files (HDK_GeometricFreeSurfacePressureSolver.{h,cpp},
 * HDK_Utilities.{h,cpp}) into oracle/_ref/libmgref_fields.so.  TEST INFRASTRUCTURE ONLY; nothing here is taken
 * from the HDK or from the reference.  See SYS/SYS_Types.h for the semantics of the whole tree; the ones that
 * live here:
 *
 *   - a raw field stores fpreal32 samples (an index field int64) in a dense UT_VoxelArray; whatever the plugin
 *     writes into one is rounded to fpreal32 where it is stored;
 *   - init(sample, orig, size, xres, yres, zres) takes the VOXEL (cell) counts; getVoxelRes() returns them.  A
 *     face-sampled field holds one more sample along its axis, a corner-sampled one along every axis: that is
 *     the size of field();
 *   - tiles are never constant (UT/UT_VoxelArray.h); makeConstant(v) fills every sample;
 *   - the voxel size is size / res per axis; indexToPos gives orig + (index + offset) * voxel size in fpreal32,
 *     offset 1/2 along every axis for centre sampling, 0 along its own axis for face sampling, 0 everywhere
 *     for corners;
 *   - getValue(pos) is the trilinear interpolant of the samples: the position in sample space is
 *     (pos - orig) / voxel size - offset, clamped to [0, samples - 1] per axis; i = floor, t = the rest; each
 *     axis blends as (1 - t) a + t b, x first, then y, then z, in fpreal32.  A position that is a sample has
 *     t = 0 on every axis and returns that sample bit for bit;
 *   - isAligned(other): same sampling, voxel counts, origin and size.
 */
#ifndef REFSTANDIN_SIM_RAWFIELD_H
#define REFSTANDIN_SIM_RAWFIELD_H

#include <UT/UT_Vector3.h>
#include <UT/UT_VoxelArray.h>

enum SIM_FieldSample
{
    SIM_SAMPLE_CENTER,
    SIM_SAMPLE_FACEX,
    SIM_SAMPLE_FACEY,
    SIM_SAMPLE_FACEZ,
    SIM_SAMPLE_CORNER
};

template <typename T>
class SIM_RawFieldStandin
{
public:
    void init(SIM_FieldSample sample, const UT_Vector3 &orig, const UT_Vector3 &size, int xres, int yres, int zres)
    {
        mySample = sample;
        myOrig = orig;
        mySize = size;
        myRes[0] = xres;
        myRes[1] = yres;
        myRes[2] = zres;
        int samples[3];
        for (int a = 0; a < 3; ++a)
        {
            myVoxelSize[a] = size[a] / fpreal32(myRes[a]);
            samples[a] = myRes[a] + (hasSampleOnLowerFace(a) ? 1 : 0);
        }
        myField.size(samples[0], samples[1], samples[2]);
    }
    template <typename S>
    void match(const SIM_RawFieldStandin<S> &src)
    {
        init(src.getSample(), src.getOrig(), src.getSize(), int(src.getVoxelRes()[0]), int(src.getVoxelRes()[1]), int(src.getVoxelRes()[2]));
    }
    void makeConstant(T v) { myField.constant(v); }

    const UT_VoxelArray<T> *field() const { return &myField; }
    UT_VoxelArray<T> *fieldNC() const { return const_cast<UT_VoxelArray<T> *>(&myField); }

    SIM_FieldSample getSample() const { return mySample; }
    const UT_Vector3 &getOrig() const { return myOrig; }
    const UT_Vector3 &getSize() const { return mySize; }
    const UT_Vector3 &getVoxelSize() const { return myVoxelSize; }
    UT_Vector3I getVoxelRes() const { return UT_Vector3I(myRes[0], myRes[1], myRes[2]); }

    template <typename S>
    bool isAligned(const SIM_RawFieldStandin<S> *o) const
    {
        return mySample == o->getSample() && getVoxelRes() == o->getVoxelRes() && myOrig == o->getOrig() && mySize == o->getSize();
    }

    bool indexToPos(int x, int y, int z, UT_Vector3 &pos) const
    {
        const int index[3] = {x, y, z};
        for (int a = 0; a < 3; ++a) pos[a] = myOrig[a] + (fpreal32(index[a]) + sampleOffset(a)) * myVoxelSize[a];
        return true;
    }

    // 0 along an axis on which the samples sit on the voxel's lower face, 1/2 where they sit in its middle
    fpreal32 sampleOffset(int axis) const { return hasSampleOnLowerFace(axis) ? fpreal32(0) : fpreal32(0.5); }

protected:
    bool hasSampleOnLowerFace(int axis) const
    {
        return mySample == SIM_SAMPLE_CORNER || (mySample == SIM_SAMPLE_FACEX && axis == 0) || (mySample == SIM_SAMPLE_FACEY && axis == 1) ||
               (mySample == SIM_SAMPLE_FACEZ && axis == 2);
    }

    SIM_FieldSample mySample = SIM_SAMPLE_CENTER;
    UT_Vector3 myOrig, mySize, myVoxelSize;
    int myRes[3] = {0, 0, 0};
    UT_VoxelArray<T> myField;
};

class SIM_RawField : public SIM_RawFieldStandin<fpreal32>
{
public:
    fpreal getValue(UT_Vector3 pos) const
    {
        int lo[3], hi[3];
        fpreal32 t[3];
        for (int a = 0; a < 3; ++a)
        {
            const int last = myField.getRes(a) - 1;
            fpreal32 s = (pos[a] - myOrig[a]) / myVoxelSize[a] - sampleOffset(a);
            s = s < fpreal32(0) ? fpreal32(0) : (s > fpreal32(last) ? fpreal32(last) : s);
            lo[a] = int(std::floor(s));
            hi[a] = lo[a] < last ? lo[a] + 1 : last;
            t[a] = s - fpreal32(lo[a]);
        }
        auto blend = [](fpreal32 tt, fpreal32 a, fpreal32 b) { return (fpreal32(1) - tt) * a + tt * b; };
        auto alongX = [&](int y, int z) { return blend(t[0], myField(lo[0], y, z), myField(hi[0], y, z)); };
        auto alongY = [&](int z) { return blend(t[1], alongX(lo[1], z), alongX(hi[1], z)); };
        return fpreal(blend(t[2], alongY(lo[2]), alongY(hi[2])));
    }
};

class SIM_RawIndexField : public SIM_RawFieldStandin<int64>
{
};

#endif
