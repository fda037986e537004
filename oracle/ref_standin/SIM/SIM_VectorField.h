/* Stand-in for the HDK's SIM_VectorField: three raw fields over one voxel grid, either all centre-sampled or
 * face-sampled (field a on the faces of axis a).  getField hands out the raw field itself, from a const object
 * too, as the HDK does.  isAligned compares sampling, voxel counts, origin and size; matchField re-creates the
 * fields (zero-filled) only where they are not aligned already; pubHandleModification counts its calls.  See
 * SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_VECTORFIELD_H
#define REFSTANDIN_SIM_VECTORFIELD_H

#include <SIM/SIM_RawField.h>

class SIM_VectorField
{
public:
    // driver side: a grid of xres x yres x zres voxels at `orig` spanning `size`
    void initStandin(bool faceSampled, const UT_Vector3 &orig, const UT_Vector3 &size, int xres, int yres, int zres)
    {
        const SIM_FieldSample faces[3] = {SIM_SAMPLE_FACEX, SIM_SAMPLE_FACEY, SIM_SAMPLE_FACEZ};
        for (int a = 0; a < 3; ++a) myFields[a].init(faceSampled ? faces[a] : SIM_SAMPLE_CENTER, orig, size, xres, yres, zres);
    }

    SIM_RawField *getField(int axis) const { return const_cast<SIM_RawField *>(&myFields[axis]); }
    SIM_RawField *getXField() const { return getField(0); }
    SIM_RawField *getYField() const { return getField(1); }
    SIM_RawField *getZField() const { return getField(2); }

    bool isFaceSampled() const
    {
        return myFields[0].getSample() == SIM_SAMPLE_FACEX && myFields[1].getSample() == SIM_SAMPLE_FACEY && myFields[2].getSample() == SIM_SAMPLE_FACEZ;
    }
    bool isAligned(const SIM_VectorField *o) const
    {
        return myFields[0].isAligned(&o->myFields[0]) && myFields[1].isAligned(&o->myFields[1]) && myFields[2].isAligned(&o->myFields[2]);
    }
    bool isAligned(const SIM_RawField *o) const { return myFields[0].isAligned(o) && myFields[1].isAligned(o) && myFields[2].isAligned(o); }

    UT_Vector3I getTotalVoxelRes() const { return myFields[0].getVoxelRes(); }
    const UT_Vector3 &getOrig() const { return myFields[0].getOrig(); }
    const UT_Vector3 &getSize() const { return myFields[0].getSize(); }
    const UT_Vector3 &getVoxelSize() const { return myFields[0].getVoxelSize(); }

    void matchField(const SIM_VectorField *o)
    {
        if (isAligned(o)) return;
        for (int a = 0; a < 3; ++a) myFields[a].match(o->myFields[a]);
    }
    void pubHandleModification() { ++myModifications; }
    int modificationsStandin() const { return myModifications; }

private:
    SIM_RawField myFields[3];
    int myModifications = 0;
};

#endif
