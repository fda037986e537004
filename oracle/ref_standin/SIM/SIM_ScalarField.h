/* Stand-in for the HDK's SIM_ScalarField: one raw field.  getField hands out the raw field itself, from a const
 * object too; matchField re-creates the field (zero-filled) only where it is not aligned with the other one
 * already, so a pressure field that matches keeps its values for the warm start; pubHandleModification counts
 * its calls.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_SCALARFIELD_H
#define REFSTANDIN_SIM_SCALARFIELD_H

#include <SIM/SIM_RawField.h>

class SIM_ScalarField
{
public:
    void initStandin(SIM_FieldSample sample, const UT_Vector3 &orig, const UT_Vector3 &size, int xres, int yres, int zres)
    {
        myField.init(sample, orig, size, xres, yres, zres);
    }

    SIM_RawField *getField() const { return const_cast<SIM_RawField *>(&myField); }
    bool isAligned(const SIM_ScalarField *o) const { return myField.isAligned(&o->myField); }
    bool isAligned(const SIM_RawField *o) const { return myField.isAligned(o); }
    UT_Vector3I getTotalVoxelRes() const { return myField.getVoxelRes(); }
    const UT_Vector3 &getOrig() const { return myField.getOrig(); }
    const UT_Vector3 &getSize() const { return myField.getSize(); }
    const UT_Vector3 &getVoxelSize() const { return myField.getVoxelSize(); }

    void matchField(const SIM_ScalarField *o)
    {
        if (!isAligned(o)) myField.match(o->myField);
    }
    void pubHandleModification() { ++myModifications; }
    int modificationsStandin() const { return myModifications; }

private:
    SIM_RawField myField;
    int myModifications = 0;
};

#endif
