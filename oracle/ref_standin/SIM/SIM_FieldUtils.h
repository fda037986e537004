/* Stand-in for the index maps of the HDK's SIM::FieldUtils (cell-centred grid, face grids with one more
 * entry along their axis): face f of axis a lies between cells f - e_a and f; and for its getFieldValue /
 * setFieldValue on voxel arrays and raw fields (a raw field's sample is handed out as fpreal32, an index
 * field's as exint).  See SYS/SYS_Types.h. */
#ifndef REFSTANDIN_SIM_FIELDUTILS_H
#define REFSTANDIN_SIM_FIELDUTILS_H

#include <SIM/SIM_RawField.h>
#include <UT/UT_Vector3.h>
#include <UT/UT_VoxelArray.h>

namespace SIM
{
namespace FieldUtils
{
    // the neighbour of `cell` along `axis`: direction 0 = minus side, 1 = plus side
    inline UT_Vector3I cellToCellMap(const UT_Vector3I &cell, int axis, int direction)
    {
        UT_Vector3I adjacent(cell);
        adjacent[axis] += direction == 0 ? -1 : 1;
        return adjacent;
    }
    // the face of `cell` on that side, as an index into the axis' face grid
    inline UT_Vector3I cellToFaceMap(const UT_Vector3I &cell, int axis, int direction)
    {
        UT_Vector3I face(cell);
        if (direction == 1) ++face[axis];
        return face;
    }
    // the cell on that side of `face`
    inline UT_Vector3I faceToCellMap(const UT_Vector3I &face, int axis, int direction)
    {
        UT_Vector3I cell(face);
        if (direction == 0) --cell[axis];
        return cell;
    }
    // every voxel of the box [start, end), x fastest
    template <typename Functor>
    inline void forEachVoxelRange(const UT_Vector3I &start, const UT_Vector3I &end, const Functor &functor)
    {
        UT_Vector3I cell;
        for (cell[2] = start[2]; cell[2] < end[2]; ++cell[2])
            for (cell[1] = start[1]; cell[1] < end[1]; ++cell[1])
                for (cell[0] = start[0]; cell[0] < end[0]; ++cell[0]) functor(cell);
    }
    template <typename T>
    inline T getFieldValue(const UT_VoxelArray<T> &field, const UT_Vector3I &cell)
    {
        return field(cell);
    }
    template <typename T>
    inline void setFieldValue(UT_VoxelArray<T> &field, const UT_Vector3I &cell, T value)
    {
        field.setValue(cell, value);
    }
    // raw fields: the sample at an index of field(); a value written is rounded to the field's storage type
    inline fpreal32 getFieldValue(const SIM_RawField &field, const UT_Vector3I &cell) { return (*field.field())(cell); }
    inline exint getFieldValue(const SIM_RawIndexField &field, const UT_Vector3I &cell) { return (*field.field())(cell); }
    inline void setFieldValue(SIM_RawField &field, const UT_Vector3I &cell, fpreal32 value) { field.fieldNC()->setValue(cell, value); }
    inline void setFieldValue(SIM_RawIndexField &field, const UT_Vector3I &cell, exint value) { field.fieldNC()->setValue(cell, value); }
} // namespace FieldUtils
} // namespace SIM

#endif
