/* Stand-in for the HDK's GAS_Utils.h: the parameter names the plugin reads its field names from, and the
 * accessor macros.  In the HDK a name such as GAS_NAME_SURFACE is a parameter whose string value names the
 * object's field; here the field is looked up under the parameter name itself (GAS/GAS_SubSolver.h).
 * GET_DATA_FUNC_{F,I,B}(name, Stem) declares getStem(), which reads option `name` of the solver as a float,
 * an integer or a toggle.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_GAS_UTILS_H
#define REFSTANDIN_GAS_UTILS_H

#define GAS_NAME_SURFACE "surface"
#define GAS_NAME_VELOCITY "velocity"
#define GAS_NAME_COLLISION "collision"
#define GAS_NAME_COLLISIONVELOCITY "collisionvelocity"
#define GAS_NAME_PRESSURE "pressure"
#define GAS_NAME_DENSITY "density"

#define GET_DATA_FUNC_F(name, Stem) \
    fpreal get##Stem() const { return getOptionStandin(name); }
#define GET_DATA_FUNC_I(name, Stem) \
    int get##Stem() const { return int(getOptionStandin(name)); }
#define GET_DATA_FUNC_B(name, Stem) \
    bool get##Stem() const { return getOptionStandin(name) != 0; }

#endif
