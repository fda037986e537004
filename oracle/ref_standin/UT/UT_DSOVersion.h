/* Stand-in for the HDK's UT_DSOVersion.h, which stamps a plugin with the version it was built for: nothing to
 * stamp here.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_UT_DSOVERSION_H
#define REFSTANDIN_UT_DSOVERSION_H
#endif
