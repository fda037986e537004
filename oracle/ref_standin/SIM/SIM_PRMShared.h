/* Stand-in for the HDK's SIM_PRMShared.h: the shared parameter defaults the plugin uses.  See
 * SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_PRMSHARED_H
#define REFSTANDIN_SIM_PRMSHARED_H

#include <PRM/PRM_Include.h>
#include <SIM/SIM_Names.h>

static PRM_Default PRMzeroDefaults[] = {PRM_Default(0), PRM_Default(0), PRM_Default(0), PRM_Default(0)};
static PRM_Default PRMoneDefaults[] = {PRM_Default(1), PRM_Default(1), PRM_Default(1), PRM_Default(1)};

#endif
