/* Stand-in for the HDK's SIM_RawIndexField.h: the class lives with SIM_RawField.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_RAWINDEXFIELD_H
#define REFSTANDIN_SIM_RAWINDEXFIELD_H

#include <SIM/SIM_RawField.h>

#endif
