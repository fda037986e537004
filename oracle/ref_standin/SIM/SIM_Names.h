/* Stand-in for the HDK's SIM_Names.h: the one option name the plugin takes from it.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_NAMES_H
#define REFSTANDIN_SIM_NAMES_H

#define SIM_NAME_TOLERANCE "tolerance"

#endif
