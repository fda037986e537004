/* Stand-in for the HDK's SIM_Object, SIM_Engine, SIM_Time and SIM_DataFactory: an object is a table of named
 * scalar and vector fields that the driver fills; engine and factory carry nothing; a time is a number.  See
 * SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_OBJECT_H
#define REFSTANDIN_SIM_OBJECT_H

#include <map>
#include <string>

#include <SIM/SIM_ScalarField.h>
#include <SIM/SIM_VectorField.h>

using SIM_Time = fpreal;

class SIM_Engine
{
};

class SIM_DataFactory
{
};

class SIM_Object
{
public:
    SIM_ScalarField &addScalarFieldStandin(const std::string &name) { return myScalars[name]; }
    SIM_VectorField &addVectorFieldStandin(const std::string &name) { return myVectors[name]; }
    SIM_ScalarField *findScalarFieldStandin(const std::string &name)
    {
        auto it = myScalars.find(name);
        return it == myScalars.end() ? nullptr : &it->second;
    }
    SIM_VectorField *findVectorFieldStandin(const std::string &name)
    {
        auto it = myVectors.find(name);
        return it == myVectors.end() ? nullptr : &it->second;
    }

private:
    std::map<std::string, SIM_ScalarField> myScalars;
    std::map<std::string, SIM_VectorField> myVectors;
};

#endif
