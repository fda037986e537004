/* Stand-in for the HDK's parameter-description types (PRM_Name, PRM_Default, PRM_Template): plain records
 * that keep what they are given, so that the plugin's parameter table is built and can be read back; nothing
 * interprets it.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_PRM_INCLUDE_H
#define REFSTANDIN_PRM_INCLUDE_H

#include <SYS/SYS_Types.h>

enum PRM_Type
{
    PRM_LIST_TERMINATOR,
    PRM_STRING,
    PRM_TOGGLE,
    PRM_FLT,
    PRM_INT
};

class PRM_Name
{
public:
    PRM_Name(const char *token = nullptr, const char *label = nullptr) : myToken(token), myLabel(label) {}
    const char *getToken() const { return myToken; }
    const char *getLabel() const { return myLabel; }

private:
    const char *myToken, *myLabel;
};

class PRM_Default
{
public:
    PRM_Default(fpreal value = 0, const char *string = nullptr) : myValue(value), myString(string) {}
    fpreal getFloat() const { return myValue; }
    const char *getString() const { return myString; }

private:
    fpreal myValue;
    const char *myString;
};

class PRM_Template
{
public:
    PRM_Template() = default;
    PRM_Template(PRM_Type type, int size, PRM_Name *name, PRM_Default *defaults = nullptr) : myType(type), mySize(size), myName(name), myDefaults(defaults)
    {
    }
    PRM_Type getType() const { return myType; }
    int getVectorSize() const { return mySize; }
    const PRM_Name *getNamePtr() const { return myName; }
    const PRM_Default *getFactoryDefaults() const { return myDefaults; }

private:
    PRM_Type myType = PRM_LIST_TERMINATOR;
    int mySize = 0;
    PRM_Name *myName = nullptr;
    PRM_Default *myDefaults = nullptr;
};

#endif
