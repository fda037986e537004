/* Stand-in for the HDK's GAS_SubSolver: the base class of the plugin.  Options are a table of numbers that the
 * driver sets (setOptionStandin) and the GET_DATA_FUNC_* accessors read; an option that was never set throws.
 * get[Const]{Scalar,Vector}Field(obj, name) return the object's field of that name, or nullptr.  addError
 * keeps the messages for the driver.  DECLARE_DATAFACTORY names BaseClass and classname() and, as in the HDK,
 * makes the description reachable for IMPLEMENT_DATAFACTORY, which builds it once.  See SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_GAS_SUBSOLVER_H
#define REFSTANDIN_GAS_SUBSOLVER_H

#include <map>
#include <string>
#include <vector>

#include <SIM/SIM_DopDescription.h>
#include <SIM/SIM_Names.h>
#include <SIM/SIM_Object.h>

#define GAS_API

enum SIM_ErrorCodeStandin
{
    SIM_MESSAGE
};
enum UT_ErrorSeverity
{
    UT_ERROR_NONE,
    UT_ERROR_MESSAGE,
    UT_ERROR_WARNING,
    UT_ERROR_ABORT,
    UT_ERROR_FATAL
};

class GAS_SubSolver
{
public:
    void setOptionStandin(const std::string &name, fpreal value) { myOptions[name] = value; }
    fpreal getOptionStandin(const std::string &name) const
    {
        auto it = myOptions.find(name);
        if (it == myOptions.end()) throw refstandin::AssertionFailed("stand-in GAS_SubSolver: option '" + name + "' was never set");
        return it->second;
    }
    const std::vector<std::string> &errorsStandin() const { return myErrors; }
    // the public door to the protected callback, as the DOP network would call it
    bool solveStandin(SIM_Engine &engine, SIM_Object *obj, SIM_Time time, SIM_Time timestep) { return solveGasSubclass(engine, obj, time, timestep); }

protected:
    explicit GAS_SubSolver(const SIM_DataFactory *) {}
    virtual ~GAS_SubSolver() {}

    virtual bool solveGasSubclass(SIM_Engine &engine, SIM_Object *obj, SIM_Time time, SIM_Time timestep) = 0;

    SIM_ScalarField *getScalarField(SIM_Object *obj, const char *name, bool = false) const { return obj->findScalarFieldStandin(name); }
    const SIM_ScalarField *getConstScalarField(SIM_Object *obj, const char *name) const { return obj->findScalarFieldStandin(name); }
    SIM_VectorField *getVectorField(SIM_Object *obj, const char *name, bool = false) const { return obj->findVectorFieldStandin(name); }
    const SIM_VectorField *getConstVectorField(SIM_Object *obj, const char *name) const { return obj->findVectorFieldStandin(name); }

    void addError(const SIM_Object *, int, const char *text, UT_ErrorSeverity) const { myErrors.push_back(text); }

    static void setGasDescription(SIM_DopDescription &) {}

private:
    std::map<std::string, fpreal> myOptions;
    mutable std::vector<std::string> myErrors;
};

#define DECLARE_STANDARD_GETCASTTOTYPE() static_assert(true, "")

#define DECLARE_DATAFACTORY(Class, Base, Description, DopDescription)                  \
public:                                                                                \
    using BaseClass = Base;                                                            \
    static const char *classname() { return #Class; }                                  \
    static const SIM_DopDescription *dataFactoryDescriptionStandin() { return DopDescription; } \
                                                                                       \
private:                                                                               \
    static_assert(true, "")

#define IMPLEMENT_DATAFACTORY(Class) ((void)Class::dataFactoryDescriptionStandin())

#endif
