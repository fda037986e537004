/* Stand-in for the HDK's SIM_DopDescription: keeps the names and the parameter table it is given.  See
 * SIM/SIM_RawField.h. */
#ifndef REFSTANDIN_SIM_DOPDESCRIPTION_H
#define REFSTANDIN_SIM_DOPDESCRIPTION_H

#include <PRM/PRM_Include.h>

class SIM_DopDescription
{
public:
    SIM_DopDescription(bool createNode, const char *nodeName, const char *nodeLabel, const char *dataName, const char *dataTypeName,
                       const PRM_Template *templates)
        : myCreateNode(createNode), myNodeName(nodeName), myNodeLabel(nodeLabel), myDataName(dataName), myDataTypeName(dataTypeName),
          myTemplates(templates)
    {
    }
    bool getCreateNode() const { return myCreateNode; }
    const char *getNodeName() const { return myNodeName; }
    const char *getNodeLabel() const { return myNodeLabel; }
    const char *getDataName() const { return myDataName; }
    const char *getDataTypeName() const { return myDataTypeName; }
    const PRM_Template *getTemplates() const { return myTemplates; }

private:
    bool myCreateNode;
    const char *myNodeName, *myNodeLabel, *myDataName, *myDataTypeName;
    const PRM_Template *myTemplates;
};

#endif
