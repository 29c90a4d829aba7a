// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): the one module the v3
// modules look up is the interface table, for multicast groups nobody joins.
#pragma once
#include "inet/common/INETDefs.h"
#include "inet/transportlayer/contract/udp/UDPSocket.h"

namespace inet {

class InterfaceEntry {
  public:
    int getInterfaceId() const { return 0; }
};

class IInterfaceTable {
  public:
    MulticastGroupList collectMulticastGroups() { return MulticastGroupList(); }
    InterfaceEntry *getInterfaceByName(const char *) { return nullptr; }
};

template <class T>
T *getModuleFromPar(cPar &, cModule *) {
    static T instance;
    return &instance;
}

}  // namespace inet
