// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): names resolve through the
// driver's world.
#pragma once
#include "inet/common/INETDefs.h"

namespace inet {

class L3AddressResolver {
  public:
    L3Address resolve(const char *name) {
        L3Address a;
        if (!tryResolve(name, a)) throw cRuntimeError("L3AddressResolver: cannot resolve '%s'", name);
        return a;
    }
    bool tryResolve(const char *name, L3Address &result) {
        result = L3Address(shim::kernel->world->resolve(name));
        return !result.isUnspecified();
    }
};

}  // namespace inet
