// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): stand-in for INET 3.3's
// common definitions, as far as the reference's v3 modules use them.
#pragma once
#include <omnetpp.h>

#define INET_API

namespace inet {

// init stages in INET's order; the v3 modules use LOCAL and LAST and return NUM_INIT_STAGES
enum { INITSTAGE_LOCAL = 0, INITSTAGE_APPLICATION_LAYER = 1, INITSTAGE_LAST = 2, NUM_INIT_STAGES = 3 };

class L3Address {
    int64 a = 0;
  public:
    L3Address() {}
    explicit L3Address(int64 x) : a(x) {}
    int64 shimRaw() const { return a; }
    bool isUnspecified() const { return a == 0; }
    bool isLinkLocal() const { return false; }
    friend bool operator==(const L3Address &x, const L3Address &y) { return x.a == y.a; }
    friend bool operator!=(const L3Address &x, const L3Address &y) { return x.a != y.a; }
};

}  // namespace inet
