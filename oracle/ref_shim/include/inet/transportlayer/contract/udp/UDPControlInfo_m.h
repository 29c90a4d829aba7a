// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): the control info INET 3.3's
// UDP attaches to a received datagram, and the message kinds of its indications.
#pragma once
#include "inet/common/INETDefs.h"

namespace inet {

enum UDPStatusInd { UDP_I_DATA = 0, UDP_I_ERROR = 1 };

class UDPDataIndication : public cObject {
    L3Address srcAddr;
    int srcPort = 0;
  public:
    UDPDataIndication(L3Address a, int p) : srcAddr(a), srcPort(p) {}
    L3Address getSrcAddr() const { return srcAddr; }
    int getSrcPort() const { return srcPort; }
};

}  // namespace inet
