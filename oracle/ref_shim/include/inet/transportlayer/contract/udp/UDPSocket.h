// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): stand-in for INET 3.3's
// UDPSocket.  sendTo() inserts, at the moment of the call, one delivery event at
// now + latency(link) into the future-event set; the options
// the v3 modules set are accepted and ignored.
#pragma once
#include "inet/common/INETDefs.h"

namespace inet {

typedef std::vector<int> MulticastGroupList;

class UDPSocket {
    cModule *owner = nullptr;
    int localPort = -1;
  public:
    void setOutputGate(cGate *g) { owner = g->owner; }
    void bind(int port) { localPort = port; }
    void bind(L3Address, int port) { localPort = port; }
    void setTimeToLive(int) {}
    void setTypeOfService(int) {}
    void setMulticastOutputInterface(int) {}
    void setBroadcast(bool) {}
    void joinLocalMulticastGroups(const MulticastGroupList &) {}
    void close() {}
    void sendTo(cPacket *pk, L3Address destAddr, int destPort);  // kernel.cc
};

}  // namespace inet
