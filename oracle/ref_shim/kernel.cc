// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): the stand-in kernel
// behind include/omnetpp.h -- the clock, scheduleAt / cancelEvent on the
// future-event set, signal registration and UDPSocket::sendTo.
#include <omnetpp.h>

#include "inet/transportlayer/contract/udp/UDPSocket.h"

namespace shim {
Kernel *kernel = nullptr;
}

SimTime simTime() { return SimTime::fromRaw(shim::kernel ? shim::kernel->now : 0); }

std::ostream &shimNullStream() {
    static std::ostream null(nullptr);  // no buffer: every write is dropped
    return null;
}

static std::vector<std::string> &signalNames() {
    static std::vector<std::string> names;
    return names;
}

simsignal_t cModule::registerSignal(const char *name) {
    auto &n = signalNames();
    for (size_t i = 0; i < n.size(); i++)
        if (n[i] == name) return (simsignal_t)i;
    n.push_back(name);
    return (simsignal_t)n.size() - 1;
}

const char *cModule::shimSignalName(simsignal_t s) { return signalNames()[(size_t)s].c_str(); }

cModule::cModule() {
    static int nextId = 2;  // module ids are unique for the life of the process
    id = nextId++;
}

void cModule::emit(simsignal_t s, const SimTime &v) { shim::kernel->world->onEmit(this, s, v); }

void cModule::scheduleAt(SimTime t, cMessage *msg) {
    if (!msg) throw cRuntimeError("scheduleAt(): message pointer is nullptr");
    if (msg->shimScheduled)
        throw cRuntimeError("scheduleAt(): message (%s)%s is currently scheduled, use cancelEvent() before rescheduling",
                            msg->getClassName(), msg->getName());
    if (t.raw() < shim::kernel->now) throw cRuntimeError("scheduleAt(): cannot schedule message to the past");
    msg->shimScheduled = true;
    msg->shimSelf = true;
    shim::kernel->insert(shim::Event{t.raw(), 0, msg, true, this, 0, 0, 0});
}

cMessage *cModule::cancelEvent(cMessage *msg) {
    if (msg) msg->shimScheduled = false;  // Kernel::pop drops the stale entry
    return msg;
}

namespace inet {

void UDPSocket::sendTo(cPacket *pk, L3Address destAddr, int destPort) {
    if (!owner) throw cRuntimeError("UDPSocket::sendTo(): no output gate");
    shim::Kernel *k = shim::kernel;
    int64 dst = destAddr.shimRaw();
    pk->shimSelf = false;
    k->insert(shim::Event{k->now + k->world->latency(owner, dst, pk), 0, pk, false, k->world->moduleAt(dst),
                          owner->shimAddr, dst, localPort});
}

}  // namespace inet
