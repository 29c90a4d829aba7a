// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md).
//
// A stand-in for the part of OMNeT++ 4.6 that the reference's two hot-path
// translation units (BrokerBaseApp3.cc, ComputeBrokerApp3.cc) touch, written
// from the signatures those files use.  It exists so that the reference's own
// handlers can be compiled in place and run event by event; it is not OMNeT++
// and holds no line of it or of the reference.
//
// What is modelled, and how, is the project's written rule (fognet_hip.h,
// "Reference signal values"):
//   simtime_t   raw int64 at 1e-12 s; SimTime(double d) = toInt64(1e12 * d);
//               SimTime * double = toInt64(t * d); toInt64(x) = floor(x + 0.5),
//               a cRuntimeError outside int64; dbl() = t * 1e-12.  Compiled with
//               -ffp-contract=off so each operation rounds on its own.
//   FES         ordered by (tick, insertion sequence); scheduleAt() on a
//               scheduled message throws; cancelEvent() removes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <exception>
#include <iostream>
#include <map>
#include <queue>
#include <sstream>
#include <string>
#include <typeinfo>
#include <vector>

typedef int64_t int64;
using std::endl;

class cRuntimeError : public std::exception {
    std::string msg;
  public:
    cRuntimeError(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        msg = buf;
    }
    const char *what() const noexcept override { return msg.c_str(); }
};

// ---- simulation time

class SimTime {
    int64 t = 0;
  public:
    static int64 toInt64(double x) {
        double f = std::floor(x + 0.5);
        if (!(std::fabs(f) < 9223372036854775808.0))
            throw cRuntimeError("SimTime: %g does not fit into a 64-bit simulation time", x);
        return (int64)f;
    }
    SimTime() {}
    SimTime(double d) : t(toInt64(1e12 * d)) {}  // non-explicit, as the reference's expressions need
    static SimTime fromRaw(int64 raw) {
        SimTime s;
        s.t = raw;
        return s;
    }
    int64 raw() const { return t; }
    double dbl() const { return (double)t * 1e-12; }
    friend SimTime operator+(const SimTime &a, const SimTime &b) { return fromRaw(a.t + b.t); }
    friend SimTime operator-(const SimTime &a, const SimTime &b) { return fromRaw(a.t - b.t); }
    friend SimTime operator*(const SimTime &a, double d) { return fromRaw(toInt64((double)a.t * d)); }
    friend SimTime operator*(double d, const SimTime &a) { return fromRaw(toInt64((double)a.t * d)); }
    friend bool operator<(const SimTime &a, const SimTime &b) { return a.t < b.t; }
    friend bool operator>(const SimTime &a, const SimTime &b) { return a.t > b.t; }
    friend bool operator<=(const SimTime &a, const SimTime &b) { return a.t <= b.t; }
    friend bool operator>=(const SimTime &a, const SimTime &b) { return a.t >= b.t; }
    friend bool operator==(const SimTime &a, const SimTime &b) { return a.t == b.t; }
    friend bool operator!=(const SimTime &a, const SimTime &b) { return a.t != b.t; }
};
typedef SimTime simtime_t;
#define SIMTIME_ZERO SimTime()
inline std::ostream &operator<<(std::ostream &o, const SimTime &s) { return o << s.dbl(); }

SimTime simTime();  // the kernel's clock (kernel.cc)

// ---- objects and messages

class cObject {
  public:
    virtual ~cObject() {}
    virtual const char *getClassName() const { return typeid(*this).name(); }
};

class cModule;

class cMessage : public cObject {
    std::string name;
    short kind = 0;
    SimTime created = simTime();
    cObject *ctrl = nullptr;
  public:
    // kernel bookkeeping (kernel.cc)
    bool shimScheduled = false, shimSelf = false;
    uint64_t shimSeq = 0;

    explicit cMessage(const char *n = nullptr, short k = 0) : name(n ? n : ""), kind(k) {}
    cMessage(const cMessage &o) : cObject(), name(o.name), kind(o.kind), created(o.created) {}
    virtual cMessage *dup() const { return new cMessage(*this); }
    const char *getName() const { return name.c_str(); }
    void setName(const char *n) { name = n ? n : ""; }
    short getKind() const { return kind; }
    void setKind(short k) { kind = k; }
    bool isSelfMessage() const { return shimSelf; }
    bool isScheduled() const { return shimScheduled; }
    SimTime getCreationTime() const { return created; }
    void setControlInfo(cObject *c) { ctrl = c; }
    cObject *getControlInfo() const { return ctrl; }
    cObject *removeControlInfo() {
        cObject *c = ctrl;
        ctrl = nullptr;
        return c;
    }
    void shimSetCreationTime(SimTime t) { created = t; }  // the driver's sender clock
};

class cPacket : public cMessage {
    int64 byteLength = 0;
  public:
    explicit cPacket(const char *n = nullptr, short k = 0) : cMessage(n, k) {}
    cPacket *dup() const override { return new cPacket(*this); }
    int64 getByteLength() const { return byteLength; }
    void setByteLength(int64 l) { byteLength = l; }
};
#define PK(msg) check_and_cast<cPacket *>(msg)

template <class T, class P>
T check_and_cast(P *p) {
    if (!p) throw cRuntimeError("check_and_cast(): cannot cast nullptr");
    T r = dynamic_cast<T>(p);
    if (!r) throw cRuntimeError("check_and_cast(): cannot cast (%s)", p->getClassName());
    return r;
}

// ---- parameters, gates, display strings

class cPar {
    double num = 0;
    std::string str;
  public:
    cPar() {}
    cPar(double v) : num(v) {}
    cPar(const char *s) : str(s) {}
    operator bool() const { return num != 0; }
    operator int() const { return (int)num; }
    operator long() const { return (long)num; }
    operator double() const { return num; }
    operator const char *() const { return str.c_str(); }
    bool boolValue() const { return num != 0; }
    long longValue() const { return (long)num; }
    double doubleValue() const { return num; }
    const char *stringValue() const { return str.c_str(); }
};

class cGate {
  public:
    cModule *owner = nullptr;
};

class cDisplayString {
  public:
    void setTagArg(const char *, int, const char *) {}
};

class cStringTokenizer {
    std::vector<std::string> tok;
    size_t next = 0;
  public:
    explicit cStringTokenizer(const char *s) {
        std::istringstream in(s ? s : "");
        std::string w;
        while (in >> w) tok.push_back(w);
    }
    const char *nextToken() { return next < tok.size() ? tok[next++].c_str() : nullptr; }
};

// ---- modules

typedef int simsignal_t;

class cModule : public cObject {
    std::map<std::string, cPar> pars;
    cGate outGate;
    cDisplayString ds;
    int id;
  public:
    int64 shimAddr = 0;  // the address the stand-in network knows this module by

    cModule();
    static simsignal_t registerSignal(const char *name);
    static const char *shimSignalName(simsignal_t s);
    void shimSetPar(const char *name, const cPar &v) { pars[name] = v; }
    cPar &par(const char *name) {
        auto it = pars.find(name);
        if (it == pars.end()) throw cRuntimeError("unknown parameter '%s'", name);
        return it->second;
    }
    int getId() const { return id; }
    bool hasGUI() const { return false; }
    cDisplayString &getDisplayString() { return ds; }
    cGate *gate(const char *) {
        outGate.owner = this;
        return &outGate;
    }
    int intrand(int) { return 0; }
    void emit(simsignal_t s, const SimTime &v);
    void emit(simsignal_t, cObject *) {}
    void recordScalar(const char *, double) {}
    void scheduleAt(SimTime t, cMessage *msg);
    cMessage *cancelEvent(cMessage *msg);
    void cancelAndDelete(cMessage *msg) {
        if (msg) cancelEvent(msg);  // never freed: see the README
    }
    virtual void handleMessage(cMessage *msg) = 0;
};
typedef cModule cSimpleModule;

#define Define_Module(CLASS) static int shim_define_module_##CLASS __attribute__((unused)) = 0
#define WATCH(x) ((void)0)
#define ASSERT(expr) ((void)((expr) ? 0 : (throw cRuntimeError("ASSERT: condition %s false", #expr), 0)))

std::ostream &shimNullStream();
#define EV shimNullStream()
#define EV_WARN shimNullStream()
#define EV_ERROR shimNullStream()

// ---- the stand-in kernel (kernel.cc): clock, future-event set, hooks to the driver

namespace shim {

struct Event {
    int64 tick;
    uint64_t seq;
    cMessage *msg;
    bool self;
    cModule *target;        // self-messages and deliveries to a module; nullptr: an address without one
    int64 srcAddr, dstAddr; // deliveries
    int srcPort;
};

// What the driver supplies: link latencies and its observations.
class World {
  public:
    virtual ~World() {}
    // one-way latency in ticks from the module `from` to the address `dst`; called by sendTo
    virtual int64 latency(cModule *from, int64 dst, cPacket *pk) = 0;
    virtual cModule *moduleAt(int64 addr) = 0;
    virtual int64 resolve(const char *name) = 0;
    virtual void onEmit(cModule *, simsignal_t, const SimTime &) {}
};

class Kernel {
    struct Later {
        bool operator()(const Event &a, const Event &b) const {
            return a.tick != b.tick ? a.tick > b.tick : a.seq > b.seq;
        }
    };
    std::priority_queue<Event, std::vector<Event>, Later> fes;
    uint64_t seq = 0;
  public:
    int64 now = 0;
    World *world = nullptr;
    void insert(Event e) {
        e.seq = seq++;
        if (e.self) e.msg->shimSeq = e.seq;
        fes.push(e);
    }
    // next live event (cancelled self-messages are dropped); false when the set is empty
    bool pop(Event &e) {
        while (!fes.empty()) {
            e = fes.top();
            fes.pop();
            if (e.self && !(e.msg->shimScheduled && e.msg->shimSeq == e.seq)) continue;
            if (e.self) e.msg->shimScheduled = false;
            now = e.tick;
            return true;
        }
        return false;
    }
};

extern Kernel *kernel;  // the world being run

}  // namespace shim
