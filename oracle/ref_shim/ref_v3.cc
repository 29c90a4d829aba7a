// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): ref_v3, the driver that
// runs the reference's own BrokerBaseApp3 and ComputeBrokerApp3 handlers under
// the stand-in kernel and writes down what they do.
//
// Reads commands from standard input, writes one JSON line per command.
//
//   replay N T
//   N lines:  mips dl ul start          (ticks; start = the node's startTime)
//   T lines:  arrive req user_ul user_dl
//     One broker and N nodes are built; the nodes connect and advertise through
//     the reference's own start -> CONNECT -> CONNACK -> ADVERTISEMIPS path; the
//     T publishes (QoS 1, message ids m0, m1, ...) are inserted before the run,
//     in trace order, after the nodes' start timers.
//
//   decide n req
//   n lines:  mips busy                 (busy: the double's bits, hex)
//     n nodes register, each advert carries (mips, busy), one publish asks for
//     req; the line reports the node the task went to.
#include <cinttypes>

#include "inet/applications/mqttapp/BrokerBaseApp3.h"
#include "inet/applications/mqttapp/ComputeBrokerApp3.h"
#include "inet/applications/mqttapp/fognetMessages/FognetMsgAdvertiseMIPS_m.h"
#include "inet/applications/mqttapp/fognetMessages/FognetMsgTask_m.h"
#include "inet/applications/mqttapp/mqttMessages/MqttMsgConnect_m.h"
#include "inet/applications/mqttapp/mqttMessages/MqttMsgPuback_m.h"
#include "inet/applications/mqttapp/mqttMessages/MqttMsgPublish_m.h"
#include "inet/transportlayer/contract/udp/UDPControlInfo_m.h"

using namespace inet;

static const int64 ADDR_BROKER = 1, ADDR_NODE0 = 16, ADDR_USER0 = (int64)1 << 40;
static const int BROKER_PORT = 1883, NODE_PORT = 1884, USER_PORT = 1885;

struct Refused {
    std::string why;
};

static int64 taskOf(const char *id) {
    if (!id || id[0] != 'm') throw Refused{"unexpected message id"};
    return strtoll(id + 1, nullptr, 10);
}

class BrokerProbe : public BrokerBaseApp3 {};

class NodeProbe : public ComputeBrokerApp3 {
  public:
    int index = 0;
    // the task releaseResource() is about to start: the head of the node's queue
    int64 headTask() const { return requests.empty() ? -1 : taskOf(requests[0]->getRequestId()); }
};

struct QEmit {
    int64 raw, tick, task;
    int node;
};
struct UserAck {
    int64 task, tick;
    int status;
};

class V3World : public shim::World {
  public:
    shim::Kernel k;
    BrokerProbe *broker = nullptr;
    std::vector<NodeProbe *> nodes;
    int N = 0;
    int64 T = 0;
    std::vector<int64> mips, dl, ul, start, arrive, req, uu, ud;
    bool decideMode = false;
    int chosen = -1;
    // observations
    std::vector<int> connectOrder;
    std::vector<int64> initAdv, taskNode, taskStatus, taskStart, taskDone;
    std::vector<QEmit> qemits;
    std::vector<UserAck> acks;
    std::vector<int64> delays;
    int64 lastHandshakeAdv = -1;

    bool isNode(int64 a) const { return a >= ADDR_NODE0 && a < ADDR_NODE0 + N; }
    bool isUser(int64 a) const { return a >= ADDR_USER0; }

    int64 resolve(const char *name) override { return strcmp(name, "broker") == 0 ? ADDR_BROKER : 0; }
    cModule *moduleAt(int64 a) override {
        if (a == ADDR_BROKER) return broker;
        if (isNode(a) && !nodes.empty()) return nodes[(size_t)(a - ADDR_NODE0)];
        return nullptr;
    }

    // called by UDPSocket::sendTo at the moment of the call
    int64 latency(cModule *from, int64 dst, cPacket *pk) override {
        int64 src = from->shimAddr;
        if (src == ADDR_BROKER && isNode(dst)) {
            int kk = (int)(dst - ADDR_NODE0);
            if (FognetMsgTask *tsk = dynamic_cast<FognetMsgTask *>(pk)) {
                if (decideMode) chosen = kk;
                else taskNode[(size_t)taskOf(tsk->getRequestID())] = kk;
            }
            return decideMode ? 0 : dl[(size_t)kk];
        }
        if (src == ADDR_BROKER && isUser(dst)) return decideMode ? 0 : ud[(size_t)(dst - ADDR_USER0)];
        if (isNode(src) && dst == ADDR_BROKER) {
            int kk = (int)(src - ADDR_NODE0);
            if (MqttMsgPuback *ack = dynamic_cast<MqttMsgPuback *>(pk)) {
                size_t t = (size_t)taskOf(ack->getMessageID());
                if (ack->getStatus() == 5) {
                    taskStatus[t] = 5;
                    taskStart[t] = k.now;
                } else if (ack->getStatus() == 4)
                    taskStatus[t] = 4;
                else if (ack->getStatus() == 6)
                    taskDone[t] = k.now;
            }
            return ul[(size_t)kk];
        }
        throw Refused{"a packet on a link the world does not have"};
    }

    void onEmit(cModule *m, simsignal_t s, const SimTime &v) override {
        const char *name = cModule::shimSignalName(s);
        if (NodeProbe *nd = dynamic_cast<NodeProbe *>(m)) {
            if (strcmp(name, "queueTime") == 0) {
                int64 t = nd->headTask();
                taskStart[(size_t)t] = k.now;
                qemits.push_back(QEmit{v.raw(), k.now, t, nd->index});
            }
        } else if (m == broker && strcmp(name, "delay") == 0)
            delays.push_back(v.raw());
    }

    void buildBroker() {
        broker = new BrokerProbe;
        broker->shimAddr = ADDR_BROKER;
        broker->shimSetPar("MIPS", cPar(1000.0));
        broker->shimSetPar("algo", cPar(0.0));
        broker->shimSetPar("localPort", cPar((double)BROKER_PORT));
        broker->shimSetPar("interfaceTableModule", cPar(""));
        broker->shimInitialize();
    }

    void deliver(cModule *target, cMessage *msg, int64 src, int port) {
        msg->setKind(UDP_I_DATA);
        msg->setControlInfo(new UDPDataIndication(L3Address(src), port));
        target->handleMessage(msg);
    }
};

static void printVec(const char *name, const std::vector<int64> &v, bool comma = true) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%" PRId64 : "%" PRId64, v[i]);
    printf(comma ? "]," : "]");
}

static void runReplay() {
    V3World w;
    shim::kernel = &w.k;
    w.k.world = &w;
    if (!(std::cin >> w.N >> w.T) || w.N < 1 || w.T < 0) throw Refused{"replay: bad header"};
    size_t N = (size_t)w.N, T = (size_t)w.T;
    w.mips.resize(N), w.dl.resize(N), w.ul.resize(N), w.start.resize(N);
    for (size_t j = 0; j < N; j++) std::cin >> w.mips[j] >> w.dl[j] >> w.ul[j] >> w.start[j];
    w.arrive.resize(T), w.req.resize(T), w.uu.resize(T), w.ud.resize(T);
    for (size_t t = 0; t < T; t++) std::cin >> w.arrive[t] >> w.req[t] >> w.uu[t] >> w.ud[t];
    if (!std::cin) throw Refused{"replay: truncated input"};
    w.initAdv.assign(N, -1);
    w.taskNode.assign(T, -1), w.taskStatus.assign(T, 0), w.taskStart.assign(T, -1), w.taskDone.assign(T, -1);

    // sendInterval above every round trip: the CONNACK always cancels that timer
    int64 rtt = 0;
    for (size_t j = 0; j < N; j++) rtt = std::max(rtt, w.dl[j] + w.ul[j]);
    double sendInterval = (double)rtt * 2e-12 + 1.0;

    w.buildBroker();
    for (size_t j = 0; j < N; j++) {
        NodeProbe *nd = new NodeProbe;
        nd->index = (int)j;
        nd->shimAddr = ADDR_NODE0 + (int64)j;
        double startS = (double)w.start[j] * 1e-12;
        if (w.start[j] < 0 || SimTime(startS).raw() != w.start[j]) throw Refused{"a node start tick no startTime gives"};
        nd->shimSetPar("MIPS", cPar((double)w.mips[j]));
        nd->shimSetPar("localPort", cPar((double)NODE_PORT));
        nd->shimSetPar("destPort", cPar((double)BROKER_PORT));
        nd->shimSetPar("startTime", cPar(startS));
        nd->shimSetPar("stopTime", cPar(-1.0));
        nd->shimSetPar("packetName", cPar("node"));
        nd->shimSetPar("messageLength", cPar(100.0));
        nd->shimSetPar("sendInterval", cPar(sendInterval));
        nd->shimSetPar("localAddress", cPar(""));
        nd->shimSetPar("destAddresses", cPar("broker"));
        nd->shimSetPar("timeToLive", cPar(-1.0));
        nd->shimSetPar("typeOfService", cPar(-1.0));
        nd->shimSetPar("multicastInterface", cPar(""));
        nd->shimSetPar("receiveBroadcast", cPar(0.0));
        nd->shimSetPar("joinLocalMulticastGroups", cPar(0.0));
        nd->shimSetPar("interfaceTableModule", cPar(""));
        w.nodes.push_back(nd);
        nd->shimInitialize();  // handleNodeStart: the START timer goes into the event set
    }
    // the trace, in trace order: its publishes precede dynamic events of the same tick
    for (size_t t = 0; t < T; t++) {
        if (t && w.arrive[t] < w.arrive[t - 1]) throw Refused{"publishes out of order"};
        std::string id = "m" + std::to_string(t);
        MqttMsgPublish *p = new MqttMsgPublish("pub");
        p->setClientID("user");
        p->setMessageID(id.c_str());
        p->setQoS(1);
        p->setMIPSRequired((int)w.req[t]);
        p->setRequiredTime(0.01);
        p->setByteLength(100);
        p->shimSetCreationTime(SimTime::fromRaw(w.arrive[t] - w.uu[t]));
        w.k.insert(shim::Event{w.arrive[t], 0, p, false, w.broker, ADDR_USER0 + (int64)t, ADDR_BROKER, USER_PORT});
    }

    bool aborted = false, firstPublish = true;
    int64 abTick = 0, abTask = -1;
    int abNode = -1;
    std::string abWhat;
    shim::Event e;
    while (w.k.pop(e)) {
        try {
            if (e.self) {
                e.target->handleMessage(e.msg);
            } else if (e.target == w.broker) {
                if (dynamic_cast<MqttMsgConnect *>(e.msg)) w.connectOrder.push_back((int)(e.srcAddr - ADDR_NODE0));
                if (dynamic_cast<FognetMsgAdvertiseMIPS *>(e.msg) && firstPublish) {
                    size_t j = (size_t)(e.srcAddr - ADDR_NODE0);
                    if (w.initAdv[j] < 0) w.initAdv[j] = w.k.now;
                    w.lastHandshakeAdv = w.k.now;
                }
                if (dynamic_cast<MqttMsgPublish *>(e.msg) && firstPublish) {
                    firstPublish = false;
                    for (size_t j = 0; j < N; j++)
                        if (w.initAdv[j] < 0) throw Refused{"the first publish is not later than the last handshake advert"};
                    for (size_t j = 0; j < N; j++)
                        if (w.connectOrder.size() != N || w.connectOrder[j] != (int)j)
                            throw Refused{"CONNECTs did not reach the broker in index order"};
                }
                w.deliver(e.target, e.msg, e.srcAddr, e.srcPort);
            } else if (e.target) {
                w.deliver(e.target, e.msg, e.srcAddr, e.srcPort);
            } else if (w.isUser(e.dstAddr)) {  // the user endpoint: a recorder
                if (MqttMsgPuback *ack = dynamic_cast<MqttMsgPuback *>(e.msg))
                    w.acks.push_back(UserAck{taskOf(ack->getMessageID()), w.k.now, ack->getStatus()});
            }
        } catch (cRuntimeError &err) {
            // nothing above handleMessage catches: the run ends here, as OMNeT++ would end it
            aborted = true;
            abTick = w.k.now;
            abWhat = err.what();
            if (NodeProbe *nd = dynamic_cast<NodeProbe *>(e.target)) {
                abNode = nd->index;
                abTask = nd->headTask();
            }
            break;
        }
    }
    if (T && firstPublish) throw Refused{"no publish ran"};

    printf("{");
    std::vector<int64> co(w.connectOrder.begin(), w.connectOrder.end());
    printVec("connect_order", co);
    printVec("init_adv_tick", w.initAdv);
    printf("\"last_handshake_adv\":%" PRId64 ",", w.lastHandshakeAdv);
    printVec("node", w.taskNode);
    printVec("status", w.taskStatus);
    printVec("start", w.taskStart);
    printVec("done", w.taskDone);
    printVec("delay", w.delays);
    printf("\"qtime\":[");
    for (size_t i = 0; i < w.qemits.size(); i++)
        printf("%s[%" PRId64 ",%" PRId64 ",%d,%" PRId64 "]", i ? "," : "", w.qemits[i].raw, w.qemits[i].tick,
               w.qemits[i].node, w.qemits[i].task);
    printf("],\"user_acks\":[");
    for (size_t i = 0; i < w.acks.size(); i++)
        printf("%s[%" PRId64 ",%d,%" PRId64 "]", i ? "," : "", w.acks[i].task, w.acks[i].status, w.acks[i].tick);
    printf("],\"abort\":");
    if (aborted) {
        std::string what;
        for (char c : abWhat) what += (c == '"' || c == '\\') ? '\'' : c;
        printf("{\"tick\":%" PRId64 ",\"node\":%d,\"task\":%" PRId64 ",\"what\":\"%s\"}", abTick, abNode, abTask,
               what.c_str());
    } else
        printf("null");
    printf("}\n");
}

static void runDecide() {
    V3World w;
    shim::kernel = &w.k;
    w.k.world = &w;
    w.decideMode = true;
    int64 req;
    if (!(std::cin >> w.N >> req) || w.N < 1) throw Refused{"decide: bad header"};
    size_t n = (size_t)w.N;
    std::vector<int64> mips(n);
    std::vector<double> busy(n);
    for (size_t j = 0; j < n; j++) {
        std::string hex;
        std::cin >> mips[j] >> hex;
        uint64_t bits = strtoull(hex.c_str(), nullptr, 16);
        memcpy(&busy[j], &bits, sizeof bits);
    }
    if (!std::cin) throw Refused{"decide: truncated input"};
    if (mips[0] == 0) throw Refused{"MIPS_0 == 0: the reference divides by it"};
    if (mips[0] == -1 && req == INT32_MIN) throw Refused{"INT32_MIN / -1"};
    w.buildBroker();
    std::vector<std::string> ids(n);
    for (size_t j = 0; j < n; j++) {  // registration, BrokerBaseApp3.cc:99-121
        ids[j] = std::to_string(1000 + j);
        MqttMsgConnect *c = new MqttMsgConnect("mqttConnect");
        c->setIsBroker(true);
        c->setClientId(ids[j].c_str());
        w.deliver(w.broker, c, ADDR_NODE0 + (int64)j, NODE_PORT);
    }
    for (size_t j = 0; j < n; j++) {
        FognetMsgAdvertiseMIPS *a = new FognetMsgAdvertiseMIPS("MIPS: ");
        a->setComputeBrokerID(ids[j].c_str());
        a->setMIPS((int)mips[j]);
        a->setBusyTime(busy[j]);
        w.deliver(w.broker, a, ADDR_NODE0 + (int64)j, NODE_PORT);
    }
    MqttMsgPublish *p = new MqttMsgPublish("pub");
    p->setClientID("user");
    p->setMessageID("m0");
    p->setQoS(1);
    p->setMIPSRequired((int)req);
    p->setRequiredTime(0.01);
    w.deliver(w.broker, p, ADDR_USER0, USER_PORT);
    if (w.chosen < 0) throw Refused{"decide: no task left the broker"};
    printf("{\"node\":%d}\n", w.chosen);
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        try {
            if (cmd == "replay") runReplay();
            else if (cmd == "decide") runDecide();
            else throw Refused{"unknown command " + cmd};
        } catch (Refused &r) {
            fprintf(stderr, "ref_v3: refused: %s\n", r.why.c_str());
            return 2;
        } catch (std::exception &x) {
            fprintf(stderr, "ref_v3: %s\n", x.what());
            return 3;
        }
        fflush(stdout);
    }
    return 0;
}
