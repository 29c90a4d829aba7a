// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgSubscribe, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgSubscribe : public cPacket {
    SHIM_PACKET(MqttMsgSubscribe)
    SHIM_STRING(clientID, ClientID)
    SHIM_STRING(topic, Topic)
    SHIM_FIELD(int, qos, Qos)
};

}  // namespace inet
