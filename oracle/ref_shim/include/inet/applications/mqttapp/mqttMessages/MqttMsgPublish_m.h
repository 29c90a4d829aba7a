// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgPublish, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgPublish : public cPacket {
    SHIM_PACKET(MqttMsgPublish)
    SHIM_STRING(clientID, ClientID)
    SHIM_STRING(topic, Topic)
    SHIM_STRING(mqttMessage, MqttMessage)
    SHIM_FIELD(int, qoS, QoS)
    SHIM_FIELD(int, MIPSRequired, MIPSRequired)
    SHIM_FIELD(double, requiredTime, RequiredTime)
    SHIM_STRING(messageID, MessageID)
};

}  // namespace inet
