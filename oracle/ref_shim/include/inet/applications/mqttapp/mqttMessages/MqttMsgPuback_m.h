// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgPuback, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgPuback : public cPacket {
    SHIM_PACKET(MqttMsgPuback)
    SHIM_FIELD(int, qos, Qos)
    SHIM_STRING(messageID, MessageID)
    SHIM_FIELD(int, status, Status)
};

}  // namespace inet
