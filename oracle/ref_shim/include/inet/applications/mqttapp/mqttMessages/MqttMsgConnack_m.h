// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgConnack, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgConnack : public cPacket {
    SHIM_PACKET(MqttMsgConnack)
    SHIM_STRING(type, Type)
    SHIM_FIELD(bool, dupFlag, DupFlag)
    SHIM_FIELD(int, qosLevel, QosLevel)
    SHIM_FIELD(bool, retain, Retain)
    SHIM_STRING(messageId, MessageId)
    SHIM_FIELD(bool, sessionPresent, SessionPresent)
    SHIM_FIELD(int, returnCode, ReturnCode)
};

}  // namespace inet
