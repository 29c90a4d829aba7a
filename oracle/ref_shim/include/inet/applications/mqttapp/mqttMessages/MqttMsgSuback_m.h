// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgSuback, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgSuback : public cPacket {
    SHIM_PACKET(MqttMsgSuback)
    SHIM_FIELD(int, grantedQosLevels, GrantedQosLevels)
};

}  // namespace inet
