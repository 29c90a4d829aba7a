// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): FognetMsgTaskAck, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class FognetMsgTaskAck : public cPacket {
    SHIM_PACKET(FognetMsgTaskAck)
    SHIM_STRING(requestID, RequestID)
    SHIM_FIELD(int, status, Status)
};

}  // namespace inet
