// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): FognetMsgTask, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class FognetMsgTask : public cPacket {
    SHIM_PACKET(FognetMsgTask)
    SHIM_STRING(requestID, RequestID)
    SHIM_FIELD(double, requiredTime, RequiredTime)
    SHIM_STRING(clientID, ClientID)
    SHIM_FIELD(int, requiredMIPS, RequiredMIPS)
};

}  // namespace inet
