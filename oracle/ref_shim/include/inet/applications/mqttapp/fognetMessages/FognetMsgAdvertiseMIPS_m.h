// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): FognetMsgAdvertiseMIPS, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class FognetMsgAdvertiseMIPS : public cPacket {
    SHIM_PACKET(FognetMsgAdvertiseMIPS)
    SHIM_FIELD(int, MIPS, MIPS)
    SHIM_STRING(computeBrokerID, ComputeBrokerID)
    SHIM_FIELD(double, busyTime, BusyTime)
};

}  // namespace inet
