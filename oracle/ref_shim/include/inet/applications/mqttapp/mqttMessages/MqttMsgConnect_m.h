// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): MqttMsgConnect, declared from the
// field list of its .msg file.
#pragma once
#include "shim_msg.h"

namespace inet {

class MqttMsgConnect : public cPacket {
    SHIM_PACKET(MqttMsgConnect)
    SHIM_FIELD(int, expectedReplyLength, ExpectedReplyLength)
    SHIM_FIELD(double, replyDelay, ReplyDelay)
    SHIM_FIELD(bool, serverClose, ServerClose)
    SHIM_STRING(type, Type)
    SHIM_FIELD(bool, dupFlag, DupFlag)
    SHIM_FIELD(int, qosLevel, QosLevel)
    SHIM_FIELD(bool, retain, Retain)
    SHIM_STRING(messageId, MessageId)
    SHIM_STRING(protocolName, ProtocolName)
    SHIM_STRING(protocolVersion, ProtocolVersion)
    SHIM_STRING(clientId, ClientId)
    SHIM_FIELD(bool, willRetain, WillRetain)
    SHIM_STRING(willQosLevel, WillQosLevel)
    SHIM_FIELD(bool, willFlag, WillFlag)
    SHIM_STRING(willTopic, WillTopic)
    SHIM_STRING(willMessage, WillMessage)
    SHIM_STRING(username, Username)
    SHIM_STRING(password, Password)
    SHIM_FIELD(bool, cleanSession, CleanSession)
    SHIM_FIELD(unsigned short, keepAlivePeriod, KeepAlivePeriod)
    SHIM_FIELD(bool, isBroker, IsBroker)
};

}  // namespace inet
