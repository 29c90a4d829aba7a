// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): stand-in for INET 3.3's
// ApplicationBase / OperationalBase.  The node is always up: handleNodeStart()
// runs once, in the application-layer init stage, and every message goes to
// handleMessageWhenUp().
#pragma once
#include "inet/common/INETDefs.h"

namespace inet {

class IDoneCallback {};

class ApplicationBase : public cSimpleModule {
  protected:
    bool isOperational = false;
    virtual int numInitStages() const { return NUM_INIT_STAGES; }
    virtual void initialize(int stage) {
        if (stage == INITSTAGE_APPLICATION_LAYER) {
            isOperational = true;
            handleNodeStart(nullptr);
        }
    }
    virtual void handleMessageWhenUp(cMessage *msg) = 0;
    virtual void finish() {}
    virtual bool handleNodeStart(IDoneCallback *doneCallback) = 0;
    virtual bool handleNodeShutdown(IDoneCallback *doneCallback) = 0;
    virtual void handleNodeCrash() = 0;
  public:
    void handleMessage(cMessage *msg) override { handleMessageWhenUp(msg); }
    void shimInitialize() {
        for (int stage = 0; stage < numInitStages(); stage++) initialize(stage);
    }
};

}  // namespace inet
