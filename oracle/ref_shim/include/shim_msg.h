// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): what OMNeT++'s message
// compiler would generate for one field of a .msg file, as far as the v3
// modules use it: a getter and a setter named after the field, strings handed
// out as const char * into the message (which is why delivered messages are
// never freed), and a dup() that returns the class itself.
#pragma once
#include "inet/common/INETDefs.h"

#define SHIM_PACKET(CLASS)                                                        \
  public:                                                                         \
    explicit CLASS(const char *n = nullptr, short k = 0) : cPacket(n, k) {}       \
    CLASS *dup() const override { return new CLASS(*this); }

#define SHIM_FIELD(TYPE, NAME, CAP)                                               \
  private:                                                                        \
    TYPE NAME##_{};                                                               \
  public:                                                                         \
    TYPE get##CAP() const { return NAME##_; }                                     \
    void set##CAP(TYPE v) { NAME##_ = v; }

#define SHIM_STRING(NAME, CAP)                                                    \
  private:                                                                        \
    std::string NAME##_;                                                          \
  public:                                                                         \
    const char *get##CAP() const { return NAME##_.c_str(); }                      \
    void set##CAP(const char *v) { NAME##_ = v ? v : ""; }
