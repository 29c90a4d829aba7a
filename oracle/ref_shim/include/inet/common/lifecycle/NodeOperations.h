// TEST INFRASTRUCTURE ONLY (oracle/ref_shim/README.md): the lifecycle operations
// are not modelled; the callback type lives in ApplicationBase.h.
#pragma once
#include "inet/applications/base/ApplicationBase.h"
