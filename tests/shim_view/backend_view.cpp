// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also wants the operator's view: the
// declaration of rm::debug::device_view with its default argument, then the shim, which defines it.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "view_contract.hpp"
#include "rmcv_shim.hpp"
