// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also rectifies icons: the declaration of
// include/imgproc.h:17, then the shim, which defines it.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "icon_contract.hpp"
#include "rmcv_shim.hpp"
