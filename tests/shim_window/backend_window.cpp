// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also runs the locked-target loop:
// the declarations of include/core.h:142-147 with their default arguments, then the shim, which defines rm::utils::GetROI.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "window_contract.hpp"
#include "rmcv_shim.hpp"
