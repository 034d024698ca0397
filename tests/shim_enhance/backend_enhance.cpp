// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also uses the reference's exposure
// helpers: the declarations of include/imgproc.h:23, 35 with their default arguments, then the shim, which defines them.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "enhance_contract.hpp"
#include "rmcv_shim.hpp"
