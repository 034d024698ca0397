// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also aims: the declarations of
// include/mobility.h with their default arguments, then the shim, which defines rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "aim_contract.hpp"
#include "rmcv_shim.hpp"
