// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also records: the reference's debug.h
// (here: its stand-in), then the shim, which defines rm::debug::logger's member functions.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h", "debug.h"
#include "record_contract.hpp"
#include "rmcv_shim.hpp"
