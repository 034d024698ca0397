// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp), compiled against cv:: headers that know CV_16UC1:
// the shim then also emits rm::extract_color_raw, with external linkage like the rest.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h"
#include "rmcv_shim.hpp"
