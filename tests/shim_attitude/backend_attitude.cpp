// The backend translation unit of INTEGRATION.md section 2 (tests/shim/backend.cpp) for a host that also reads the MCU link: the declarations
// of include/core.h:188 and hardware/include/serialport.h:49 with their default arguments, then the shim, which defines
// rm::utils::homogeneous and rm::lookup_CRC.
#include "rm_contract.hpp" // in the reference tree: "core.h", "imgproc.h", "objdetect.h", "mobility.h", "serialport.h"
#include "attitude_contract.hpp"
#include "rmcv_shim.hpp"
