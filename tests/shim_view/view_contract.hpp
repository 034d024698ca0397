// TEST-ONLY: the DECLARATION a host adds next to the reference's include/debug.h for the shim's one addition there, with its default
// argument (the debug thread's size, executable/main.cpp:96).  No logic.
#pragma once
#include "rm_contract.hpp"
#include "rmcv_abi.h"
namespace rm::debug {
cv::Mat device_view(rmcv_ctx* context, int frame, const cv::Size& size = {1024, 768});
} // namespace rm::debug
