// TEST-ONLY: what a host sees of the reference's include/debug.h for rm::debug::logger -- the class's interface and the three members the
// shim's definitions touch (the reference's class also owns its OpenCV video and storage objects, which the shim never uses).  No logic.
#pragma once
#include "rm_contract.hpp"
#include "rmcv_abi.h"
#define RMCV_DEBUG_H
namespace rm::debug {
class logger {
    int64 section_id = 0;
    int64 frame_id = 0;
    bool reading = true;

public:
    explicit logger(int64 section_id = -1, int FPS = 210, const cv::Size& resolution = {1280, 1024});
    ~logger();
    void write(const cv::Mat& image, const cv::Mat& data);
};
} // namespace rm::debug
