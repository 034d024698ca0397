// The test-only cv:: stand-in of tests/shim_window (tests/cv_mock plus cv::Size), which is all rm::debug::logger needs of OpenCV.
#pragma once
#include "../../shim_window/opencv2/opencv.hpp"
