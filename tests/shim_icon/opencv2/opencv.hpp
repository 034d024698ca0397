// The test-only cv:: stand-in of tests/shim_window (tests/cv_mock plus cv::Size), which is all rm::affine_correction needs of OpenCV.
#pragma once
#include "../../shim_window/opencv2/opencv.hpp"
