// The test-only cv:: stand-in of tests/cv_mock, which already has what rm::utils::homogeneous needs of OpenCV: a CV_64F cv::Mat with rows of
// doubles and cv::Mat::zeros.  RMCV_CV_HAS_MAT64 tells include/rmcv_shim.hpp so (real OpenCV headers are recognised by their CV_VERSION).
#pragma once
#include "../../cv_mock/opencv2/opencv.hpp"
#define RMCV_CV_HAS_MAT64 1
