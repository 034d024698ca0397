// TEST-ONLY: the DECLARATION of the reference's include/imgproc.h:17 next to tests/shim/rm_contract.hpp.  No logic.
#pragma once
#include "rm_contract.hpp"
namespace rm {
cv::Mat affine_correction(const cv::Mat& source, cv::Point2f vertices[4], cv::Size outSize);
} // namespace rm
