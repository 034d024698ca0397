// TEST-ONLY: the DECLARATIONS of the reference's include/core.h:142-147 (with their default arguments) next to tests/shim/rm_contract.hpp.
// No logic.
#pragma once
#include "rm_contract.hpp"
namespace rm::utils {
cv::Rect GetROI(cv::Point2f* imagePoints, int pointsCount, float scaleFactor = 1.0f, const cv::Size& frameSize = {-1, -1},
                const cv::Rect& previous = {0, 0, 0, 0});
cv::Rect GetROI(cv::Point2f* imagePoints, int pointsCount, const cv::Size2f& scaleFactor = {1, 1}, const cv::Size& frameSize = {-1, -1},
                const cv::Rect& previous = {0, 0, 0, 0});
} // namespace rm::utils
