// TEST-ONLY: the DECLARATIONS of the reference's include/imgproc.h:23, 35 (with their default arguments) next to tests/shim/rm_contract.hpp,
// plus the fused call the shim adds.  No logic.
#pragma once
#include "rm_contract.hpp"
namespace rm {
void CalcGamma(cv::Mat& source, cv::Mat& calibration, float gamma = 0.5f);
void AutoEnhance(cv::Mat& frame, float maxGainFactor = 100.0, float minGainFactor = 50.0);
std::tuple<std::vector<contour>, cv::Mat> extract_color_enhanced(cv::InputArray image, camp target, int lower_bound, float maxGainFactor = 100.0,
                                                                 float minGainFactor = 50.0);
} // namespace rm
