// TEST-ONLY: the DECLARATIONS of the reference's include/mobility.h:18-23,55-62,75,95-97 (with their default arguments) next to
// tests/shim/rm_contract.hpp.  No logic.
#pragma once
#include "rm_contract.hpp"
#define RMCV_MOBILITY_H
namespace rm {
[[maybe_unused]] typedef enum CompensateMode { COMPENSATE_NONE = 0, COMPENSATE_CLASSIC = 1, COMPENSATE_NI = 2 } CompensateMode;
[[maybe_unused]] double DeltaHeight(cv::InputArray translationVector, double motorAngle, const cv::Point2f& offset = {0, 0}, double angleOffset = 0);
[[maybe_unused]] double Distance(cv::InputArray translationVector);
double ProjectileAngle(double v0, double g, double d, double h);
[[maybe_unused]] double SolveGEA(cv::InputArray translationVector, cv::OutputArray gimbalErrorAngle, double g, double v0, double h,
                                 const cv::Point2f& offset = {0, 0}, double angleOffset = 0, rm::CompensateMode mode = rm::COMPENSATE_NONE);
} // namespace rm
