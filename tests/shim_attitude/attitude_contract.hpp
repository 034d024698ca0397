// TEST-ONLY: the DECLARATIONS of the reference's include/core.h:188 and hardware/include/serialport.h:49 (with their default arguments) next to
// tests/shim/rm_contract.hpp.  No logic.  (The reference's default for crcTable is its table rm::CRC8, which lives in serialport.h; the shim
// never reads the argument, and the table is not repeated here.)
#pragma once
#include "rm_contract.hpp"
#define RMCV_SERIALPORT_H
namespace rm::utils {
cv::Mat homogeneous(const cv::Mat& rotation, const cv::Mat& translation = cv::Mat::zeros(3, 1, CV_64F));
} // namespace rm::utils
namespace rm {
unsigned char lookup_CRC(unsigned char* data, unsigned char dataLength, const unsigned char* crcTable = nullptr);
} // namespace rm
