// The test-only cv:: stand-in of tests/cv_mock plus the one name rm::extract_color_raw needs of OpenCV: the 16-bit single-channel
// matrix type.  Compile-only (tests/test_raw_layout_cpu.py checks which symbols the backend object defines): the stand-in's cv::Mat
// still sizes every non-BGR row at one byte per pixel, so no 16-bit matrix is ever allocated through it.
#pragma once
#include "../../cv_mock/opencv2/opencv.hpp"
#ifndef CV_16UC1
#define CV_16UC1 2
#endif
