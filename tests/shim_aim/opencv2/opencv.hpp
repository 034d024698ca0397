// The test-only cv:: stand-in of tests/cv_mock plus what rm::SolveGEA & co. need of OpenCV's array proxies: _InputArray::kind() with its MAT
// flag, and an _OutputArray a cv::Mat converts to.  RMCV_CV_HAS_ARRAY_KINDS tells include/rmcv_shim.hpp so (real OpenCV headers are
// recognised by their CV_VERSION).  tests/cv_mock's own proxy -- Mat only, no kind() -- is renamed out of the way.
#pragma once
#define _InputArray _InputArray_mat_only
#define InputArray InputArray_mat_only
#include "../../cv_mock/opencv2/opencv.hpp"
#undef _InputArray
#undef InputArray
#define RMCV_CV_HAS_ARRAY_KINDS 1
namespace cv {
struct _InputArray {
    enum KindFlag { NONE = 0, MAT = 1 << 16, STD_VECTOR = 3 << 16 };
    const Mat* m = nullptr;
    int k = NONE;
    _InputArray(const Mat& mm) : m(&mm), k(MAT) {}
    _InputArray(const std::vector<double>&) : k(STD_VECTOR) {}
    int kind() const { return k; }
    Mat getMat() const { return m ? *m : Mat(); }
};
typedef const _InputArray& InputArray;
struct _OutputArray : _InputArray {
    Mat* out;
    _OutputArray(Mat& mm) : _InputArray(mm), out(&mm) {}
    void assign(const Mat& v) const { *out = v; }
};
typedef const _OutputArray& OutputArray;
} // namespace cv
