// TEST-ONLY caller of the link test for rm::debug::logger: sees declarations only (never the shim).  In the current directory it opens
// section ID, writes two synthetic BGR frames (W x H, the second one through a row stride) and one single-channel frame, each with a `data`
// record, closes the logger, and opens the section again: the directory exists, so that logger is read-only and its write is dropped.
//   shim_record_main ID W H
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "record_contract.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    const long long id = atoll(argv[1]);
    const int w = atoi(argv[2]), h = atoi(argv[3]);
    std::vector<unsigned char> tight((size_t)3 * w * h), wide((size_t)(3 * w + 9) * h, 0xEE), gray((size_t)w * h);
    if (rmcv_synth_frame(tight.data(), w, h, 3 * w, 3, 1, 0) || rmcv_synth_frame(wide.data(), w, h, 3 * w + 9, 4, 1, 0)) return 2;
    for (size_t i = 0; i < gray.size(); i++) gray[i] = tight[3 * i + 1];
    double numbers[3] = {1.5, -2.0, 1e9};
    {
        rm::debug::logger log(id);
        cv::Mat a(h, w, CV_8UC3, tight.data()), b(h, w, CV_8UC3, wide.data()), c(h, w, CV_8UC1, gray.data());
        b.step = (size_t)3 * w + 9;
        cv::Mat data(1, 3, CV_64F), none;
        for (int i = 0; i < 3; i++) data.at<double>(0, i) = numbers[i];
        log.write(a, data);
        log.write(b, none);
        log.write(c, data);
    }
    {
        rm::debug::logger again(id); // the section exists: read-only
        cv::Mat a(h, w, CV_8UC3, tight.data()), none;
        again.write(a, none);
    }
    std::printf("written 3\n");
    return 0;
}
