// TEST-ONLY caller of the link test for rm::affine_correction: sees the declaration only (never the shim).  For every record of the input
// file -- an armour's icon and an output size -- it makes the call of executable/main.cpp:180,
//     cv::Mat icon = rm::affine_correction(frame->image, armour.icon, {20, 20});
// with the record's size, and writes the vertices as the call left them (clamped in place) and the icon's bytes.
// Input: int32 w, h | the BGR image, 3 w h bytes | int32 n | per record 8 float32 (the icon), int32 ow, oh.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icon_contract.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int w = 0, h = 0, n = 0;
    if (std::fread(&w, 4, 1, in) != 1 || std::fread(&h, 4, 1, in) != 1) return 2;
    cv::Mat image(h, w, CV_8UC3);
    if (std::fread(image.data, 1, (size_t)3 * w * h, in) != (size_t)3 * w * h || std::fread(&n, 4, 1, in) != 1) return 2;
    for (int i = 0; i < n; i++) {
        rm::armour armour{{}};
        float q[8];
        int size[2];
        if (std::fread(q, 4, 8, in) != 8 || std::fread(size, 4, 2, in) != 2) return 2;
        for (int k = 0; k < 4; k++) armour.icon[k] = cv::Point2f(q[2 * k], q[2 * k + 1]);
        cv::Mat icon = rm::affine_correction(image, armour.icon, {size[0], size[1]});
        if (icon.rows != size[1] || icon.cols != size[0] || icon.type() != CV_8UC3) return 3;
        for (int k = 0; k < 4; k++) q[2 * k] = armour.icon[k].x, q[2 * k + 1] = armour.icon[k].y;
        std::fwrite(q, 4, 8, out);
        for (int y = 0; y < icon.rows; y++) std::fwrite(icon.ptr<unsigned char>(y), 1, (size_t)3 * icon.cols, out);
    }
    bool threw = false; // a size the rule does not take: the shim throws, as a cv::Exception would escape
    try {
        rm::armour armour{{}};
        rm::affine_correction(image, armour.icon, {257, 20});
    } catch (const std::exception&) {
        threw = true;
    }
    std::printf("records %d refused %d\n", n, threw ? 1 : 0);
    return std::fclose(out) ? 3 : 0;
}
