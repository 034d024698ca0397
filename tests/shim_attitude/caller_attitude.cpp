// TEST-ONLY caller of the link test for rm::utils::homogeneous and rm::lookup_CRC: sees declarations only (never the shim).  Builds
// h_base2gripper the way executable/main.cpp:170 does -- the default translation -- and with a translation, checks a packet the way
// main.cpp:120-121 does, and prints what the test compares with the ABI's host functions.  Needs no GPU.
#include <cstdio>

#include "attitude_contract.hpp"

static void show(const char* name, const cv::Mat& m)
{
    std::printf("%s rows %d cols %d type %d", name, m.rows, m.cols, m.type());
    for (int i = 0; i < m.rows; i++)
        for (int j = 0; j < m.cols; j++) std::printf(" %a", m.ptr<double>(i)[j]);
    std::printf("\n");
}

int main()
{
    cv::Mat rotation(3, 3, CV_64F);
    for (int i = 0; i < 9; i++) rotation.ptr<double>(i / 3)[i % 3] = 0.125 * (i + 1) - 0.5;
    show("default", rm::utils::homogeneous(rotation));
    cv::Mat translation(3, 1, CV_64F);
    for (int i = 0; i < 3; i++) translation.ptr<double>(i)[0] = 10.5 * (i + 1);
    show("full", rm::utils::homogeneous(rotation, translation));
    show("bad_rotation", rm::utils::homogeneous(cv::Mat(4, 3, CV_64F), translation));
    show("bad_translation", rm::utils::homogeneous(rotation, cv::Mat(1, 3, CV_64F)));
    unsigned char buffer[24];
    for (int i = 0; i < 24; i++) buffer[i] = (unsigned char)(7 * i + 3);
    buffer[0] = 0x38;
    std::printf("crc %d\n", (int)rm::lookup_CRC(buffer, 23));
    unsigned char one[1] = {0xFF};
    std::printf("crc_one %d\n", (int)rm::lookup_CRC(one, 1));
    std::printf("crc_none %d\n", (int)rm::lookup_CRC(buffer, 0));
    return 0;
}
