// TEST-ONLY caller of the link test for the aiming functions: sees declarations only (never the shim).  Calls the four rm:: functions the
// way a robot's loop does -- the reference's default arguments, then every argument -- and prints what the test compares with the ABI's
// host functions.  Needs no GPU.
#include <cstdio>

#include "aim_contract.hpp"

int main()
{
    cv::Mat tvec(3, 1, CV_64F);
    const double tv[3] = {10.0, -5.0, 300.0};
    for (int i = 0; i < 3; i++) tvec.ptr<double>()[i] = tv[i];
    std::printf("angle %a\n", rm::ProjectileAngle(15, 9.8, 3, 0.2));
    std::printf("distance %a\n", rm::Distance(tvec));
    std::printf("height_default %a\n", rm::DeltaHeight(tvec, 0.1));
    std::printf("height_full %a\n", rm::DeltaHeight(tvec, 0.1, cv::Point2f(1.5f, -2.5f), 0.01));
    cv::Mat gea;
    const double t0 = rm::SolveGEA(tvec, gea, 9.8, 28.0, 20.0); // COMPENSATE_NONE, no offsets
    std::printf("gea_default %a %a %a rows %d cols %d type %d\n", t0, gea.ptr<double>()[0], gea.ptr<double>()[1], gea.rows, gea.cols, gea.type());
    cv::Mat gea2;
    const double t1 = rm::SolveGEA(tvec, gea2, 9.8, 28.0, 20.0, cv::Point2f(1.5f, -2.5f), 0.01, rm::COMPENSATE_CLASSIC);
    std::printf("gea_classic %a %a %a\n", t1, gea2.ptr<double>()[0], gea2.ptr<double>()[1]);
    cv::Mat gea3;
    const double t2 = rm::SolveGEA(tvec, gea3, 9.8, 28.0, 20.0, {0, 0}, 0, rm::COMPENSATE_NI);
    std::printf("gea_ni %a created %d\n", t2, gea3.rows * gea3.cols);
    const std::vector<double> not_a_mat{10.0, -5.0, 300.0}; // anything but a cv::Mat: NAN, as the reference answers
    cv::Mat gea4;
    std::printf("not_mat %a %a %a created %d\n", rm::Distance(not_a_mat), rm::DeltaHeight(not_a_mat, 0.1), rm::SolveGEA(not_a_mat, gea4, 9.8, 28.0, 20.0),
                gea4.rows * gea4.cols);
    return 0;
}
