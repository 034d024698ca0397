// k_attitude.hip -- per-stream gimbal attitude: in front of a tracked batch, what the MCU sent for every camera stream -- a
// 24-byte serial packet, or the attitude table as it stands -- becomes the stream's base2gripper (what k_pnp puts positions into the base
// frame with), its world2camera and motor angle (what k_aim reads) and its enemy colour (what k_frame_keys reads), without the host.
//   rm::euler<double>::to_matrix   include/core.h:66-84
//   rm::utils::homogeneous         src/core.cpp:406-416
//   rm::lookup_CRC                 hardware/src/serialport.cpp:9-18
//   the packet check and decode    executable/main.cpp:120-143
// The step itself is device_attitude.h, the same source rmcv_attitude_step_host and the host functions run on the CPU.  The tracker's
// attitude tables and their setters and getters: rmcv_tracker.hip; the launcher takes the view of them (tracker_plan.h).
//
// Mapping (gfx950, wave64).  A few hundred dependent chains of scalar fp64 between a 24-byte load and a 300-byte store: ONE LANE PER STREAM,
// 64-lane workgroups, ceil(n_streams / 64) of them.  Ordinary vector loads and stores; no LDS, no atomics, no waits between workgroups;
// nothing is indexed dynamically in registers (no scratch).  Latency-bound like k_aim: the point is not its speed but that the host does
// nothing.
#include <math.h>
#include <string.h>

#include "rmcv_internal.h"
#include "device_attitude.h"

namespace rmcv {

// PER_STREAM: the lane's own hand-eye matrix in place of the config's -- 16 doubles that live in 32 VGPRs where the config's
// live in SGPRs.  A build of its own, so that the kernel a tracker without the table launches is the one it always launched.
template <bool PER_STREAM>
__global__ __launch_bounds__(64) void k_attitude(rmcv_attitude_config cfg, int n_streams, const uint8_t* __restrict__ packets,
                                                 rmcv_attitude* __restrict__ attitudes, int32_t* __restrict__ camps,
                                                 int32_t* __restrict__ packet_errors, double* __restrict__ base2gripper,
                                                 rmcv_aim_input* __restrict__ inputs,
                                                 const double* __restrict__ stream_g2c /* PER_STREAM: [n_streams][16] */)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n_streams) return;
    if (PER_STREAM) { // 16 ordinary vector loads, constant indices
        const double* m = stream_g2c + (size_t)f * 16;
#pragma unroll
        for (int i = 0; i < 16; i++) cfg.gripper2camera[i] = m[i];
    }
    att_stream(&cfg, packets ? packets + (size_t)f * RMCV_SERIAL_PACKET_BYTES : nullptr, &attitudes[f], camps ? &camps[f] : nullptr,
               &packet_errors[f], base2gripper ? base2gripper + (size_t)f * 16 : nullptr, &inputs[f]);
}

// v: the tracker's (tracker_plan.h); its attitude and aim tables are there while attitude is on
hipError_t launch_attitude(const TrackerView& v, const void* d_packets, double* d_base2gripper, hipStream_t s)
{
    const int n = v.cfg.n_streams;
    auto go = [&](auto kernel, const double* g2c) {
        return launch(kernel, dim3((n + 63) / 64), dim3(64), 0, s, v.att_cfg, n, (const uint8_t*)d_packets, v.attitudes, v.camps, v.packet_errors,
                      d_base2gripper, v.aim_inputs, g2c);
    };
    return v.stream_g2c ? go(k_attitude<true>, v.stream_g2c) : go(k_attitude<false>, nullptr);
}

} // namespace rmcv

using namespace rmcv;

extern "C" {

int rmcv_euler_to_matrix(const rmcv_attitude* a, double R[9])
{
    if (!a || !R) return RMCV_ERR_BAD_ARG;
    double r[9];
    att_to_matrix(a, r);
    for (int i = 0; i < 9; i++) R[i] = att_canon(r[i]);
    return RMCV_OK;
}

int rmcv_homogeneous(const double R[9], const double t[3], double H[16])
{
    if (!R || !H) return RMCV_ERR_BAD_ARG;
    double h[16];
    att_homogeneous(R, t, h);
    memcpy(H, h, sizeof(h));
    return RMCV_OK;
}

uint8_t rmcv_crc8(const uint8_t* data, int n)
{
    if (!data || n <= 0) return 0;
    return att_crc8(data, n);
}

int rmcv_serial_decode(const uint8_t pkt[24], int32_t* camp, rmcv_attitude* att)
{
    if (!pkt || !camp || !att) return RMCV_ERR_BAD_ARG;
    return att_decode(pkt, camp, att);
}

int rmcv_serial_encode(int32_t camp, float yaw_deg, float pitch_deg, float roll_deg, uint8_t pkt[24])
{
    if (!pkt || (camp != RMCV_CAMP_RED && camp != RMCV_CAMP_BLUE)) return RMCV_ERR_BAD_ARG;
    memset(pkt, 0, RMCV_SERIAL_PACKET_BYTES);
    pkt[0] = 0x38;
    pkt[1] = camp == RMCV_CAMP_RED ? 1 : 0;
    const struct { int at; float v; } put[3] = {{3, yaw_deg}, {11, pitch_deg}, {15, roll_deg}};
    for (const auto& f : put) {
        uint32_t u;
        memcpy(&u, &f.v, 4);
        for (int k = 0; k < 4; k++) pkt[f.at + k] = (uint8_t)(u >> (8 * k));
    }
    pkt[RMCV_SERIAL_PACKET_BYTES - 1] = att_crc8(pkt, RMCV_SERIAL_PACKET_BYTES - 1);
    return RMCV_OK;
}

int rmcv_attitude_step_host(const rmcv_attitude_config* cfg, const uint8_t* pkt, rmcv_attitude* att, int32_t* camp, int32_t* packet_errors,
                            double base2gripper[16], rmcv_aim_input* input)
{
    if (!cfg || !att || !packet_errors || !input || att_check_config(cfg)) return RMCV_ERR_BAD_ARG;
    att_stream(cfg, pkt, att, camp, packet_errors, base2gripper, input);
    return RMCV_OK;
}

void rmcv_default_attitude_config(rmcv_attitude_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    rmcv_pnp_config p;
    rmcv_default_pnp_config(&p);
    for (int i = 0; i < 16; i++) c->gripper2camera[i] = p.gripper2camera[i];
    c->motor_angle_mode = RMCV_ATT_MOTOR_KEEP;
}

} // extern "C"
