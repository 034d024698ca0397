// k_attitude.hip -- per-stream gimbal attitude: in front of a tracked batch, what the MCU sent for every camera stream -- a
// 24-byte serial packet, or the attitude table as it stands -- becomes the stream's base2gripper (what k_pnp puts positions into the base
// frame with), its world2camera and motor angle (what k_aim reads) and its enemy colour (what k_frame_keys reads), without the host.
//   rm::euler<double>::to_matrix   include/core.h:66-84
//   rm::utils::homogeneous         src/core.cpp:406-416
//   rm::lookup_CRC                 hardware/src/serialport.cpp:9-18
//   the packet check and decode    executable/main.cpp:120-143
// The step itself is device_attitude.h, the same source rmcv_attitude_step_host and the host functions run on the CPU.
//
// Mapping (gfx950, wave64).  A few hundred dependent chains of scalar fp64 between a 24-byte load and a 300-byte store: ONE LANE PER STREAM,
// 64-lane workgroups, ceil(n_streams / 64) of them.  Ordinary vector loads and stores; no LDS, no atomics, no waits between workgroups;
// nothing is indexed dynamically in registers (no scratch).  Latency-bound like k_aim: the point is not its speed but that the host does
// nothing.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

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

bool tracker_attitude_on(const rmcv_tracker* t) { return t->att_on; }

hipError_t launch_attitude(const rmcv_tracker* t, const void* d_packets, double* d_base2gripper, hipStream_t s)
{
    const int n = t->cfg.n_streams;
    auto go = [&](auto kernel, const double* g2c) {
        return launch(kernel, dim3((n + 63) / 64), dim3(64), 0, s, t->att_cfg, n, (const uint8_t*)d_packets, t->attitudes,
                      t->camps_on ? t->b.camps : nullptr, t->packet_errors, d_base2gripper, t->aim_inputs, g2c);
    };
    return t->stream_g2c_on ? go(k_attitude<true>, t->stream_g2c) : go(k_attitude<false>, nullptr);
}

} // namespace rmcv

using namespace rmcv;

#define TCHK(t, call, what)                                                        \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) return tracker_fail((t), RMCV_ERR_HIP, what, e__);  \
    } while (0)

// the attitudes and the packet counters (zero), on first use; the aim tables with them (the step writes the inputs)
static int att_alloc(rmcv_tracker* t)
{
    void* d_in = nullptr;
    int rc = rmcv_tracker_device_aim_inputs(t, &d_in); // (allocates the aim tables if they are not there yet)
    if (rc) return rc;
    if (t->attitudes) return RMCV_OK;
    const size_t n = (size_t)t->cfg.n_streams;
    rmcv_attitude* d_att = nullptr;
    int32_t* d_err = nullptr;
    hipError_t e = hipMalloc((void**)&d_att, n * sizeof(rmcv_attitude));
    if (e == hipSuccess) {
        t->allocs.push_back(d_att);
        e = hipMalloc((void**)&d_err, n * sizeof(int32_t));
    }
    if (e == hipSuccess) {
        t->allocs.push_back(d_err);
        e = hipMemset(d_att, 0, n * sizeof(rmcv_attitude));
    }
    if (e == hipSuccess) e = hipMemset(d_err, 0, n * sizeof(int32_t));
    if (e != hipSuccess) return tracker_fail(t, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "allocating the attitude tables", e);
    t->attitudes = d_att;
    t->packet_errors = d_err;
    return RMCV_OK;
}

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

int rmcv_tracker_set_attitude(rmcv_tracker* t, const rmcv_attitude_config* cfg)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    if (cfg) { // (the refusals need no device)
        const char* bad = att_check_config(cfg);
        if (bad) return tracker_fail(t, RMCV_ERR_BAD_ARG, bad);
    }
    hipSetDevice(t->device);
    int rc = tracker_wait_done(t);
    if (rc) return rc;
    if (!cfg) {
        t->att_on = false;
        return RMCV_OK;
    }
    if ((rc = att_alloc(t))) return rc;
    t->att_cfg = *cfg;
    t->att_on = true;
    return RMCV_OK;
}

int rmcv_tracker_set_stream_cameras(rmcv_tracker* t, const double* gripper2camera)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    const size_t n = (size_t)t->cfg.n_streams;
    if (gripper2camera) { // (the refusals need no device)
        for (size_t f = 0; f < n; f++)
            for (int i = 0; i < 16; i++)
                if (!att_finite(gripper2camera[f * 16 + i])) {
                    char msg[160];
                    snprintf(msg, sizeof(msg), "rmcv_tracker_set_stream_cameras: stream %d: every entry of gripper2camera must be finite", (int)f);
                    return tracker_fail(t, RMCV_ERR_BAD_ARG, msg);
                }
    }
    hipSetDevice(t->device);
    int rc = tracker_wait_done(t);
    if (rc) return rc;
    if (!gripper2camera) {
        t->stream_g2c_on = false;
        return RMCV_OK;
    }
    if (!t->stream_g2c) {
        double* d = nullptr;
        const hipError_t e = hipMalloc((void**)&d, n * 16 * sizeof(double));
        if (e != hipSuccess) return tracker_fail(t, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "allocating the streams' gripper2camera table", e);
        t->allocs.push_back(d);
        t->stream_g2c = d;
    }
    TCHK(t, hipMemcpy(t->stream_g2c, gripper2camera, n * 16 * sizeof(double), hipMemcpyHostToDevice), "H2D stream cameras");
    t->stream_g2c_on = true;
    return RMCV_OK;
}

int rmcv_tracker_set_attitudes(rmcv_tracker* t, const rmcv_attitude* attitudes)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    int rc = tracker_wait_done(t);
    if (rc) return rc;
    if ((rc = att_alloc(t))) return rc;
    const size_t bytes = (size_t)t->cfg.n_streams * sizeof(rmcv_attitude);
    if (attitudes) TCHK(t, hipMemcpy(t->attitudes, attitudes, bytes, hipMemcpyHostToDevice), "H2D attitudes");
    else TCHK(t, hipMemset(t->attitudes, 0, bytes), "attitudes");
    return RMCV_OK;
}

int rmcv_tracker_get_attitudes(rmcv_tracker* t, rmcv_attitude* out, int32_t* packet_errors, int cap)
{
    if (!t || cap < 0) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait_done(t);
    if (rc) return rc;
    const size_t n = (size_t)std::min(cap, t->cfg.n_streams);
    if (!n) return RMCV_OK;
    if (!t->attitudes) { // (never used: what the tables would hold)
        if (out) memset(out, 0, n * sizeof(rmcv_attitude));
        if (packet_errors) memset(packet_errors, 0, n * sizeof(int32_t));
        return RMCV_OK;
    }
    if (out) TCHK(t, hipMemcpy(out, t->attitudes, n * sizeof(rmcv_attitude), hipMemcpyDeviceToHost), "D2H attitudes");
    if (packet_errors) TCHK(t, hipMemcpy(packet_errors, t->packet_errors, n * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H packet errors");
    return RMCV_OK;
}

int rmcv_tracker_device_attitudes(rmcv_tracker* t, void** d_attitudes)
{
    if (!t || !d_attitudes) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = att_alloc(t);
    if (rc) return rc;
    *d_attitudes = t->attitudes;
    return RMCV_OK;
}

int rmcv_tracker_get_aim_inputs(rmcv_tracker* t, rmcv_aim_input* out, int cap)
{
    if (!t || cap < 0 || (cap > 0 && !out)) return RMCV_ERR_BAD_ARG;
    hipSetDevice(t->device);
    const int rc = tracker_wait_done(t);
    if (rc) return rc;
    const size_t n = (size_t)std::min(cap, t->cfg.n_streams);
    if (!n) return RMCV_OK;
    if (!t->aim_inputs) { // (never used: the defaults)
        memset(out, 0, n * sizeof(rmcv_aim_input));
        for (size_t f = 0; f < n; f++)
            for (int i = 0; i < 4; i++) out[f].world2camera[i * 5] = 1.0;
        return RMCV_OK;
    }
    TCHK(t, hipMemcpy(out, t->aim_inputs, n * sizeof(rmcv_aim_input), hipMemcpyDeviceToHost), "D2H aim inputs");
    return RMCV_OK;
}

} // extern "C"
