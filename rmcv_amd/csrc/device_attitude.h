/*
 * device_attitude.h -- the attitude step in front of a tracked batch for ONE camera stream, host and device from the same
 * source: what the MCU sent for the stream becomes the stream's base2gripper, world2camera, motor angle and enemy colour.
 *   rm::euler<double>::to_matrix   include/core.h:66-84
 *   rm::utils::homogeneous         src/core.cpp:406-416
 *   rm::lookup_CRC                 hardware/src/serialport.cpp:9-18   (bitwise, from the polynomial: no table)
 *   the packet check and decode    executable/main.cpp:120-143
 * Every product is a general one, summed left to right as written -- ((a0*b0 + a1*b1) + a2*b2) (+ a3*b3) -- with the matrices' zeros and
 * ones taking part, so signed zeros come out as a general product gives them.  sin and cos are pinned_math.h's (the same bits on the host
 * and on gfx950).  Compile with -ffp-contract=off, no fast-math.  Every NaN that leaves is THE quiet NaN (att_canon, as device_aim.h's
 * aim_canon): the sign and payload of a computed NaN depend on the machine.
 *
 * Execution model.  att_stream is ONE LANE per stream: a dependent chain of a few dozen fp64 operations between ordinary loads and stores.
 * Every array below is indexed by constants only (nothing lands in scratch).
 */
#ifndef RMCV_DEVICE_ATTITUDE_H
#define RMCV_DEVICE_ATTITUDE_H

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "pinned_math.h"

#define ATT_PI 3.141592653589793 /* CV_PI */

PM_FN double att_canon(double x) { return x != x ? __builtin_nan("") : x; }
PM_FN int att_finite(double x) { return x - x == 0.0; }

/* C = A . B, 3x3 row-major; C is neither A nor B */
#define ATT_E3(A, B, i, j) (((A)[3 * (i)] * (B)[(j)] + (A)[3 * (i) + 1] * (B)[3 + (j)]) + (A)[3 * (i) + 2] * (B)[6 + (j)])
PM_FN void att_mul3(const double* A, const double* B, double* C)
{
    C[0] = ATT_E3(A, B, 0, 0); C[1] = ATT_E3(A, B, 0, 1); C[2] = ATT_E3(A, B, 0, 2);
    C[3] = ATT_E3(A, B, 1, 0); C[4] = ATT_E3(A, B, 1, 1); C[5] = ATT_E3(A, B, 1, 2);
    C[6] = ATT_E3(A, B, 2, 0); C[7] = ATT_E3(A, B, 2, 1); C[8] = ATT_E3(A, B, 2, 2);
}

/* core.h:66-84: R = (Rz . Ry) . Rx of euler{x = roll, y = pitch, z = yaw} */
PM_FN void att_to_matrix(const rmcv_attitude* a, double* R)
{
    const double cz = pm_cos(a->yaw), sz = pm_sin(a->yaw), cy = pm_cos(a->pitch), sy = pm_sin(a->pitch), cx = pm_cos(a->roll), sx = pm_sin(a->roll);
    const double rz[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};
    const double ry[9] = {cy, 0.0, sy, 0.0, 1.0, 0.0, -sy, 0.0, cy};
    const double rx[9] = {1.0, 0.0, 0.0, 0.0, cx, -sx, 0.0, sx, cx};
    double zy[9];
    att_mul3(rz, ry, zy);
    att_mul3(zy, rx, R);
}

/* core.cpp:406-416: R and t (NULL: zeros) in an identity 4x4 */
PM_FN void att_homogeneous(const double* R, const double* t, double* H)
{
    H[0] = R[0]; H[1] = R[1]; H[2] = R[2];   H[3] = t ? t[0] : 0.0;
    H[4] = R[3]; H[5] = R[4]; H[6] = R[5];   H[7] = t ? t[1] : 0.0;
    H[8] = R[6]; H[9] = R[7]; H[10] = R[8];  H[11] = t ? t[2] : 0.0;
    H[12] = 0.0; H[13] = 0.0; H[14] = 0.0;   H[15] = 1.0;
}

/* serialport.cpp:9-18 with the table's polynomial worked bit by bit: x^8 + x^5 + x^4 + 1 (0x31), MSB first, init 0, no reflection, no final xor */
PM_FN uint8_t att_crc8(const uint8_t* data, int n)
{
    uint32_t crc = 0;
    for (int i = 0; i < n; i++) {
        crc ^= data[i];
        for (int b = 0; b < 8; b++) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x31u) & 0xFFu : (crc << 1) & 0xFFu;
    }
    return (uint8_t)crc;
}

PM_FN float att_f32le(const uint8_t* p)
{
    const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
/* main.cpp:138: `deg * CV_PI / 180.0f` -- a float times a double, divided by a float */
PM_FN double att_radians(float deg) { return ((double)deg * ATT_PI) / (double)180.0f; }

/* main.cpp:120-143: 1 and (*camp, *att) for a valid packet; 0, nothing written, for a rejected one */
PM_FN int att_decode(const uint8_t* pkt, int32_t* camp, rmcv_attitude* att)
{
    if (pkt[0] != 0x38 || pkt[RMCV_SERIAL_PACKET_BYTES - 1] != att_crc8(pkt, RMCV_SERIAL_PACKET_BYTES - 1)) return 0;
    *camp = (pkt[1] & 0x01) ? RMCV_CAMP_RED : RMCV_CAMP_BLUE;
    att->yaw = att_canon(att_radians(att_f32le(pkt + 3)));
    att->pitch = att_canon(att_radians(att_f32le(pkt + 11)));
    att->roll = att_canon(att_radians(att_f32le(pkt + 15)));
    return 1;
}

/* rows 0..2 of A . B, 4x4 row-major, in the aim step's row order (device_aim.h: aim_solve_at); row 3 is never read behind it */
#define ATT_E4(A, B, i, j) ((((A)[4 * (i)] * (B)[(j)] + (A)[4 * (i) + 1] * (B)[4 + (j)]) + (A)[4 * (i) + 2] * (B)[8 + (j)]) + (A)[4 * (i) + 3] * (B)[12 + (j)])
PM_FN void att_mul4_rows(const double* A, const double* B, double* C)
{
    C[0] = ATT_E4(A, B, 0, 0); C[1] = ATT_E4(A, B, 0, 1); C[2] = ATT_E4(A, B, 0, 2);  C[3] = ATT_E4(A, B, 0, 3);
    C[4] = ATT_E4(A, B, 1, 0); C[5] = ATT_E4(A, B, 1, 1); C[6] = ATT_E4(A, B, 1, 2);  C[7] = ATT_E4(A, B, 1, 3);
    C[8] = ATT_E4(A, B, 2, 0); C[9] = ATT_E4(A, B, 2, 1); C[10] = ATT_E4(A, B, 2, 2); C[11] = ATT_E4(A, B, 2, 3);
}

/* a rigid [R t; 0 1] (rows 0..2 of m are read) -> [R^T  -R^T t; 0 1]: the body of rmcv_rigid_inverse.  r is not m. */
#define ATT_INV_ROW(m, r, i)                                                                    \
    (r)[4 * (i)] = (m)[(i)]; (r)[4 * (i) + 1] = (m)[4 + (i)]; (r)[4 * (i) + 2] = (m)[8 + (i)]; \
    (r)[4 * (i) + 3] = -(((m)[(i)] * (m)[3] + (m)[4 + (i)] * (m)[7]) + (m)[8 + (i)] * (m)[11])
PM_FN void att_rigid_inverse(const double* m, double* r)
{
    ATT_INV_ROW(m, r, 0);
    ATT_INV_ROW(m, r, 1);
    ATT_INV_ROW(m, r, 2);
    r[12] = 0.0; r[13] = 0.0; r[14] = 0.0;
    r[15] = 1.0;
}

/* one stream's step.  pkt: the stream's 24 bytes or NULL (the attitude as it stands); camp: the tracker's camp entry or NULL (table off);
 * base2gripper: the batch context's entry or NULL (no pose tables) */
PM_FN void att_stream(const rmcv_attitude_config* cfg, const uint8_t* pkt, rmcv_attitude* att, int32_t* camp, int32_t* packet_errors,
                      double* base2gripper, rmcv_aim_input* input)
{
    rmcv_attitude a = *att;
    if (pkt) {
        int32_t c = 0;
        rmcv_attitude d;
        if (att_decode(pkt, &c, &d)) {
            a = d;
            *att = d;
            if (camp) *camp = c;
        } else {
            *packet_errors = *packet_errors + 1; /* the reference's `continue`: the last good package stays in use */
        }
    }
    double R[9], B[16], M[12], W[16];
    att_to_matrix(&a, R);
    att_homogeneous(R, (const double*)0, B);
    if (base2gripper) {
        base2gripper[0] = att_canon(B[0]);   base2gripper[1] = att_canon(B[1]);   base2gripper[2] = att_canon(B[2]);   base2gripper[3] = B[3];
        base2gripper[4] = att_canon(B[4]);   base2gripper[5] = att_canon(B[5]);   base2gripper[6] = att_canon(B[6]);   base2gripper[7] = B[7];
        base2gripper[8] = att_canon(B[8]);   base2gripper[9] = att_canon(B[9]);   base2gripper[10] = att_canon(B[10]); base2gripper[11] = B[11];
        base2gripper[12] = B[12];            base2gripper[13] = B[13];            base2gripper[14] = B[14];            base2gripper[15] = B[15];
    }
    att_mul4_rows(B, cfg->gripper2camera, M);
    att_rigid_inverse(M, W);
    double* o = input->world2camera;
    o[0] = att_canon(W[0]);  o[1] = att_canon(W[1]);  o[2] = att_canon(W[2]);   o[3] = att_canon(W[3]);
    o[4] = att_canon(W[4]);  o[5] = att_canon(W[5]);  o[6] = att_canon(W[6]);   o[7] = att_canon(W[7]);
    o[8] = att_canon(W[8]);  o[9] = att_canon(W[9]);  o[10] = att_canon(W[10]); o[11] = att_canon(W[11]);
    o[12] = W[12];           o[13] = W[13];           o[14] = W[14];            o[15] = W[15];
    if (cfg->motor_angle_mode == RMCV_ATT_MOTOR_PITCH) input->motor_angle = a.pitch;
}

/* what rmcv_tracker_set_attitude refuses; NULL: fine */
PM_FN const char* att_check_config(const rmcv_attitude_config* c)
{
    int ok = 1;
    for (int i = 0; i < 16; i++) ok &= att_finite(c->gripper2camera[i]);
    if (!ok) return "attitude config: every entry of gripper2camera must be finite";
    if (c->motor_angle_mode != RMCV_ATT_MOTOR_KEEP && c->motor_angle_mode != RMCV_ATT_MOTOR_PITCH) return "attitude config: motor_angle_mode out of range";
    return (const char*)0;
}

#endif /* RMCV_DEVICE_ATTITUDE_H */
