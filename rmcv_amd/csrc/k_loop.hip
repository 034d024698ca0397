// k_loop.hip -- the session recorder's loop records: the tracker, aim and attitude state of the recorded streams, captured
// on the device behind a tracked batch's step, the trigger rule evaluated against the previous batch's record, and the latch that makes the
// recorder freeze by itself.  The record's layout and the rule are device_loop.h, the same source the host readers and
// rmcv_loop_trigger_host use.  Here too: the *_from_loop extractors, a replay's way back from a record (rmcv_tracker_restore: rmcv_tracker.hip).
//
// Mapping (gfx950, wave64).  ONE LAUNCH, one workgroup of 4 wavefronts per chosen frame; nothing here is heavy -- a record is under 1 KB
// of scalars plus 2584 bytes a track -- so the shape is chosen for latency: every copy is 8-byte words, one word per lane and trip (a track
// is 8-byte aligned, and 2584 = 8 * 323 bytes from the next: no wider access is aligned), consecutive lanes on consecutive words.  Thread
// 0 writes the scalars the rule reads and then evaluates it against the predecessor's record (written by an earlier launch); it reads back
// only its own stores.  No workgroup waits for another; every loop is bounded by the recorder's track_cap or a struct's size; nothing is
// indexed dynamically in registers (no scratch).  The latch is ONE vector atomic compare-and-swap on a device word; the winner writes the
// latch record with ordinary vector stores to device memory and to the mapped host copy, __threadfence_system(), then the `set` words.
#include <string.h>

#include "rmcv_internal.h"
#include "device_loop.h"

namespace rmcv {

static constexpr int LOOP_THREADS = 256;

// the latch record without its `set` word
__device__ static inline void latch_fill(LoopLatch* l, uint32_t hit, int k, int f, uint64_t sequence)
{
    l->fired = hit;
    l->k = k;
    l->stream = f;
    l->sequence = sequence;
}

__global__ __launch_bounds__(LOOP_THREADS) void k_loop_record(LoopArgs a)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= a.n) return;
    const int f = a.idx.f[k];
    if (f < 0 || f >= a.n_streams) return; // (the host has checked the list against the tracker)
    uint8_t* rec = a.out + (int64_t)k * a.pitch;
    rmcv_loop_state* o = reinterpret_cast<rmcv_loop_state*>(rec);
    int nt = a.tb.n_tracking[f];
    const int n_live = nt < 0 ? 0 : (nt > a.trk_cap ? a.trk_cap : nt);
    const int n_keep = n_live > a.rec_cap ? a.rec_cap : n_live;
    // ---- the tracks and their side records, from the tracker's CURRENT list (the step has just flipped sel): [track | side] per slot
    {
        const size_t at = ((size_t)(a.tb.sel[f] & 1) * a.n_streams + f) * a.trk_cap;
        const uint64_t* tr = reinterpret_cast<const uint64_t*>(a.tb.tracks + at);
        const uint64_t* sd = reinterpret_cast<const uint64_t*>(a.tb.side + at * 8);
        uint64_t* dst = reinterpret_cast<uint64_t*>(rec + sizeof(rmcv_loop_state));
        const int total = n_keep * LOOP_SLOT_WORDS; // <= rec_cap * 323
        for (int w = tid; w < total; w += LOOP_THREADS) {
            const int j = w / LOOP_SLOT_WORDS, r = w - j * LOOP_SLOT_WORDS;
            dst[w] = r < LOOP_TRACK_WORDS ? tr[(size_t)j * LOOP_TRACK_WORDS + r] : sd[(size_t)j * 4 + (r - LOOP_TRACK_WORDS)];
        }
    }
    // ---- the arrays of the fixed part (wavefronts 1 .. 3; wavefront 0 has the scalars and the rule)
    if (tid >= 64) {
        const int t = tid - 64; // 0 .. 191; every part below is shorter
        const int words_in = (int)(sizeof(rmcv_aim_input) / 8), words_att = (int)(sizeof(rmcv_attitude) / 8);
        const int words_tc = (int)(sizeof(rmcv_tracker_config) / 8), words_ac = (int)(sizeof(rmcv_aim_config) / 8);
        const int words_tt = (int)(sizeof(rmcv_attitude_config) / 8);
        if (t < words_in) {
            uint64_t v = 0; // the defaults: identity, 0
            if (a.aim_inputs) v = reinterpret_cast<const uint64_t*>(a.aim_inputs + f)[t];
            else if (t < 16 && t % 5 == 0) v = 0x3FF0000000000000ull;
            reinterpret_cast<uint64_t*>(&o->aim_input)[t] = v;
        }
        if (t < words_att) reinterpret_cast<uint64_t*>(&o->attitude)[t] = a.has_att ? reinterpret_cast<const uint64_t*>(a.attitudes + f)[t] : 0;
        if (t < 24) o->packet[t] = a.packets ? a.packets[(size_t)f * 24 + t] : (uint8_t)0;
        if (t < words_tc) reinterpret_cast<uint64_t*>(&o->tracker_config)[t] = reinterpret_cast<const uint64_t*>(&a.tcfg)[t];
        if (t < words_ac) {
            uint64_t v = 0;
            if (a.has_aim) v = a.aim_cfgs ? reinterpret_cast<const uint64_t*>(a.aim_cfgs + f)[t] : reinterpret_cast<const uint64_t*>(&a.aim_cfg)[t];
            reinterpret_cast<uint64_t*>(&o->aim_config)[t] = v;
        }
        if (t < words_tt) reinterpret_cast<uint64_t*>(&o->attitude_config)[t] = a.has_att ? reinterpret_cast<const uint64_t*>(&a.att_cfg)[t] : 0;
        if (t < 16) {
            double v = 0;
            if (a.has_att) v = a.stream_g2c ? a.stream_g2c[(size_t)f * 16 + t] : a.att_cfg.gripper2camera[t];
            o->gripper2camera[t] = v;
        }
        return;
    }
    if (tid != 0) return;
    // ---- the scalars, the aim record, and the rule
    o->stream = f;
    o->n_tracking = nt;
    o->status = a.tb.status[f];
    o->n_armours = a.n_armours[f];
    o->origin_next = a.tb.origins[f];
    rmcv_point eff = {0, 0};
    if (a.win_eff) eff = a.win_eff[f];
    o->origin_eff = eff;
    o->frame_status = a.frame_status[f];
    o->has_camps = a.has_camps;
    o->camp = a.tb.camps[f];
    o->lower_bound = a.tb.lower_bounds[f];
    o->has_key = a.key_eff != nullptr;
    FrameKey key = {0, 0, 0, 0};
    if (a.key_eff) key = a.key_eff[f];
    o->key[0] = key.ca, o->key[1] = key.cb, o->key[2] = key.lb, o->key[3] = key.all_pass;
    o->has_cameras = a.cam_eff != nullptr;
    o->cam_eff = a.cam_eff ? a.cam_eff[f] : 0;
    o->has_aim = a.has_aim;
    o->has_attitude = a.has_att;
    o->has_packet = a.packets != nullptr;
    o->packet_errors = a.has_att ? a.packet_errors[f] : 0;
    o->n_tracks = n_keep;
    o->flags = nt > a.rec_cap ? RMCV_LOOP_TRUNCATED : 0;
    o->trig_frame_status_mask = a.trig.frame_status_mask;
    o->trig_aim_jump_deg = a.trig.aim_jump_deg;
    o->timestamp = a.timestamp;
    o->sequence = a.sequence;
    {
        rmcv_aim aim; // zero: what the records hold before the first aim step
        memset(&aim, 0, sizeof(aim));
        if (a.aims) aim = a.aims[f];
        o->aim = aim;
    }
    uint32_t fired = 0;
    if (a.prev) fired = loop_trigger(reinterpret_cast<const rmcv_loop_state*>(a.prev + (int64_t)k * a.pitch), o, &a.trig);
    o->fired = fired;
    o->has_prev = a.prev != nullptr;
    const uint32_t hit = fired & a.trig.mask;
    if (hit && a.latch_word && atomicCAS(a.latch_word, 0u, 1u) == 0u) {
        latch_fill(a.d_latch, hit, k, f, a.sequence);
        latch_fill(a.hd_latch, hit, k, f, a.sequence);
        __threadfence_system();
        a.d_latch->set = 1;
        a.hd_latch->set = 1;
        __threadfence_system();
    }
}

hipError_t launch_loop_record(const LoopArgs& a, hipStream_t s) { return launch(k_loop_record, dim3(a.n), dim3(LOOP_THREADS), 0, s, a); }

} // namespace rmcv

using namespace rmcv;

extern "C" {

int64_t rmcv_loop_bound(int track_cap) { return loop_bound(track_cap); }

int rmcv_loop_trigger_host(const void* prev, const void* cur, const rmcv_trigger_config* cfg, uint32_t* fired)
{
    if (!prev || !cur || !cfg || !fired) return RMCV_ERR_BAD_ARG;
    rmcv_loop_state p, c; // (a caller's record need not be aligned)
    memcpy(&p, prev, sizeof(p));
    memcpy(&c, cur, sizeof(c));
    *fired = loop_trigger(&p, &c, cfg);
    return RMCV_OK;
}

int rmcv_tracker_config_from_loop(const void* rec, rmcv_tracker_config* out) { return loop_tracker_config(rec, out); }
int rmcv_tracker_aim_config_from_loop(const void* rec, rmcv_aim_config* out, int32_t* has) { return loop_aim_config(rec, out, has); }
int rmcv_tracker_attitude_config_from_loop(const void* rec, rmcv_attitude_config* out, double g2c[16], int32_t* has)
{
    return loop_attitude_config(rec, out, g2c, has);
}

} // extern "C"
