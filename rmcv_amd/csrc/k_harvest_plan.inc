// k_harvest_plan.inc -- the body of k_harvest_plan (k_harvest.hip; DESIGN.md 4m), compiled twice.  HP_KERNEL: the kernel's name.  HP_NOVEL
// (k_novelty.hip; DESIGN.md 4n): the kernel takes the keep bytes k_harvest_novel left for this append, [frame][max_armours], as a further
// input of harvest_keeps -- a candidate is kept when the rule of device_harvest.h keeps it AND its byte is set.  Without HP_NOVEL the text
// below is k_harvest_plan's as it always was.
#ifdef HP_NOVEL
#define HP_KEEP_PARAM const uint8_t* __restrict__ keep,
#define HP_KEEP_OF(f) , keep + (int64_t)(f) * max_armours
#define HP_FRAME_KEPT novel_frame_kept
#define HP_FRAME_EMIT novel_frame_emit
#else
#define HP_KEEP_PARAM
#define HP_KEEP_OF(f)
#define HP_FRAME_KEPT harvest_frame_kept
#define HP_FRAME_EMIT harvest_frame_emit
#endif

__global__ __launch_bounds__(256) void HP_KERNEL(const int32_t* __restrict__ n_armours, const int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ labels, const int32_t* __restrict__ identity, HP_KEEP_PARAM int n_frames,
                                                     int max_armours, int flags, int32_t capacity, HarvestCounters* __restrict__ ctr,
                                                     HarvestItem* __restrict__ list)
{
    __shared__ int s_carry[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (n_frames + 255) / 256;
    const int f0 = t * per, f1 = f0 + per < n_frames ? f0 + per : n_frames;
    const int32_t count = ctr->count; // (read by every thread before thread 0 rewrites it: the barriers below lie between)
    int mine = 0;
    for (int f = f0; f < f1; f++)
        mine += HP_FRAME_KEPT(n_armours[f], max_armours, status[f], labels[f], flags, identity ? identity + (int64_t)f * max_armours : nullptr HP_KEEP_OF(f));
    // inclusive scan of the wave's 64 totals, then the waves' carries through LDS
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane == 63) s_carry[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (q < wave) base += s_carry[q];
        total += s_carry[q];
    }
    int64_t k0 = (int64_t)base + incl - mine;
    for (int f = f0; f < f1; f++)
        k0 += HP_FRAME_EMIT(f, n_armours[f], max_armours, status[f], labels[f], flags, identity ? identity + (int64_t)f * max_armours : nullptr, k0,
                                 count, capacity, list HP_KEEP_OF(f));
    __syncthreads();
    if (t == 0) {
        int32_t now;
        int64_t drop;
        ctr->n_list = harvest_finish(count, capacity, total, &now, &drop);
        ctr->count = now;
        ctr->dropped += drop;
    }
}

#undef HP_KEEP_PARAM
#undef HP_KEEP_OF
#undef HP_FRAME_KEPT
#undef HP_FRAME_EMIT
