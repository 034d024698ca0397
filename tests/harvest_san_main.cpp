// harvest_san_main.cpp -- the host path of rmcv_amd/csrc/device_harvest.h as a stand-alone program (tests/test_harvest_plan.py builds it
// plainly, tests/test_harvest_sanitized.py with -fsanitize=address,undefined).  Every table is a heap block of exactly its size, the work
// list exactly as long as the rows that get a slot: a read or write one entry beyond any of them is the sanitizer's to find.
//
//   in : int32 n_calls, then per call  int32 n_frames, max_armours, flags, count, capacity, has_identity; int64 dropped;
//        int32 n_armours[n_frames], status[n_frames], labels[n_frames], identity[n_frames][max_armours] (if has_identity)
//   out: per call  int32 n_items, count; int64 dropped; int32 items[n_items][3]; int32 kept_per_frame[n_frames]
#include <stdio.h>
#include <stdlib.h>

#include "../rmcv_amd/csrc/device_harvest.h"

using namespace rmcv;

static int32_t* block(FILE* f, size_t n)
{
    int32_t* p = static_cast<int32_t*>(malloc(n * sizeof(int32_t))); // (malloc(0) may be null: such a table is never read)
    if (n && (!p || fread(p, sizeof(int32_t), n, f) != n)) exit(3);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_calls = 0;
    if (fread(&n_calls, 4, 1, in) != 1) return 3;
    for (int c = 0; c < n_calls; c++) {
        int32_t h[6];
        int64_t dropped = 0;
        if (fread(h, 4, 6, in) != 6 || fread(&dropped, 8, 1, in) != 1) return 3;
        const int n_frames = h[0], max_armours = h[1], flags = h[2];
        const int32_t count = h[3], capacity = h[4];
        int32_t* n_armours = block(in, (size_t)n_frames);
        int32_t* status = block(in, (size_t)n_frames);
        int32_t* labels = block(in, (size_t)n_frames);
        int32_t* identity = h[5] ? block(in, (size_t)n_frames * max_armours) : nullptr;
        int32_t* per_frame = static_cast<int32_t*>(malloc((size_t)n_frames * sizeof(int32_t)));
        int64_t kept = 0;
        for (int f = 0; f < n_frames; f++) {
            per_frame[f] = harvest_frame_kept(n_armours[f], max_armours, status[f], labels[f], flags, identity ? identity + (size_t)f * max_armours : nullptr);
            kept += per_frame[f];
        }
        const int64_t room = (int64_t)capacity - count;
        const size_t n_list = (size_t)(kept < room ? kept : room);
        HarvestItem* list = static_cast<HarvestItem*>(malloc(n_list * sizeof(HarvestItem)));
        int32_t now = 0;
        int64_t drop = 0;
        const int32_t n_items = harvest_plan_seq(n_armours, status, labels, identity, n_frames, max_armours, flags, count, capacity, list, &now, &drop);
        if ((size_t)n_items != n_list) return 4;
        dropped += drop;
        fwrite(&n_items, 4, 1, out);
        fwrite(&now, 4, 1, out);
        fwrite(&dropped, 8, 1, out);
        if (n_items) fwrite(list, sizeof(HarvestItem), (size_t)n_items, out);
        if (n_frames) fwrite(per_frame, 4, (size_t)n_frames, out);
        free(list), free(per_frame), free(identity), free(labels), free(status), free(n_armours);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
