/*
 * session_file.h -- the session recorder's file, host-side only: what rmcv_recorder_save and rmcv_session_append write and
 * rmcv_session_open reads.  Little-endian, as the structs lie in memory:
 *   header   8 bytes "RMCVSESS" | u32 version = 1 | u32 entry_bytes = sizeof(rmcv_record_entry)
 *   record   u64 record_bytes (everything behind this word) | rmcv_record_entry | the user blob, zeros to a multiple of 8 |
 *            the packed frames 0 .. n_frames - 1 back to back (sizes[k] bytes each, multiples of 8: device_pack.h) |
 *            with entry.loop_bytes != 0: the n_frames loop records back to back, loop_bytes each (device_loop.h)
 * A file none of whose entries has loop records is, byte for byte, what the format was before it knew them (loop_bytes took a pad word).
 * Records follow each other to the end of the file; there is no count, so a writer appends.  The reader checks every length against what
 * is left of the file before it uses it, and accepts nothing behind the last whole record.
 */
#ifndef RMCV_SESSION_FILE_H
#define RMCV_SESSION_FILE_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "device_loop.h"
#include "device_pack.h"

#define SESSION_VERSION 1u
static const char SESSION_MAGIC[8] = {'R', 'M', 'C', 'V', 'S', 'E', 'S', 'S'};
static const int64_t SESSION_HEAD = 16;

struct SessionRec {
    int64_t entry, user, frame[RMCV_RECORDER_MAX_FRAMES]; // offsets into the file
    int64_t loop;                                         // ... of the first loop record (entry.loop_bytes apart); 0: none
};

/* an entry whose lengths a recorder can have written */
static inline int session_entry_ok(const rmcv_record_entry& e)
{
    if (e.n_frames < 0 || e.n_frames > RMCV_RECORDER_MAX_FRAMES || e.user_bytes < 0) return 0;
    if (!pack_geometry_ok(e.w_bytes, e.h, e.lag)) return 0;
    const int64_t lo = pack_header_bytes(e.w_bytes, e.h) + pack_table_bytes(e.h), hi = pack_bound(e.w_bytes, e.h);
    for (int k = 0; k < e.n_frames; k++)
        if (e.sizes[k] < lo || e.sizes[k] > hi || (e.sizes[k] & 7)) return 0;
    if (e.loop_bytes != 0 && loop_cap_of(e.loop_bytes) < 0) return 0; // an area of some track_cap, or none
    return 1;
}
/* bytes of a record behind its length word */
static inline int64_t session_record_bytes(const rmcv_record_entry& e)
{
    int64_t n = (int64_t)sizeof(rmcv_record_entry) + pack_align8(e.user_bytes);
    for (int k = 0; k < e.n_frames; k++) n += e.sizes[k];
    n += (int64_t)e.n_frames * e.loop_bytes;
    return n;
}

/* data[0 .. len) as a session: RMCV_OK and the records' offsets, or RMCV_ERR_BAD_ARG */
static inline int session_parse(const uint8_t* data, int64_t len, std::vector<SessionRec>* recs)
{
    recs->clear();
    if (!data || len < SESSION_HEAD || memcmp(data, SESSION_MAGIC, 8) != 0) return RMCV_ERR_BAD_ARG;
    if (pack_get32(data + 8) != SESSION_VERSION || pack_get32(data + 12) != sizeof(rmcv_record_entry)) return RMCV_ERR_BAD_ARG;
    int64_t at = SESSION_HEAD;
    while (at < len) {
        if (len - at < 8 + (int64_t)sizeof(rmcv_record_entry)) return RMCV_ERR_BAD_ARG;
        const uint64_t said = (uint64_t)pack_get32(data + at) | (uint64_t)pack_get32(data + at + 4) << 32;
        rmcv_record_entry e;
        memcpy(&e, data + at + 8, sizeof(e));
        if (!session_entry_ok(e)) return RMCV_ERR_BAD_ARG;
        const int64_t bytes = session_record_bytes(e);
        if (said != (uint64_t)bytes || bytes > len - at - 8) return RMCV_ERR_BAD_ARG;
        SessionRec r;
        r.entry = at + 8;
        r.user = r.entry + (int64_t)sizeof(rmcv_record_entry);
        int64_t f = r.user + pack_align8(e.user_bytes);
        for (int k = 0; k < RMCV_RECORDER_MAX_FRAMES; k++) {
            r.frame[k] = f;
            if (k < e.n_frames) f += e.sizes[k];
        }
        r.loop = e.loop_bytes ? f : 0;
        // (the records lie inside the file: `bytes` above covers them.)  Their counts, before anything else of them is read
        for (int k = 0; e.loop_bytes && k < e.n_frames; k++) {
            rmcv_loop_state st;
            memcpy(&st, data + f + (int64_t)k * e.loop_bytes, sizeof(st));
            if (!loop_counts_ok(&st, e.loop_bytes)) return RMCV_ERR_BAD_ARG;
        }
        recs->push_back(r);
        at += 8 + bytes;
    }
    return RMCV_OK;
}

static inline int session_write_header(FILE* f)
{
    uint8_t h[16];
    memcpy(h, SESSION_MAGIC, 8);
    pack_put32(h + 8, SESSION_VERSION);
    pack_put32(h + 12, (uint32_t)sizeof(rmcv_record_entry));
    return fwrite(h, 1, sizeof(h), f) == sizeof(h) ? RMCV_OK : RMCV_ERR_BAD_ARG;
}

/* one record; packed[k]: sizes[k] bytes; loops[k]: e.loop_bytes bytes (with e.loop_bytes != 0) */
static inline int session_write_record(FILE* f, const rmcv_record_entry& e, const void* user, const uint8_t* const* packed,
                                       const uint8_t* const* loops = nullptr)
{
    if (!session_entry_ok(e) || (e.user_bytes > 0 && !user) || (e.loop_bytes != 0 && e.n_frames > 0 && !loops)) return RMCV_ERR_BAD_ARG;
    for (int k = 0; e.loop_bytes && k < e.n_frames; k++) { // what the reader would refuse is not written
        rmcv_loop_state st;
        if (!loops[k]) return RMCV_ERR_BAD_ARG;
        memcpy(&st, loops[k], sizeof(st));
        if (!loop_counts_ok(&st, e.loop_bytes)) return RMCV_ERR_BAD_ARG;
    }
    const int64_t bytes = session_record_bytes(e);
    uint8_t w[8];
    pack_put32(w, (uint32_t)bytes);
    pack_put32(w + 4, (uint32_t)((uint64_t)bytes >> 32));
    bool ok = fwrite(w, 1, 8, f) == 8 && fwrite(&e, 1, sizeof(e), f) == sizeof(e);
    if (ok && e.user_bytes > 0) ok = fwrite(user, 1, (size_t)e.user_bytes, f) == (size_t)e.user_bytes;
    const uint8_t zeros[8] = {0};
    const size_t pad = (size_t)(pack_align8(e.user_bytes) - e.user_bytes);
    if (ok && pad) ok = fwrite(zeros, 1, pad, f) == pad;
    for (int k = 0; k < e.n_frames && ok; k++) ok = packed && packed[k] && fwrite(packed[k], 1, (size_t)e.sizes[k], f) == (size_t)e.sizes[k];
    for (int k = 0; e.loop_bytes && k < e.n_frames && ok; k++) ok = fwrite(loops[k], 1, (size_t)e.loop_bytes, f) == (size_t)e.loop_bytes;
    return ok ? RMCV_OK : RMCV_ERR_BAD_ARG;
}

#endif /* RMCV_SESSION_FILE_H */
