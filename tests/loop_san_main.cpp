// TEST-ONLY stand-alone program around the host side of the recorder's loop records -- rmcv_amd/csrc/device_loop.h (the layout's checks,
// the trigger rule, the setup extractors) and rmcv_amd/csrc/session_file.h (the session file's writer and reader) -- for a sanitizer build
// (tests/test_loop_sanitized.py: -fsanitize=address,undefined; no GPU, nothing loaded into python).  Every buffer is a heap block of exactly
// its size, so a read or write too far shows.
//   loop_san_main SESSION
// A session of two records WITH loop records (track_cap 2; 2 and 1 frames) is written to SESSION; then session_parse runs on every prefix
// length of it and with single bytes altered -- the first record's length word, its entry (loop_bytes included), and the fixed part of each
// of the three loop records -- and every parse that succeeds is walked, every byte its offsets promise.  Then the rule and the extractors
// run on records whose n_tracks is negative or beyond any area.  Every call must return RMCV_OK or RMCV_ERR_BAD_ARG;
// stdout: "prefixes_ok N altered_ok N hostile_refused N sum S".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rmcv_amd/csrc/session_file.h"

static uint8_t* block(size_t n) { return static_cast<uint8_t*>(std::malloc(n ? n : 1)); }
static int fail(const char* what) { std::fprintf(stderr, "%s\n", what); return 5; }

// what rmcv_session_entry / _frame / _loop read of a parsed session, and what a reader of a loop record reads behind its fixed part
static unsigned walk(const uint8_t* data, const std::vector<SessionRec>& recs)
{
    unsigned sum = 0;
    for (const SessionRec& r : recs) {
        rmcv_record_entry e;
        std::memcpy(&e, data + r.entry, sizeof(e));
        for (int i = 0; i < e.user_bytes; i++) sum += data[r.user + i];
        for (int k = 0; k < e.n_frames; k++)
            for (int64_t i = 0; i < e.sizes[k]; i++) sum += data[r.frame[k] + i];
        for (int k = 0; k < e.n_frames && e.loop_bytes; k++) {
            const uint8_t* rec = data + r.loop + (int64_t)k * e.loop_bytes;
            rmcv_loop_state st;
            std::memcpy(&st, rec, sizeof(st));
            for (int64_t i = 0; i < e.loop_bytes; i++) sum += rec[i];
            for (int j = 0; j < st.n_tracks; j++) sum += rec[loop_track_at(j)] + rec[loop_side_at(j) + LOOP_SIDE_BYTES - 1]; // (inside the area: parse has checked n_tracks)
        }
    }
    return sum;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 1;
    const int w = 40, h = 3, lag = 3, cap = 2;
    uint8_t* plane = block((size_t)w * h);
    for (int i = 0; i < w * h; i++) plane[i] = (uint8_t)(i * 7 + (i >> 3));
    int64_t size = 0;
    uint8_t* packed = block((size_t)pack_bound(w, h));
    if (pack_host(plane, w, h, w, lag, packed, pack_bound(w, h), &size) != RMCV_OK) return fail("pack_host failed");
    const int64_t lb = loop_bound(cap);
    if (lb <= 0 || loop_cap_of(lb) != cap || loop_cap_of(lb + 8) != -1 || loop_cap_of(0) != -1 || loop_cap_of(-lb) != -1) return fail("loop_bound / loop_cap_of");
    uint8_t* loops[3];
    for (int r = 0; r < 3; r++) {
        loops[r] = block((size_t)lb);
        std::memset(loops[r], 0, (size_t)lb);
        rmcv_loop_state st;
        std::memset(&st, 0, sizeof(st));
        st.stream = r, st.n_tracks = st.n_tracking = r % (cap + 1), st.n_armours = 1, st.has_aim = 1, st.tracker_config.track_cap = 4;
        std::memcpy(loops[r], &st, sizeof(st));
        for (int64_t i = (int64_t)sizeof(st); i < loop_bound(st.n_tracks); i++) loops[r][i] = (uint8_t)(i + r);
    }
    {
        std::FILE* f = std::fopen(argv[1], "wb");
        if (!f || session_write_header(f) != RMCV_OK) return fail("session header");
        for (int t = 0; t < 2; t++) {
            rmcv_record_entry e;
            std::memset(&e, 0, sizeof(e));
            e.ticket = e.sequence = (uint64_t)t;
            e.n_frames = 2 - t, e.batch_frames = 2, e.w = e.w_bytes = e.stride = w, e.h = h, e.lag = lag, e.input_format = -1, e.sample_bits = 8;
            e.user_bytes = 3 + t, e.loop_bytes = (int32_t)lb;
            const uint8_t* frames[2] = {packed, packed};
            const uint8_t* lp[2] = {loops[2 * t], loops[1]};
            for (int k = 0; k < e.n_frames; k++) e.sizes[k] = size;
            if (session_write_record(f, e, "user", frames, lp) != RMCV_OK) return fail("session record");
            if (t == 0 && session_write_record(f, e, "user", frames, nullptr) != RMCV_ERR_BAD_ARG) return fail("a record with loop_bytes and no loop records was written");
        }
        if (std::fclose(f) != 0) return 3;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const long total = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t* file = block((size_t)total);
    if (std::fread(file, 1, (size_t)total, f) != (size_t)total) return 3;
    std::fclose(f);
    int prefixes_ok = 0, altered_ok = 0, hostile_refused = 0;
    unsigned sum = 0;
    std::vector<SessionRec> recs;
    for (long len = 0; len <= total; len++) {
        uint8_t* cut = block((size_t)len);
        std::memcpy(cut, file, (size_t)len);
        const int rc = session_parse(cut, len, &recs);
        if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("session_parse: a prefix returned something else");
        if (rc == RMCV_OK) { prefixes_ok++; sum += walk(cut, recs); }
        std::free(cut);
    }
    if (session_parse(file, total, &recs) != RMCV_OK || recs.size() != 2) return fail("the whole file does not parse");
    // the bytes to alter: the first record's length word and entry, then the fixed part of each loop record
    std::vector<long> at;
    for (long a = SESSION_HEAD; a < (long)(SESSION_HEAD + 8 + sizeof(rmcv_record_entry)); a++) at.push_back(a);
    for (const long first : {(long)recs[0].loop, (long)(recs[0].loop + lb), (long)recs[1].loop})
        for (long a = 0; a < (long)sizeof(rmcv_loop_state); a++) at.push_back(first + a);
    for (const long a : at)
        for (unsigned x : {0x01u, 0x80u, 0xFFu}) {
            uint8_t* alt = block((size_t)total);
            std::memcpy(alt, file, (size_t)total);
            alt[a] ^= (uint8_t)x;
            const int rc = session_parse(alt, total, &recs);
            if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("session_parse: an altered byte returned something else");
            if (rc == RMCV_OK) { altered_ok++; sum += walk(alt, recs); }
            std::free(alt);
        }
    // hostile counts: a record of exactly the fixed part's size, n_tracks negative or beyond any area
    for (const int32_t n : {-1, INT32_MIN, RMCV_TRACKER_MAX_CAP + 1, INT32_MAX, 0}) {
        uint8_t* rec = block(sizeof(rmcv_loop_state));
        rmcv_loop_state st;
        std::memset(&st, 0, sizeof(st));
        st.n_tracks = st.n_tracking = n, st.has_aim = st.has_attitude = 1, st.n_armours = 1;
        std::memcpy(rec, &st, sizeof(st));
        rmcv_tracker_config tc;
        rmcv_aim_config ac;
        rmcv_attitude_config tt;
        double g[16];
        int32_t has = 0;
        const int rcs[3] = {loop_tracker_config(rec, &tc), loop_aim_config(rec, &ac, &has), loop_attitude_config(rec, &tt, g, &has)};
        for (const int rc : rcs) {
            if (rc != (n == 0 ? RMCV_OK : RMCV_ERR_BAD_ARG)) return fail("an extractor took a hostile count");
            hostile_refused += rc == RMCV_ERR_BAD_ARG;
        }
        if (loop_counts_ok(&st, lb) != (n == 0)) return fail("loop_counts_ok took a hostile count");
        // the rule reads the fixed parts alone, whatever the counts say
        rmcv_loop_state p, c;
        std::memcpy(&p, rec, sizeof(p));
        std::memcpy(&c, rec, sizeof(c));
        c.n_armours = 0;
        rmcv_trigger_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        if (loop_trigger(&p, &c, &cfg) != RMCV_TRIG_NO_ARMOURS) return fail("loop_trigger on a hostile record");
        std::free(rec);
    }
    std::printf("prefixes_ok %d altered_ok %d hostile_refused %d sum %u\n", prefixes_ok, altered_ok, hostile_refused, sum);
    std::free(file); std::free(plane); std::free(packed);
    for (int r = 0; r < 3; r++) std::free(loops[r]);
    return 0;
}
