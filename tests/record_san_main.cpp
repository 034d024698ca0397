// TEST-ONLY stand-alone program around the host side of the session recorder -- rmcv_amd/csrc/device_pack.h (pack_host, unpack_host) and
// rmcv_amd/csrc/session_file.h (the session file's writer and reader) -- for a sanitizer build (tests/test_record_sanitized.py:
// -fsanitize=address,undefined; no GPU, nothing loaded into python).  Every buffer is a heap block of exactly its size, so a read or write
// too far shows.
//   record_san_main IN OUT SESSION
// IN : int32 n_cases, then per case: int32 w_bytes, h, stride, lag; uint8 plane[h][stride]
// OUT: per case: int64 size; uint8 packed[size]          (compared with the numpy restatement by the test)
// Then, on the LAST case's packed frame and on a session file of two records written to SESSION:
//   unpack_host / session_parse on every prefix length, and with single bytes of header, row table, length word and entry altered.
// Every call must return RMCV_OK or RMCV_ERR_BAD_ARG; stdout: "frame_prefixes_ok N  frame_altered_ok N  session_prefixes_ok N  session_altered_ok N".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rmcv_amd/csrc/session_file.h"

static uint8_t* block(size_t n) { return static_cast<uint8_t*>(std::malloc(n ? n : 1)); }
static void get(std::FILE* f, void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }
static int fail(const char* what) { std::fprintf(stderr, "%s\n", what); return 5; }

// what rmcv_session_entry / rmcv_session_frame read of a parsed session: every byte the offsets promise
static unsigned walk(const uint8_t* data, const std::vector<SessionRec>& recs)
{
    unsigned sum = 0;
    for (const SessionRec& r : recs) {
        rmcv_record_entry e;
        std::memcpy(&e, data + r.entry, sizeof(e));
        for (int i = 0; i < e.user_bytes; i++) sum += data[r.user + i];
        for (int k = 0; k < e.n_frames; k++)
            for (int64_t i = 0; i < e.sizes[k]; i++) sum += data[r.frame[k] + i];
    }
    return sum;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t cases = 0;
    get(in, &cases, 4);
    uint8_t* last = nullptr; // the last case's packed frame and plane
    uint8_t* last_plane = nullptr;
    int64_t last_size = 0;
    int lw = 0, lh = 0, llag = 0;
    for (int32_t c = 0; c < cases; c++) {
        int32_t hd[4];
        get(in, hd, 16);
        const int w = hd[0], h = hd[1], stride = hd[2], lag = hd[3];
        uint8_t* plane = block((size_t)h * stride);
        get(in, plane, (size_t)h * stride);
        // the size first (a block of the bound), then once more into a block of exactly that size
        int64_t size = 0, again = 0;
        uint8_t* big = block((size_t)pack_bound(w, h));
        if (pack_host(plane, w, h, stride, lag, big, pack_bound(w, h), &size) != RMCV_OK) return fail("pack_host failed");
        uint8_t* packed = block((size_t)size);
        if (pack_host(plane, w, h, stride, lag, packed, size, &again) != RMCV_OK || again != size) return fail("pack_host into an exact block failed");
        if (pack_host(plane, w, h, stride, lag, packed, size - 8, &again) != RMCV_ERR_CAPACITY)
            return fail("pack_host did not report a block that is too small");
        if (pack_host(plane, w, h, stride, lag, packed, size, &again) != RMCV_OK) return fail("pack_host failed the second time");
        uint8_t* back = block((size_t)h * w);
        if (unpack_host(packed, size, w, h, lag, back, w) != RMCV_OK) return fail("unpack_host refused what pack_host wrote");
        for (int y = 0; y < h; y++)
            if (std::memcmp(back + (size_t)y * w, plane + (size_t)y * stride, (size_t)w) != 0) return fail("the round trip differs");
        if (std::fwrite(&size, 8, 1, out) != 1 || std::fwrite(packed, 1, (size_t)size, out) != (size_t)size) return 3;
        std::free(big);
        std::free(back);
        if (c == cases - 1) {
            last = packed, last_plane = plane, last_size = size, lw = w, lh = h, llag = lag;
            // (the plane was read with its stride; the fuzz below unpacks to tight rows)
        } else {
            std::free(packed);
            std::free(plane);
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0 || !last) return 3;

    // ---- the packed frame: every prefix, then single bytes of header and row table altered
    int frame_prefixes_ok = 0, frame_altered_ok = 0;
    uint8_t* dst = block((size_t)lh * lw);
    for (int64_t len = 0; len <= last_size; len++) {
        uint8_t* cut = block((size_t)len);
        std::memcpy(cut, last, (size_t)len);
        const int rc = unpack_host(len ? cut : nullptr, len, lw, lh, llag, dst, lw);
        if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("unpack_host: a prefix returned something else");
        frame_prefixes_ok += rc == RMCV_OK;
        std::free(cut);
    }
    const int64_t head = pack_header_bytes(lw, lh) + pack_table_bytes(lh);
    for (int64_t at = 0; at < head; at++)
        for (unsigned x : {0x01u, 0x08u, 0x10u, 0x80u, 0xFFu}) {
            uint8_t* alt = block((size_t)last_size);
            std::memcpy(alt, last, (size_t)last_size);
            alt[at] ^= (uint8_t)x;
            const int rc = unpack_host(alt, last_size, lw, lh, llag, dst, lw);
            if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("unpack_host: an altered byte returned something else");
            frame_altered_ok += rc == RMCV_OK;
            std::free(alt);
        }

    // ---- a session file of two records: every prefix, then single bytes of the first record's length word and entry altered
    {
        std::FILE* f = std::fopen(argv[3], "wb");
        if (!f || session_write_header(f) != RMCV_OK) return fail("session header");
        for (int t = 0; t < 2; t++) {
            rmcv_record_entry e;
            std::memset(&e, 0, sizeof(e));
            e.ticket = e.sequence = (uint64_t)t;
            e.n_frames = 1 + t, e.batch_frames = 2, e.w = e.w_bytes = e.stride = lw, e.h = lh, e.lag = llag, e.input_format = -1, e.sample_bits = 8;
            e.user_bytes = 3 + t;
            const uint8_t* frames[2] = {last, last};
            for (int k = 0; k < e.n_frames; k++) e.sizes[k] = last_size;
            if (session_write_record(f, e, "user", frames) != RMCV_OK) return fail("session record");
        }
        if (std::fclose(f) != 0) return 3;
    }
    std::FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const long total = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t* file = block((size_t)total);
    get(f, file, (size_t)total);
    std::fclose(f);
    int session_prefixes_ok = 0, session_altered_ok = 0;
    unsigned sum = 0;
    std::vector<SessionRec> recs;
    for (long len = 0; len <= total; len++) {
        uint8_t* cut = block((size_t)len);
        std::memcpy(cut, file, (size_t)len);
        const int rc = session_parse(cut, len, &recs);
        if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("session_parse: a prefix returned something else");
        if (rc == RMCV_OK) { session_prefixes_ok++; sum += walk(cut, recs); }
        std::free(cut);
    }
    for (long at = 0; at < (long)(SESSION_HEAD + 8 + sizeof(rmcv_record_entry)); at++)
        for (unsigned x : {0x01u, 0x80u, 0xFFu}) {
            uint8_t* alt = block((size_t)total);
            std::memcpy(alt, file, (size_t)total);
            alt[at] ^= (uint8_t)x;
            const int rc = session_parse(alt, total, &recs);
            if (rc != RMCV_OK && rc != RMCV_ERR_BAD_ARG) return fail("session_parse: an altered byte returned something else");
            if (rc == RMCV_OK) { session_altered_ok++; sum += walk(alt, recs); }
            std::free(alt);
        }
    std::printf("frame_prefixes_ok %d frame_altered_ok %d session_prefixes_ok %d session_altered_ok %d sum %u\n", frame_prefixes_ok, frame_altered_ok,
                session_prefixes_ok, session_altered_ok, sum);
    std::free(dst); std::free(file); std::free(last); std::free(last_plane);
    return 0;
}
