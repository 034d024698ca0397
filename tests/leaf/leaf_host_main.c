/* TEST-ONLY stand-alone program, written in the common subset of C and C++ (tests/test_leaf_cpu.py):
 *   - built as C by `gcc -O2 -ffp-contract=off -fno-fast-math` it is the gcc build of the leaf functions, the build the CPU oracle and the
 *     tests' references are made with;
 *   - built as C++ by `g++ -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all` it is the sanitized run of the same loops.
 *   leaf_host_main IN OUT      (the files of tests/leaf/leaf_main.hip; OUT as under --host-only)
 */
#include <stdio.h>
#include <stdlib.h>

#include "leaf_funcs.h"

static void fail(const char* what)
{
    fprintf(stderr, "leaf_host_main: %s\n", what);
    exit(2);
}
static void get(FILE* f, void* p, size_t bytes) { if (bytes && fread(p, 1, bytes, f) != bytes) fail("short input"); }
static void put(FILE* f, const void* p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, f) != bytes) fail("short write"); }

int main(int argc, char** argv)
{
    static const int nargs_of[LEAF_N_FUNCS] = LEAF_NARGS_TABLE;
    FILE *in, *out;
    uint32_t head[2], out_head[4], r;
    if (argc != 3) fail("usage: leaf_host_main IN OUT");
    in = fopen(argv[1], "rb");
    out = fopen(argv[2], "wb");
    if (!in || !out) fail("cannot open the files");
    get(in, head, sizeof(head));
    if (head[0] != LEAF_MAGIC) fail("not a case file");
    out_head[0] = LEAF_MAGIC; out_head[1] = head[1]; out_head[2] = 0; out_head[3] = 0;
    put(out, out_head, sizeof(out_head));
    for (r = 0; r < head[1]; r++) {
        uint32_t rec[4], rec_out[2], k;
        uint64_t n, i, *a[LEAF_MAX_ARGS] = {0}, *res;
        const uint64_t* ptr[LEAF_MAX_ARGS] = {0};
        int fid;
        get(in, rec, sizeof(rec));
        get(in, &n, sizeof(n));
        fid = (int)rec[0];
        if (fid < 0 || fid >= LEAF_N_FUNCS || (int)rec[2] != nargs_of[fid] || n > (1u << 22)) fail("bad record");
        for (k = 0; k < rec[2]; k++) {
            a[k] = (uint64_t*)malloc((n ? n : 1) * 8);
            if (!a[k]) fail("out of memory");
            get(in, a[k], n * 8);
            ptr[k] = a[k];
        }
        res = (uint64_t*)malloc((n ? n : 1) * 8);
        if (!res) fail("out of memory");
        for (i = 0; i < n; i++) res[i] = leaf_eval(fid, ptr, i);
        rec_out[0] = rec[0]; rec_out[1] = 0;
        put(out, rec_out, sizeof(rec_out));
        put(out, &n, sizeof(n));
        put(out, res, n * 8);
        for (k = 0; k < rec[2]; k++) free(a[k]);
        free(res);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
