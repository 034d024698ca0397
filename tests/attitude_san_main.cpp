// TEST-ONLY stand-alone program around the host path of rmcv_amd/csrc/device_attitude.h, for a sanitizer build (tests/test_attitude_sanitized.py:
// -fsanitize=address,undefined; no GPU, nothing loaded into python).  Every table is a heap block of exactly its size, so a stream too far shows.
//   attitude_san_main IN OUT
// IN : int32 n, int32 rounds, int32 camps_on, int32 pose_tables, rmcv_attitude_config, rmcv_attitude[n], int32 camps[n], rmcv_aim_input[n],
//      then per round: int32 has_packets, uint8 packets[n][24] if so
// OUT: per round: rmcv_attitude[n], int32 camps[n], int32 packet_errors[n], double base2gripper[n][16] (if pose_tables), rmcv_aim_input[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rmcv_amd/csrc/device_attitude.h"

template <typename T> static T* block(size_t n) { return static_cast<T*>(std::calloc(n ? n : 1, sizeof(T))); }
template <typename T> static void get(std::FILE* f, T* p, size_t n) { if (std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }
template <typename T> static void put(std::FILE* f, const T* p, size_t n) { if (std::fwrite(p, sizeof(T), n, f) != n) std::exit(3); }

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int32_t head[4];
    get(in, head, 4);
    const size_t n = (size_t)head[0];
    const int rounds = head[1], camps_on = head[2], pose = head[3];
    rmcv_attitude_config cfg;
    get(in, &cfg, 1);
    if (att_check_config(&cfg)) return 4;
    rmcv_attitude* att = block<rmcv_attitude>(n);
    int32_t* camps = block<int32_t>(n);
    int32_t* errors = block<int32_t>(n);
    double* b2g = block<double>(n * 16);
    rmcv_aim_input* inputs = block<rmcv_aim_input>(n);
    uint8_t* packets = block<uint8_t>(n * RMCV_SERIAL_PACKET_BYTES);
    get(in, att, n);
    get(in, camps, n);
    get(in, inputs, n);
    for (int r = 0; r < rounds; r++) {
        int32_t has = 0;
        get(in, &has, 1);
        if (has) get(in, packets, n * RMCV_SERIAL_PACKET_BYTES);
        for (size_t f = 0; f < n; f++)
            att_stream(&cfg, has ? packets + f * RMCV_SERIAL_PACKET_BYTES : nullptr, &att[f], camps_on ? &camps[f] : nullptr, &errors[f],
                       pose ? b2g + f * 16 : nullptr, &inputs[f]);
        put(out, att, n);
        put(out, camps, n);
        put(out, errors, n);
        if (pose) put(out, b2g, n * 16);
        put(out, inputs, n);
    }
    std::free(att); std::free(camps); std::free(errors); std::free(b2g); std::free(inputs); std::free(packets);
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 3;
}
