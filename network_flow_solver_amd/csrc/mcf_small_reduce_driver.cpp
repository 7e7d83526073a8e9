// mcf_small_reduce_driver.cpp -- stand-alone program round mcf_small_reduce_host.cpp, test infrastructure only: built together
// with that file, with the compiler's address / undefined-behaviour checks, by tests/test_small_loop_reduce_cpu.py.
//
// usage: driver CASE_FILE...   Each file holds cases back to back, little endian: int64 header[3] = kind, n, last; kind 0 (one
// side of the ratio test) is followed by int64 res[n], kind 1 (the arg-max of a wave) by uint64 packed[64].  Prints one line per
// case -- "r <d> <k> <narrow>" / "a <lane> <key> <stages>" -- and returns 0 when the 32-bit and the 64-bit path agree on every case.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int mcf_small_ratio_side_host(const int64_t* res, int32_t n, int32_t last, int32_t allow_narrow, int64_t* d_out, int32_t* k_out,
                                         int32_t* narrow_out);
extern "C" int mcf_small_argmax_host(const uint64_t* packed, int32_t staged, int32_t* lane_out, uint64_t* key_out, int32_t* stages_out);

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        int64_t h[3];
        while (std::fread(h, sizeof(int64_t), 3, f) == 3) {
            if (h[0] == 0 && h[1] >= 0 && h[1] < (1 << 20)) {
                std::vector<int64_t> res((size_t)h[1]);
                if (h[1] && std::fread(res.data(), sizeof(int64_t), res.size(), f) != res.size()) { std::fclose(f); return 2; }
                int64_t d[2] = {0, 0};
                int32_t k[2] = {0, 0}, narrow[2] = {0, 0};
                for (int w = 0; w < 2; ++w)
                    if (mcf_small_ratio_side_host(res.data(), (int32_t)h[1], (int32_t)h[2], w, &d[w], &k[w], &narrow[w]) != 0) bad = 1;
                if (d[0] != d[1] || k[0] != k[1] || narrow[0] != 0) bad = 1;
                std::printf("r %lld %d %d\n", (long long)d[1], k[1], narrow[1]);
            } else if (h[0] == 1) {
                uint64_t packed[64];
                if (std::fread(packed, sizeof(uint64_t), 64, f) != 64) { std::fclose(f); return 2; }
                int32_t lane[2] = {0, 0}, stages[2] = {0, 0};
                uint64_t key[2] = {0, 0};
                for (int w = 0; w < 2; ++w)
                    if (mcf_small_argmax_host(packed, w, &lane[w], &key[w], &stages[w]) != 0) bad = 1;
                if (lane[0] != lane[1] || key[0] != key[1] || stages[0] != 0) bad = 1;
                std::printf("a %d %llu %d\n", lane[1], (unsigned long long)key[1], stages[1]);
            } else {
                std::fprintf(stderr, "%s: malformed case\n", argv[a]);
                std::fclose(f);
                return 2;
            }
        }
        std::fclose(f);
    }
    return bad;
}
