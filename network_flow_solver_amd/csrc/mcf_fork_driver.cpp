// mcf_fork_driver.cpp -- stand-alone program round mcf_fork_host.cpp, test infrastructure only: built together with that
// file, with the compiler's address / undefined-behaviour checks, by tests/test_fork_cpu.py.
//
// usage: driver   Runs the coverage check of the copy kernel's arithmetic over the segment lists, destination counts and
// grid sizes of the test (lengths 0, 1, 15, 16, 17, 4 (n + 1) for n = 64..67 and one segment longer than a grid's stride).
// The counters are allocated exactly: a write outside them is the sanitizer's to find.  Prints one line per case and
// returns 0 when every byte of every segment was written to every destination exactly once and nothing else was.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int mcf_fork_chunk_bytes_host(void);
extern "C" int mcf_fork_group_host(void);
extern "C" int mcf_fork_cover_host(int32_t nseg, const int64_t* bytes, int64_t count, int32_t grid, int64_t stride, uint8_t* writes,
                                   uint32_t* reads, int64_t* outside);

int main() {
    const int64_t chunk = mcf_fork_chunk_bytes_host();
    const int64_t group = mcf_fork_group_host();
    const int grids[] = {1, 3, 8, 64};
    const std::vector<int64_t> lens = {0, 1, 15, 16, 17, 4 * 65, 4 * 66, 4 * 67, 4 * 68, 0, 64 * chunk + 4 * 66 + 3, 16};
    int64_t longest = 0;
    for (int64_t b : lens) if (b > longest) longest = b;
    const int64_t stride = longest + 16;
    const int64_t counts[] = {1, 2, group + 1};
    int bad = 0;
    for (int64_t count : counts)
        for (int grid : grids) {
            std::vector<uint8_t> writes((size_t)(count * (int64_t)lens.size() * stride), 0);
            std::vector<uint32_t> reads((size_t)((int64_t)lens.size() * stride), 0);
            int64_t outside = -1;
            if (mcf_fork_cover_host((int32_t)lens.size(), lens.data(), count, grid, stride, writes.data(), reads.data(), &outside) != 0) return 2;
            int64_t wrong = 0;
            for (int64_t d = 0; d < count; ++d)
                for (size_t s = 0; s < lens.size(); ++s)
                    for (int64_t b = 0; b < stride; ++b)
                        if (writes[(size_t)((d * (int64_t)lens.size() + (int64_t)s) * stride + b)] != (b < lens[s] ? 1 : 0)) ++wrong;
            std::printf("count %lld grid %d: wrong %lld outside %lld\n", (long long)count, grid, (long long)wrong, (long long)outside);
            if (wrong || outside) bad = 1;
        }
    return bad;
}
