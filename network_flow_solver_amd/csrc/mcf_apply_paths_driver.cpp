// mcf_apply_paths_driver.cpp -- stand-alone program round mcf_apply_paths_run_host (mcf_apply_paths_host.cpp), test infrastructure
// only: built together with that file, with the compiler's address / undefined-behaviour checks, by tests/test_apply_paths_cpu.py.
//
// usage: driver CASE_FILE...   Each file is one case, little endian: int64 header[6] = n, m, rule, block_size, max_pivots,
// has_basis; then tail int32[m], head int32[m], cost int64[m], cap int64[m], supply int64[n] and, with has_basis, in_tree int8[m],
// at_upper int8[m].  Prints one line per case (the report) and returns 0 when no case shows a difference.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int32_t mcf_apply_paths_report_len();
extern "C" int mcf_apply_paths_run_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                                        const int64_t* supply, const int8_t* in_tree, const int8_t* at_upper, int32_t rule, int64_t block_size,
                                        int64_t max_pivots, int64_t* report, int64_t* flow, int64_t* pi, int32_t* parent, int32_t* depth);

namespace {
template <typename T>
bool read_n(std::FILE* f, std::vector<T>& out, size_t count) {
    out.resize(count);
    return count == 0 || std::fread(out.data(), sizeof(T), count, f) == count;
}
}  // namespace

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        int64_t h[6];
        std::vector<int32_t> tail, head;
        std::vector<int64_t> cost, cap, supply;
        std::vector<int8_t> in_tree, at_upper;
        bool ok = std::fread(h, sizeof(int64_t), 6, f) == 6 && h[0] >= 1 && h[0] < (1 << 20) && h[1] >= 0 && h[1] < (1 << 24);
        const size_t n = ok ? (size_t)h[0] : 0, m = ok ? (size_t)h[1] : 0;
        ok = ok && read_n(f, tail, m) && read_n(f, head, m) && read_n(f, cost, m) && read_n(f, cap, m) && read_n(f, supply, n);
        if (ok && h[5]) ok = read_n(f, in_tree, m) && read_n(f, at_upper, m);
        std::fclose(f);
        if (!ok) { std::fprintf(stderr, "%s: short or malformed case file\n", argv[a]); return 2; }
        std::vector<int64_t> report((size_t)mcf_apply_paths_report_len(), 0), flow(m, 0), pi(n + 1, 0);
        std::vector<int32_t> parent(n + 1, 0), depth(n + 1, 0);
        const int rc = mcf_apply_paths_run_host((int32_t)n, (int64_t)m, tail.data(), head.data(), cost.data(), cap.data(), supply.data(),
                                                h[5] ? in_tree.data() : nullptr, h[5] ? at_upper.data() : nullptr, (int32_t)h[2], h[3], h[4],
                                                report.data(), flow.data(), pi.data(), parent.data(), depth.data());
        std::printf("%s rc %d report", argv[a], rc);
        for (int64_t x : report) std::printf(" %lld", (long long)x);
        std::printf("\n");
        // report[4], [5], [13]: differing sources, differing states, a written segment table (mcf_apply_paths_host.cpp)
        if (rc != 0 || report[4] != 0 || report[5] != 0 || report[13] != 0) bad = 1;
    }
    return bad;
}
