// mcf_small_budget_driver.cpp -- stand-alone program round mcf_small_budget_host.cpp, test infrastructure only: built together
// with that file, with the compiler's address / undefined-behaviour checks, by tests/test_small_loop_budget_cpu.py.
//
// usage: driver   Runs the pair arithmetic for the tree sizes of the tests, the packed counts for every pair of the tests' counts
// over every placing in four waves, and whole twin solves of seeded instances made here (a ring with chords, capacities small
// enough for bound flips).  Prints one line per case; returns 0 when every case agrees.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int mcf_budget_pairs_host(int32_t n_nodes, int64_t m_pad, int64_t arcw_count, int32_t devex, int32_t depths, int64_t* out);
extern "C" int mcf_budget_counts_host(const int32_t* n1, const int32_t* n2, int32_t* sum1, int32_t* sum2);
extern "C" int mcf_budget_twin_host(int32_t n, int64_t m, const int32_t* tail, const int32_t* head, const int64_t* cost, const int64_t* cap,
                                    const int64_t* supply, int64_t max_pivots, int32_t finish_mode, int64_t* report);

int main() {
    int bad = 0;
    const int32_t trees[7] = {2, 3, 5, 64, 65, 257, 1370};
    for (int32_t nn : trees) {
        int64_t out[7];
        const int rc = mcf_budget_pairs_host(nn, 1024, 1024 + nn - 1, 0, 12, out);
        if (rc != 0 || out[1] != 0 || out[2] != 0 || out[0] == 0) bad = 1;
        std::printf("pairs %d: rc %d compared %lld mismatches %lld unaligned %lld\n", nn, rc, (long long)out[0], (long long)out[1], (long long)out[2]);
        if ((out[6] != 0) != (nn < 1370)) bad = 1;   // (only the bound itself is beyond every instance with arcs)
    }
    const int32_t counts[6] = {0, 1, 63, 64, 65, 1370};
    long long packed = 0;
    for (int32_t a : counts) for (int32_t b : counts) for (int wa = 0; wa < 4; ++wa) for (int wb = 0; wb < 4; ++wb) {
        // everything in one wave, or split over two
        int32_t n1[4] = {0, 0, 0, 0}, n2[4] = {0, 0, 0, 0}, s1 = -1, s2 = -1;
        n1[wa] = a - a / 2; n1[(wa + 1) % 4] += a / 2;
        n2[wb] = b - b / 3; n2[(wb + 2) % 4] += b / 3;
        if (mcf_budget_counts_host(n1, n2, &s1, &s2) != 0 || s1 != a || s2 != b) bad = 1;
        packed += 1;
    }
    std::printf("counts: %lld cases\n", packed);
    for (uint32_t seed = 1; seed <= 3; ++seed) {
        const int32_t n = 30 + 17 * (int32_t)seed;
        std::vector<int32_t> tail, head;
        std::vector<int64_t> cost, cap, supply((size_t)n, 0);
        uint32_t x = seed * 2654435761u;
        auto rnd = [&](uint32_t mod) { x = x * 1664525u + 1013904223u; return (x >> 8) % mod; };
        for (int32_t u = 0; u < n; ++u) {
            tail.push_back(u); head.push_back((u + 1) % n); cost.push_back(1 + rnd(50)); cap.push_back(2 + rnd(6));
            for (int c = 0; c < 3; ++c) { tail.push_back(u); head.push_back((u + 1 + (int32_t)rnd((uint32_t)n - 1)) % n); cost.push_back(1 + rnd(90)); cap.push_back(1 + rnd(4)); }
        }
        for (int32_t u = 0; u + 1 < n; u += 2) { const int64_t s = 1 + rnd(3); supply[(size_t)u] += s; supply[(size_t)((u * 7 + 3) % n)] -= s; }
        int64_t report[12];
        const int rc = mcf_budget_twin_host(n, (int64_t)tail.size(), tail.data(), head.data(), cost.data(), cap.data(), supply.data(), -1, (int32_t)(seed % 3), report);
        if (rc != 0 || report[6] != 0 || report[7] != 0 || report[0] == 0) bad = 1;
        std::printf("twin %u: rc %d pivots %lld swaps %lld flips %lld first %lld second %lld cur1 %lld bad_ctx %lld bad_arrays %lld status %lld\n", seed, rc,
                    (long long)report[0], (long long)report[1], (long long)report[2], (long long)report[3], (long long)report[4], (long long)report[5],
                    (long long)report[6], (long long)report[7], (long long)report[8]);
    }
    return bad;
}
