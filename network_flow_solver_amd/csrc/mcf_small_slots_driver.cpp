// mcf_small_slots_driver.cpp -- stand-alone program round mcf_small_slots_host.cpp, test infrastructure only: built together with
// that file, with the compiler's address / undefined-behaviour checks, by tests/test_small_loop_slots_cpu.py.
//
// usage: driver CASE_FILE...   Each file holds cases back to back, little endian: int32 header[4] = kind, a, b, c.
//   kind 0 (violations): a pairs; int32 s[a], int32 rc[a].                       Prints "v <selects> <flat> <signed>" per pair.
//   kind 1 (one lane's sweep): a register slots, b arcs from LDS, c accumulators; with t = a + b: int32 st[t], rc[t], orig[t],
//           uint32 info[t].                                                      Prints "s <best> <info>".
//   kind 2 (the pick): uint32 words[16].                                         Prints "p <key> <arc> <rc> <tail> <head> <state>".
// Returns 0 when on every case the compare-free / one-trip form, the form the kernel had before and (kind 1) mcf_cand_better agree.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int mcf_slots_violation_host(const int32_t* s, const int32_t* rc, int32_t n, uint32_t* selects_out, uint32_t* flat_out, int32_t* signed_out);
extern "C" int mcf_slots_sweep_host(int32_t chains, int32_t ns, const int32_t* st, const int32_t* rc, const int32_t* orig, const uint32_t* info_inv,
                                    int32_t n_lds, uint64_t* best_out, uint32_t* info_out);
extern "C" int mcf_slots_pick_host(const uint32_t* words, int32_t flat, int64_t* out);

namespace {
template <typename T> bool rd(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        int32_t h[4];
        while (std::fread(h, sizeof(int32_t), 4, f) == 4) {
            if (h[0] == 0 && h[1] >= 0 && h[1] < (1 << 20)) {
                const size_t n = (size_t)h[1];
                std::vector<int32_t> s(n), rc(n), sg(n);
                std::vector<uint32_t> sel(n), flat(n);
                if (!rd(f, s) || !rd(f, rc)) { std::fclose(f); return 2; }
                if (mcf_slots_violation_host(s.data(), rc.data(), h[1], sel.data(), flat.data(), sg.data()) != 0) bad = 1;
                for (size_t i = 0; i < n; ++i) {
                    if (sel[i] != flat[i] || (uint32_t)(sg[i] > 0 ? sg[i] : 0) != sel[i]) bad = 1;
                    std::printf("v %u %u %d\n", sel[i], flat[i], sg[i]);
                }
            } else if (h[0] == 1 && h[1] >= 1 && h[1] <= 16 && h[2] >= 0 && h[2] < (1 << 16)) {
                const size_t t = (size_t)h[1] + (size_t)h[2];
                std::vector<int32_t> st(t), rc(t), orig(t);
                std::vector<uint32_t> info(t);
                if (!rd(f, st) || !rd(f, rc) || !rd(f, orig) || !rd(f, info)) { std::fclose(f); return 2; }
                uint64_t best[3] = {0, 0, 0};
                uint32_t inf[3] = {0, 0, 0};
                const int32_t forms[3] = {h[3], 0, -1};
                for (int w = 0; w < 3; ++w)
                    if (mcf_slots_sweep_host(forms[w], h[1], st.data(), rc.data(), orig.data(), info.data(), h[2], &best[w], &inf[w]) != 0) bad = 1;
                if (best[0] != best[1] || best[0] != best[2] || inf[0] != inf[1] || inf[0] != inf[2]) bad = 1;
                std::printf("s %llu %u\n", (unsigned long long)best[0], inf[0]);
            } else if (h[0] == 2) {
                std::vector<uint32_t> w(16);
                if (!rd(f, w)) { std::fclose(f); return 2; }
                int64_t out[2][7] = {{0}, {0}};
                for (int x = 0; x < 2; ++x) if (mcf_slots_pick_host(w.data(), x, out[x]) != 0) bad = 1;
                for (int j = 0; j < 7; ++j) if (out[0][j] != out[1][j]) bad = 1;
                std::printf("p %lld %lld %lld %lld %lld %lld\n", (long long)out[1][0], (long long)out[1][1], (long long)out[1][2], (long long)out[1][3],
                            (long long)out[1][4], (long long)out[1][5]);
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
