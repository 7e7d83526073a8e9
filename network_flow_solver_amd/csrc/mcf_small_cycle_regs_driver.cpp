// mcf_small_cycle_regs_driver.cpp -- stand-alone program round mcf_small_cycle_regs_host.cpp, test infrastructure only: built
// together with that file, with the compiler's address / undefined-behaviour checks, by tests/test_small_loop_regs_cpu.py.
//
// usage: driver BASE ARCS THREADS FEW REG ...   (five numbers per case).  Prints one line per case -- "<slots> <masked> <from LDS>
// <slot of the last arc>" -- and returns 0 when every arc of every case was priced exactly once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int mcf_small_even_deal_host(int32_t base, int32_t arcs, int32_t threads, int32_t few, int32_t reg, int32_t* times,
                                        int32_t* lane_of, int32_t* slot_of, int32_t* from_lds, int32_t* slots_out, int64_t* masked_out);

int main(int argc, char** argv) {
    if ((argc - 1) % 5 != 0) { std::fprintf(stderr, "five numbers per case\n"); return 2; }
    int bad = 0;
    for (int a = 1; a + 4 < argc; a += 5) {
        const int32_t base = (int32_t)std::atol(argv[a]), arcs = (int32_t)std::atol(argv[a + 1]), threads = (int32_t)std::atol(argv[a + 2]);
        const int32_t few = (int32_t)std::atol(argv[a + 3]), reg = (int32_t)std::atol(argv[a + 4]);
        if (arcs < 0 || arcs > (1 << 24)) return 2;
        std::vector<int32_t> times((size_t)arcs, 0), lane((size_t)arcs, -1), slot((size_t)arcs, -1), lds((size_t)arcs, -1);
        int32_t slots = 0;
        int64_t masked = 0;
        if (mcf_small_even_deal_host(base, arcs, threads, few, reg, times.data(), lane.data(), slot.data(), lds.data(), &slots, &masked) != 0) {
            bad = 1;
            continue;
        }
        int64_t from_lds = 0;
        for (int32_t i = 0; i < arcs; ++i) {
            if (times[(size_t)i] != 1 || lane[(size_t)i] != i % threads) bad = 1;
            from_lds += lds[(size_t)i];
        }
        std::printf("%d %lld %lld %d\n", slots, (long long)masked, (long long)from_lds, arcs ? slot[(size_t)arcs - 1] : -1);
    }
    return bad;
}
