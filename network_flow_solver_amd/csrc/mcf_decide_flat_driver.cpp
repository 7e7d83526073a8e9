// mcf_decide_flat_driver.cpp -- stand-alone program round mcf_decide_flat_host.cpp, test infrastructure only: built together with
// that file, with the compiler's address / undefined-behaviour checks, by tests/test_small_loop_decide_cpu.py.
//
// usage: driver.  Runs the whole enumeration, prints its counts on one line and returns 0 when mcf_pivot_decide_flat left the
// control block of mcf_pivot_decide in every case.
#include <cstdint>
#include <cstdio>

extern "C" int mcf_decide_flat_sweep_host(int64_t* counts);

int main() {
    int64_t counts[24];
    const int rc = mcf_decide_flat_sweep_host(counts);
    for (int i = 0; i < 24; ++i) std::printf(i ? " %lld" : "%lld", (long long)counts[i]);
    std::printf("\n");
    return rc == 0 ? 0 : 1;
}
