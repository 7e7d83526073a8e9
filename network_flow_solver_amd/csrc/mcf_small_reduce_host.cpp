// mcf_small_reduce_host.cpp -- host restatement of the fused LDS loop's 32-bit reductions, test infrastructure only.
//
// small_ratio_side and the front kernel's arg-max (mcf_engine.hip) reduce over the 64 lanes of a wave with DPP steps; the
// arithmetic round those steps -- which sides are narrow, the 32-bit key of a residual and its way back, the winner out of the
// ballot, the two stages of the arg-max -- is the MCF_HD functions of mcf_core.h.  This file calls the very same functions round
// plain loops over an array of 64 "lanes", in the order of the device code, so the CPU test-suite can hold them against a direct
// 64-bit statement of the rule.  It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>

#include "mcf_core.h"

namespace {
constexpr int kLanes = 64;

template <bool LAST>
void ratio_side(const int64_t* res, int32_t n, bool allow_narrow, int64_t* d_out, int32_t* k_out, int32_t* narrow_out) {
    int64_t d = MCF_INF;
    int32_t k = -1;
    *narrow_out = 0;
    if (allow_narrow) {
        bool wide[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const int64_t r0 = lane < n ? res[lane] : MCF_INF;
            wide[lane] = !mcf_ratio_narrow_ok(r0);
            for (int32_t i = 64 + lane; i < n; i += 64) wide[lane] |= !mcf_ratio_narrow_ok(res[i]);
        }
        uint64_t ballot = 0;
        for (int lane = 0; lane < kLanes; ++lane) ballot |= (uint64_t)wide[lane] << lane;
        if (ballot == 0) {
            for (int32_t base = 0; base < n; base += 64) {
                uint32_t key[kLanes], mn = 0xffffffffu;
                for (int lane = 0; lane < kLanes; ++lane) {
                    const int32_t i = base + lane;
                    key[lane] = mcf_ratio_key32(i < n ? res[i] : MCF_INF);
                    if (key[lane] < mn) mn = key[lane];   // (the wave's v_min_u32 steps)
                }
                uint64_t mask = 0;
                for (int lane = 0; lane < kLanes; ++lane) mask |= (uint64_t)(base + lane < n && key[lane] == mn) << lane;
                mcf_ratio_take<LAST>(mcf_ratio_unkey32(mn), mask, base, d, k);
            }
            *d_out = d; *k_out = k; *narrow_out = 1;
            return;
        }
    }
    for (int32_t base = 0; base < n; base += 64) {
        int64_t r[kLanes], mn = INT64_MAX;
        for (int lane = 0; lane < kLanes; ++lane) {
            const int32_t i = base + lane;
            r[lane] = i < n ? res[i] : INT64_MAX;
            if (r[lane] < mn) mn = r[lane];
        }
        uint64_t mask = 0;
        for (int lane = 0; lane < kLanes; ++lane) mask |= (uint64_t)(r[lane] == mn) << lane;
        mcf_ratio_take<LAST>(mn, mask, base, d, k);
    }
    *d_out = d; *k_out = k;
}
}  // namespace

extern "C" {

// One side of the ratio test over res[0 .. n) as small_ratio_side<last> runs it.  narrow_out: 1 when the 32-bit path ran.
int mcf_small_ratio_side_host(const int64_t* res, int32_t n, int32_t last, int32_t allow_narrow, int64_t* d_out, int32_t* k_out,
                              int32_t* narrow_out) {
    if (n < 0 || (n > 0 && !res) || !d_out || !k_out || !narrow_out) return -1;
    if (last) ratio_side<true>(res, n, allow_narrow != 0, d_out, k_out, narrow_out);
    else ratio_side<false>(res, n, allow_narrow != 0, d_out, k_out, narrow_out);
    return 0;
}

// The front kernel's per-wave arg-max over packed[0 .. 64) = (violation << 32) | ~id per lane (violation 0: nothing eligible).
// lane_out: the lane that writes the wave's slot, key_out: the key it writes (0: nothing eligible), stages_out: 32-bit
// reductions run (staged) or 0 (one 64-bit maximum).  Returns -1 when not exactly one lane would write.
int mcf_small_argmax_host(const uint64_t* packed, int32_t staged, int32_t* lane_out, uint64_t* key_out, int32_t* stages_out) {
    if (!packed || !lane_out || !key_out || !stages_out) return -1;
    bool any, win[kLanes];
    *stages_out = 0;
    if (staged) {
        uint32_t vmx = 0;
        for (int lane = 0; lane < kLanes; ++lane) if (mcf_argmax_viol(packed[lane]) > vmx) vmx = mcf_argmax_viol(packed[lane]);
        *stages_out = 1;
        any = vmx != 0;
        uint64_t tied = 0;
        for (int lane = 0; lane < kLanes; ++lane) {
            win[lane] = mcf_argmax_viol(packed[lane]) == vmx;
            tied |= (uint64_t)win[lane] << lane;
        }
        if (any && (tied & (tied - 1))) {
            uint32_t imx = 0;
            for (int lane = 0; lane < kLanes; ++lane) if (mcf_argmax_second(packed[lane], vmx) > imx) imx = mcf_argmax_second(packed[lane], vmx);
            *stages_out = 2;
            for (int lane = 0; lane < kLanes; ++lane) win[lane] = win[lane] && (uint32_t)packed[lane] == imx;
        }
    } else {
        uint64_t mx = 0;   // (the device reduces the keys as signed values: a violation is below 2^31)
        for (int lane = 0; lane < kLanes; ++lane) if ((int64_t)packed[lane] > (int64_t)mx) mx = packed[lane];
        any = (mx >> 32) != 0;
        for (int lane = 0; lane < kLanes; ++lane) win[lane] = packed[lane] == mx;
    }
    int writers = 0;
    for (int lane = 0; lane < kLanes; ++lane) {
        if (any ? win[lane] : lane == 0) {
            ++writers;
            *lane_out = lane;
            *key_out = any ? packed[lane] : 0;
        }
    }
    return writers == 1 ? 0 : -1;
}

}  // extern "C"
