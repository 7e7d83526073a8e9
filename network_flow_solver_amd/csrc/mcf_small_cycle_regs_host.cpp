// mcf_small_cycle_regs_host.cpp -- host restatement of the fused LDS loop's even deal of the Dantzig register sweep, test
// infrastructure only.
//
// solve_small_body (mcf_engine.hip) deals the arcs of a Dantzig sweep evenly over the lanes of the workgroup: the lane-to-arc map
// and the number of unrolled register slots a sweep executes are the MCF_HD functions mcf_even_* of mcf_core.h.  This file calls the
// very same functions round plain loops over `threads` "lanes", in the order of the device code -- the register slots first, the
// arcs from slot `reg` on in the loop that prices them from LDS -- so the CPU test-suite can check that every arc is priced exactly
// once and that the slot a lane hands over unpacks to the arc it priced.  It is NOT a CPU path of the library: nothing in the
// package loads it.
#include <cstdint>

#include "mcf_core.h"

extern "C" {

// One sweep over the engine arcs [base, base + arcs) by `threads` lanes with `reg` register slots per lane, compiled for `few` and
// `reg` slots.  times[i]: how often arc base + i was priced; lane_of[i] / slot_of[i]: the lane and the slot (as small_info carries
// it) of its last pricing; from_lds[i]: 1 when the LDS loop priced it.  *slots_out: the unrolled register slots executed,
// *masked_out: executed register slots over all lanes that held no arc.  Returns 0, -1 on bad arguments, -2 when a slot does
// not unpack to its arc or a lane prices outside the range.
int mcf_small_even_deal_host(int32_t base, int32_t arcs, int32_t threads, int32_t few, int32_t reg, int32_t* times, int32_t* lane_of,
                             int32_t* slot_of, int32_t* from_lds, int32_t* slots_out, int64_t* masked_out) {
    if (base < 0 || arcs < 0 || threads <= 0 || few <= 0 || few > reg || !slots_out || !masked_out) return -1;
    if (arcs > 0 && (!times || !lane_of || !slot_of || !from_lds)) return -1;
    const int32_t r_hi = base + arcs;
    const int32_t ns = mcf_even_reg_slots(arcs, threads, few, reg);   // (uniform: a constant of the launch)
    int64_t masked = 0;
    for (int32_t t = 0; t < threads; ++t) {
        const int32_t r_lo = mcf_even_arc(base, t, 0, threads);
        int32_t r_n = 0;   // slots in use, as the prologue counts them over all `reg` slots
        for (int32_t k = 0; k < reg; ++k) r_n += mcf_even_arc(base, t, k, threads) < r_hi ? 1 : 0;
        for (int32_t k = 0; k < ns; ++k) {
            if (!(k < r_n)) { ++masked; continue; }   // (priced with its state masked to 0: never a winner)
            const int32_t i = mcf_even_arc(base, t, k, threads);
            if (i < base || i >= r_hi || r_lo + k * threads != i) return -2;
            times[i - base] += 1; lane_of[i - base] = t; slot_of[i - base] = k; from_lds[i - base] = 0;
        }
        int32_t q = reg;
        for (int32_t i = r_lo + reg * threads; i < r_hi; i += threads, ++q) {
            if (i < base || r_lo + q * threads != i) return -2;
            times[i - base] += 1; lane_of[i - base] = t; slot_of[i - base] = q; from_lds[i - base] = 1;
        }
    }
    *slots_out = ns;
    *masked_out = masked;
    return 0;
}

int32_t mcf_small_even_slots_host(int32_t arcs, int32_t threads) { return mcf_even_slots(arcs, threads); }

}  // extern "C"
