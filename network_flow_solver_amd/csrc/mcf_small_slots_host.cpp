// mcf_small_slots_host.cpp -- host restatement of what the fused LDS loop's front kernel changed when it was budgeted in issue
// slots, test infrastructure only.
//
// The narrow register sweep (mcf_engine.hip: solve_small_body, small_price_flat) and the pick of the handing-over arg-max
// (small_handover_pick, small_pick_one_trip) do their arithmetic with the MCF_HD functions of mcf_core.h: mcf_narrow_violation*,
// mcf_narrow_key, mcf_narrow_start, mcf_narrow_pick, mcf_narrow_record.  This file calls the very same functions in the order of
// the device code -- a lane's slots dealt over its accumulators, the merge, the one compare with the start value, then the arcs
// priced from LDS -- next to the forms the kernel had before (two selects per violation, one serial chain of unsigned compares; a
// pick that branches on "anything eligible") and next to mcf_cand_better, so that the CPU test-suite can hold them against each
// other.  It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>

#include "mcf_core.h"

namespace {
constexpr int kMaxSlots = 16;

// what small_price_lds_narrow does with one arc beyond the register slots (both forms of the sweep end with it)
void lds_arc(int32_t st, int32_t rc, int32_t orig, uint32_t info_inv, uint64_t& best, uint32_t& info) {
    const uint64_t p = ((uint64_t)mcf_narrow_violation_selects(st, rc) << 32) | (uint32_t)~orig;
    if (p > best) { best = p; info = info_inv | ((uint32_t)st & 0x80000000u); }
}
}  // namespace

extern "C" {

// The violation of n (state, reduced cost) pairs in all three forms: selects_out the two-select form, flat_out the compare-free one
// clamped at 0, signed_out the compare-free one as the sweep uses it.
int mcf_slots_violation_host(const int32_t* s, const int32_t* rc, int32_t n, uint32_t* selects_out, uint32_t* flat_out, int32_t* signed_out) {
    if (n < 0 || (n > 0 && (!s || !rc || !selects_out || !flat_out || !signed_out))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        if (s[i] < -1 || s[i] > 1) return -1;
        selects_out[i] = mcf_narrow_violation_selects(s[i], rc[i]);
        flat_out[i] = mcf_narrow_violation(s[i], rc[i]);
        signed_out[i] = mcf_narrow_violation_signed(s[i], rc[i]);
    }
    return 0;
}

// One lane's sweep: ns register slots (a slot past the lane's last arc holds rc 0, id 0, info_inv as given and whatever state),
// then n_lds arcs priced from LDS.  chains >= 1: the compare-free form on that many accumulators (slot k goes to accumulator
// k % chains; merge; one compare with the start value); chains == 0: the serial chain of the two-select form; chains == -1:
// mcf_cand_better over (violation, packed id) -- the rule itself.  best_out: the packed key (high word 0: nothing eligible),
// info_out: the winner's info word (0 when nothing is eligible).
int mcf_slots_sweep_host(int32_t chains, int32_t ns, const int32_t* st, const int32_t* rc, const int32_t* orig, const uint32_t* info_inv,
                         int32_t n_lds, uint64_t* best_out, uint32_t* info_out) {
    if (ns < 1 || ns > kMaxSlots || n_lds < 0 || chains < -1 || chains > ns || !st || !rc || !orig || !info_inv || !best_out || !info_out) return -1;
    uint64_t nbest = (uint64_t)mcf_narrow_start();
    uint32_t info = 0;
    if (chains >= 1) {
        int64_t nb[kMaxSlots];
        uint32_t inf[kMaxSlots];
        for (int k = 0; k < ns; ++k) {
            const int64_t p = mcf_narrow_key(mcf_narrow_violation_signed(st[k], rc[k]), orig[k]);
            const int a = k % chains;
            if (k < chains || p > nb[a]) { nb[a] = p; inf[a] = info_inv[k] | ((uint32_t)st[k] & 0x80000000u); }
        }
        for (int a = 1; a < chains; ++a) if (nb[a] > nb[0]) { nb[0] = nb[a]; inf[0] = inf[a]; }
        if (!(nb[0] > mcf_narrow_start())) { nb[0] = mcf_narrow_start(); inf[0] = 0; }
        nbest = (uint64_t)nb[0]; info = inf[0];
    } else if (chains == 0) {
        for (int k = 0; k < ns; ++k) {
            const uint64_t p = ((uint64_t)mcf_narrow_violation_selects(st[k], rc[k]) << 32) | (uint32_t)~orig[k];
            if (p > nbest) { nbest = p; info = info_inv[k] | ((uint32_t)st[k] & 0x80000000u); }
        }
    } else {
        int64_t key = 0, arc = -1;
        for (int k = 0; k < ns + n_lds; ++k) {
            const int64_t viol = st[k] > 0 ? -(int64_t)rc[k] : (int64_t)rc[k];
            const int64_t pid = mcf_pack_arc(orig[k], k);
            if (st[k] != 0 && viol > 0 && mcf_cand_better(viol, pid, key, arc)) {
                key = viol; arc = pid;
                nbest = ((uint64_t)viol << 32) | (uint32_t)~orig[k];
                info = info_inv[k] | ((uint32_t)st[k] & 0x80000000u);
            }
        }
        *best_out = nbest; *info_out = info;
        return 0;
    }
    for (int k = ns; k < ns + n_lds; ++k) lds_arc(st[k], rc[k], orig[k], info_inv[k], nbest, info);
    *best_out = nbest; *info_out = info;
    return 0;
}

// `cases` sweeps of the same shape back to back (case c reads its ns + n_lds entries from c * (ns + n_lds) on).
int mcf_slots_sweep_batch_host(int32_t chains, int32_t ns, int32_t n_lds, int64_t cases, const int32_t* st, const int32_t* rc, const int32_t* orig,
                               const uint32_t* info_inv, uint64_t* best_out, uint32_t* info_out) {
    if (cases < 0 || ns < 1 || n_lds < 0) return -1;
    const int64_t t = (int64_t)ns + n_lds;
    for (int64_t c = 0; c < cases; ++c)
        if (mcf_slots_sweep_host(chains, ns, st + c * t, rc + c * t, orig + c * t, info_inv + c * t, n_lds, best_out + c, info_out + c) != 0) return -1;
    return 0;
}

// The pick over four per-wave slots of four words each (mcf_narrow_pick's layout).  flat != 0: mcf_narrow_pick; flat == 0: the
// form that branches on "anything eligible" and leaves the empty record alone.  out[7]: key, arc, rc, tail, head, state, pad.
int mcf_slots_pick_host(const uint32_t* words, int32_t flat, int64_t* out) {
    if (!words || !out) return -1;
    int64_t key = 0, arc = -1;
    McfCandX wx;
    wx.rc = 0; wx.arc = -1; wx.tail = 0; wx.head = 0; wx.state = 0; wx.pad = 0;
    if (flat) {
        uint32_t w[4][4];
        for (int q = 0; q < 4; ++q) for (int j = 0; j < 4; ++j) w[q][j] = words[4 * q + j];
        mcf_narrow_pick<4>(w, key, arc, wx);
    } else {
        int b = 0;
        auto k64 = [&](int q) { return ((uint64_t)words[4 * q + 1] << 32) | words[4 * q]; };
        for (int q = 1; q < 4; ++q) if (k64(q) > k64(b)) b = q;
        key = (int64_t)(k64(b) >> 32);
        if (key > 0) {
            wx = mcf_narrow_record(words[4 * b + 3], key, (int32_t)~words[4 * b], (int32_t)words[4 * b + 2]);
            arc = wx.arc;
        } else { key = 0; arc = -1; }
    }
    out[0] = key; out[1] = arc; out[2] = wx.rc; out[3] = wx.tail; out[4] = wx.head; out[5] = wx.state; out[6] = wx.pad;
    return wx.arc == arc || arc == -1 ? 0 : -1;
}

}  // extern "C"
