// mcf_decide_flat_host.cpp -- mcf_pivot_decide_flat against mcf_pivot_decide on the host, test infrastructure only.
//
// The fused LDS loop's 256-lane front kernel decides a pivot with mcf_pivot_decide_flat (mcf_core.h), a second statement of
// mcf_pivot_decide + mcf_pivot_swap for the dense layout without Devex weights that selects where the first one returns.  The
// contract is that from the same control block, cycle and path arrays it leaves every byte of the control block that
// mcf_pivot_decide leaves.  This file runs the two MCF_HD functions from the same start over an enumeration of starts and compares
// the two control blocks with memcmp.  Everything a pivot's descriptor holds starts as non-zero junk, so that "keeps what it had"
// is really checked.  It is NOT a CPU path of the library: nothing in the package loads it.
#include <cstdint>
#include <cstring>

#include "mcf_core.h"

namespace {

const int64_t kBig = ((int64_t)1 << 32);
const int64_t kResiduals[6] = {0, 1, 5, kBig - 2, kBig + 5, MCF_INF};
const int32_t kSide = 4;     // recorded path elements per side: indices 0, 1 and the last one (3) leave
const int32_t kA0 = 20;      // old position of the leaving node

// Where the new parent sits against the re-hung subtree [kA0, kA0 + S): (position, subtree size) of the entering arc's end
// point that becomes v_in.  tA = pos + 1, tB = pos + size.
struct Place { int32_t pos, size_base, size_per_s; };
const Place kPlaces[7] = {
    {10, 1, 0},     // tA == tB, in front of T2
    {10, 5, 0},     // tB is nearer, in front of T2
    {30, 5, 0},     // tA is nearer, behind T2
    {10, 40, 0},    // tA in front, tB far behind: tA
    {10, 10, 1},    // tB == kA0 + S: T2 ends v_in's block already and stays where it is
    {10, 19, 1},    // tA in front and tB behind at the same distance: the tie goes to tA
    {5, 17, 1},     // tB two behind T2's end, tA far in front: tB
};

struct Case {
    int64_t d1, d2, cap;
    int32_t s, parity, S, kpos, minus, place;
};

// A control block of junk: every 32-bit word in [1, 2^20], so that the 64-bit counters can still be added to.
void junk_ctx(McfCtx* c, uint32_t seed) {
    uint32_t words[sizeof(McfCtx) / 4];
    for (size_t i = 0; i < sizeof(McfCtx) / 4; ++i) {
        seed = seed * 1664525u + 1013904223u;
        words[i] = 1u + ((seed >> 8) & 0xfffffu);
    }
    std::memcpy(c, words, sizeof(McfCtx));
}

// Runs one case; returns 0 when the two control blocks agree, else 1 + the first differing byte.  *ref_out: what
// mcf_pivot_decide left.
int run_case(const Case& q, McfCtx* ref_out, int32_t* k_leave) {
    McfCtx start;
    junk_ctx(&start, 12345u + (uint32_t)q.place * 7919u + (uint32_t)q.kpos);
    // as mcf_pivot_begin_t leaves it
    start.status = MCF_RUNNING;
    start.apply = 0; start.stage = 0; start.nchg = 0;
    start.pv_e = 77; start.pv_s = q.s; start.pv_first = 41; start.pv_second = 42;
    start.pv_rc = q.s > 0 ? -9 : 9;
    start.pv_cap = q.cap;

    // which side the reference's order picks (only to put -1 on the side that does not leave)
    const int leaves = (q.d2 <= q.cap && q.d2 <= q.d1) ? 2 : (q.cap <= q.d1 ? 0 : 1);
    McfCycle cy;
    std::memset(&cy, 0, sizeof(cy));
    cy.d1 = q.d1; cy.d2 = q.d2;
    const int32_t kk = q.kpos == 2 ? kSide - 1 : q.kpos;
    cy.k1 = q.d1 < MCF_INF ? kk : -1;
    cy.k2 = q.d2 < MCF_INF ? kk : -1;
    if (q.minus) { if (leaves != 1) cy.k1 = -1; if (leaves != 2) cy.k2 = -1; }
    cy.n1 = kSide; cy.n2 = kSide;
    const Place& pu = kPlaces[q.place];
    const Place& pw = kPlaces[(q.place + 3) % 7];
    cy.p0u = pu.pos; cy.r0u.size = pu.size_base + pu.size_per_s * q.S; cy.r0u.depth = 6; cy.r0u.parent = 3; cy.r0u.pred = 12;
    cy.p0w = pw.pos; cy.r0w.size = pw.size_base + pw.size_per_s * q.S; cy.r0w.depth = 9; cy.r0w.parent = 4; cy.r0w.pred = 15;
    *k_leave = leaves == 1 ? cy.k1 : (leaves == 2 ? cy.k2 : -1);

    McfNode rec1[kSide], rec2[kSide];
    int32_t ppos1[kSide], ppos2[kSide], path1[kSide], path2[kSide];
    for (int32_t j = 0; j < kSide; ++j) {
        const bool q1 = j == cy.k1, q2 = j == cy.k2;
        rec1[j].parent = 100 + j; rec1[j].pred = ((7 + j) << 1) | q.parity; rec1[j].size = q1 ? q.S : q.S + 5 + j; rec1[j].depth = 5 - j;
        rec2[j].parent = 200 + j; rec2[j].pred = ((57 + j) << 1) | q.parity; rec2[j].size = q2 ? q.S : q.S + 6 + j; rec2[j].depth = 8 - j;
        ppos1[j] = q1 ? kA0 : 200 + 10 * j;
        ppos2[j] = q2 ? kA0 : 300 + 10 * j;
        path1[j] = 500 + j; path2[j] = 600 + j;
    }
    McfPaths pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.path1 = path1; pp.path2 = path2; pp.rec1 = rec1; pp.rec2 = rec2; pp.ppos1 = ppos1; pp.ppos2 = ppos2;
    pp.slot1 = ppos1; pp.slot2 = ppos2;

    McfCtx a = start, b = start;
    McfView v;
    std::memset(&v, 0, sizeof(v));   // no blocked list (bmeta), no Devex weights
    v.n_nodes = 64;
    v.ctx = &a;
    mcf_pivot_decide(v, pp, cy);
    v.ctx = &b;
    mcf_pivot_decide_flat(v, pp, cy);
    *ref_out = a;
    if (std::memcmp(&a, &b, sizeof(McfCtx)) == 0) return 0;
    const unsigned char *pa = reinterpret_cast<const unsigned char*>(&a), *pb = reinterpret_cast<const unsigned char*>(&b);
    for (size_t i = 0; i < sizeof(McfCtx); ++i)
        if (pa[i] != pb[i]) return 1 + (int)i;
    return 1;
}

}  // namespace

extern "C" {

// counts[]: 0 cases, 1 mismatches, 2 unbounded, 3 bound flips, 4 swaps on the first side, 5 on the second, 6 degenerate,
// 7 swaps with t == tA != tB, 8 with t == tB != tA, 9 with costA == costB and tA != tB, 10 with t <= a0, 11 with t == a0 + S,
// 12 with t > a0 + S, 13 one-node T2 on the first side, 14 on the second (the adjacency range moves), 15 swaps with -1 on the
// other side, 16 / 17 / 18 swaps with k == 0 / 1 / the last index, 19 swaps with both parities seen (bit mask 1 | 2),
// 20 swaps with both states seen (bit mask), 21 swaps of a three-node T2, 22 first mismatch: case number, 23: its byte.
enum { MCF_DECIDE_FLAT_COUNTS = 24 };

int mcf_decide_flat_sweep_host(int64_t* counts) {
    if (!counts) return -1;
    for (int i = 0; i < MCF_DECIDE_FLAT_COUNTS; ++i) counts[i] = 0;
    counts[22] = -1; counts[23] = -1;
    Case q;
    for (int i1 = 0; i1 < 6; ++i1) for (int i2 = 0; i2 < 6; ++i2) for (int ic = 0; ic < 6; ++ic)
    for (int s = -1; s <= 1; s += 2) for (int parity = 0; parity < 2; ++parity) for (int S = 1; S <= 3; S += 2)
    for (int kpos = 0; kpos < 3; ++kpos) for (int minus = 0; minus < 2; ++minus) for (int place = 0; place < 7; ++place) {
        q.d1 = kResiduals[i1]; q.d2 = kResiduals[i2]; q.cap = kResiduals[ic];
        q.s = s; q.parity = parity; q.S = S; q.kpos = kpos; q.minus = minus; q.place = place;
        McfCtx r;
        int32_t k = -1;
        const int bad = run_case(q, &r, &k);
        if (bad) { if (counts[1] == 0) { counts[22] = counts[0]; counts[23] = bad - 1; } counts[1] += 1; }
        counts[0] += 1;
        if (r.status == MCF_UNBOUNDED) { counts[2] += 1; continue; }
        if (r.pv_delta == 0) counts[6] += 1;
        if (r.stage == 1) { counts[3] += 1; continue; }
        if (r.stage != 2) return -2;
        counts[r.pv_result == 1 ? 4 : 5] += 1;
        const Place& pl = kPlaces[r.pv_result == 1 ? (place + 3) % 7 : place];   // v_in: the end point on the other side
        const int32_t tA = pl.pos + 1, tB = pl.pos + pl.size_base + pl.size_per_s * S;
        const int32_t costA = tA <= kA0 ? kA0 - tA : tA - (kA0 + S), costB = tB <= kA0 ? kA0 - tB : tB - (kA0 + S);
        const int32_t t = costA <= costB ? tA : tB;   // (the case is what its place says: checked on the reference's descriptor)
        if (r.t2_old != kA0 || r.t2_size != S || r.pv_k != k) return -3;
        if (r.t2_new != (t <= kA0 ? t : t - S) || r.lo != (t < kA0 ? t : kA0) || r.hi != (t > kA0 + S ? t : kA0 + S)) return -4;
        if (tA != tB) counts[t == tA ? 7 : 8] += 1;
        if (tA != tB && costA == costB) counts[9] += 1;
        counts[t <= kA0 ? 10 : (t == kA0 + S ? 11 : 12)] += 1;
        if (S == 1) counts[r.pv_result == 1 ? 13 : 14] += 1;
        if (S == 3) counts[21] += 1;
        if (minus) counts[15] += 1;
        counts[k == 0 ? 16 : (k == 1 ? 17 : 18)] += 1;
        counts[19] |= 1 << parity;
        counts[20] |= s > 0 ? 1 : 2;
    }
    return counts[1] == 0 ? 0 : 1;
}

int32_t mcf_decide_flat_ctx_bytes_host(void) { return (int32_t)sizeof(McfCtx); }

}  // extern "C"
