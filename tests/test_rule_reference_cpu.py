"""The Devex and candidate-list references of ``rule_reference.py`` -- plain Python from the written rule (``DESIGN.md`` section 4,
"State of the pricing rules") -- against the CPU emulation -- compiled from the kernels' own header -- pivot for pivot, on the
instances of ``rule_instances.py``; the events those instances exist for, asserted on the reference's trajectory; the restated
reference solver's objective; and the first pivots of one case recomputed here from the raw arrays, without either.

What of a case's options the emulation can be given: the block size is an argument of ``emul_solve``; ``stay``, the tuner switched
off or on, and the number of pricing workgroups are environment switches of the emulation (``MCF_DEVEX_CYCLIC``,
``MCF_DEVEX_NOTUNE``, ``MCF_DEVEX_TUNE``, ``MCF_EMUL_PRICE_BLOCKS``) -- so every case is compared whole, the candidate list at 8,
16 and 64 pricing workgroups."""

from __future__ import annotations

import numpy as np
import pytest

import oracle
import rule_instances as ri
import rule_reference as rr
from planted_trees import MCF_INF

CASE_IDS = list(ri.CASES)
DEVEX_IDS = [c for c in CASE_IDS if ri.CASES[c][1] == ri.DEVEX]
LIST_IDS = [c for c in CASE_IDS if ri.CASES[c][1] == ri.LIST]


def _env(opt) -> dict:
    env = {}
    if opt.get("stay"):
        env["MCF_DEVEX_CYCLIC"] = "0"
    if opt.get("tuner", 0) < 0:
        env["MCF_DEVEX_NOTUNE"] = "1"
    if opt.get("tuner", 0) > 0:
        env["MCF_DEVEX_TUNE"] = "1"
    if "price_blocks" in opt:
        env["MCF_EMUL_PRICE_BLOCKS"] = str(opt["price_blocks"])
    return env


def _emul(cid: str, max_pivots: int = -1, trace: int = 0) -> dict:
    name, rule, opt = ri.CASES[cid]
    inst = ri.instance(name)
    with pytest.MonkeyPatch.context() as mp:         # (the emulation reads the environment at every solve)
        for k in ("MCF_DEVEX_CYCLIC", "MCF_DEVEX_NOTUNE", "MCF_DEVEX_TUNE", "MCF_EMUL_PRICE_BLOCKS"):
            mp.delenv(k, raising=False)
        for k, v in _env(opt).items():
            mp.setenv(k, v)
        return oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, block_size=opt.get("block_size", 0),
                                 max_pivots=max_pivots, trace=trace)


def _same_state(em, s, n, tag):
    assert np.array_equal(em["flow"], s["flow"]), tag
    assert np.array_equal(em["in_tree"] != 0, s["state"] == 0), tag
    assert np.array_equal(em["potential"], s["potential"][:n]), tag
    for k in ("parent", "pred_arc", "depth", "size"):
        assert np.array_equal(em[k], s[k]), tag + (k,)
    keys = [k for k in ("pivots", "degenerate", "bound_flips", "arcs_priced", "minor_pivots", "major_sweeps") if k in s]
    assert {k: em[k] for k in keys} == {k: s[k] for k in keys}, tag


@pytest.mark.parametrize("name", list(ri.INSTANCES))
def test_instance_fits_the_fused_loop(name):
    inst = ri.instance(name)
    n, m = inst.n, inst.m
    m_pad = (m + 1023) // 1024 * 1024
    assert n <= 256 and m_pad * 21 + (m + n) * 16 + (n + 1) * 112 + 4096 < 150 * 1024
    assert int(inst.supply.sum()) == 0 and (inst.tail != inst.head).all()


@pytest.mark.parametrize("cid", CASE_IDS)
def test_entering_arcs_equal_the_emulation(cid):
    """Every entering arc of the whole solve, the totals and the final state."""
    tr = ri.trajectory(cid)
    em = _emul(cid, trace=8 * tr["total"] + 4096)
    trace = em["trace"]
    assert (trace == -2).any(), "the trace holds every pricing pass"
    got = trace[trace >= 0]
    k = next((i for i, (a, b) in enumerate(zip(got.tolist(), tr["entering"].tolist())) if a != b), None)
    assert k is None and len(got) == tr["total"], (cid, "first difference at pivot", None if k is None else k + 1, len(got), tr["total"])
    assert em["status"] == tr["status"] == "optimal" and em["objective"] == tr["objective"]
    _same_state(em, tr["final"], ri.instance(ri.CASES[cid][0]).n, (cid, "final"))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_checkpoints_equal_the_emulation(cid):
    """Flows, potentials, parents and the counters after the first 6 pivots and from 2 before to 2 after every event."""
    tr = ri.trajectory(cid)
    n = ri.instance(ri.CASES[cid][0]).n
    for k in tr["stops"]:
        em = _emul(cid, max_pivots=k)
        assert em["status"] == "iteration_limit", (cid, k)
        _same_state(em, tr["snaps"][k], n, (cid, k))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_reference_reaches_the_restated_simplex_objective(cid):
    name, rule, _ = ri.CASES[cid]
    tr = ri.trajectory(cid)
    ref = oracle.solve_soa(ri.instance(name), strategy="devex" if rule == ri.DEVEX else "candidate_list", reference_order=False)
    assert ref["status"] == tr["status"] == "optimal" and ref["objective"] == tr["objective"]


def _granule_steps(tr):
    out = []
    for _, g, _, _ in tr["pass_log"]:
        if not out or out[-1] != g:
            out.append(g)
    return out


def _walks(tr):
    """(the longest run of empty blocks that ended at a block with an eligible arc, the run of empty blocks at the end)."""
    best = run = 0
    for _, _, _, found in tr["pass_log"]:
        if found:
            best, run = max(best, run), 0
        else:
            run += 1
    return best, run


def _kinds(tr, what):
    return [k for k, w in tr["events"] if w == what]


@pytest.mark.parametrize("cid, steps", (("flips_1100", [8, 12, 18, 27, 40, 60, 64]), ("flips_1100_quarter", [16, 24, 36, 54, 64])))
def test_flips_fill_the_touched_list_and_grow_the_block(cid, steps):
    tr = ri.trajectory(cid)
    swaps = tr["total"] - int(tr["flip"].sum())
    assert tr["total"] > rr.WLIST_CAP and swaps < rr.RESET_SWAPS and not _kinds(tr, "reset")
    assert _kinds(tr, "early_reset") == [rr.WLIST_CAP + 1], "1 024 weights set, the next pivot resets"
    before, at = tr["snaps"][rr.WLIST_CAP], tr["snaps"][rr.WLIST_CAP + 1]
    assert (before["weights"] != 1).any() and not before["reset"] and at["reset"] and (at["weights"] == 1).all()
    assert not (tr["flip"] & tr["degenerate"]).any(), "a flip moves flow: the tuner alone calls it degenerate"
    for k in _kinds(tr, "tuner"):
        assert int(tr["degenerate"][k - 50:k].sum()) * 10 < 3 * 50 < int((tr["degenerate"] | tr["flip"])[k - 50:k].sum()) * 10, "grown for the flips"
    assert _granule_steps(tr) == steps and _kinds(tr, "tuner") == [50 * (i + 1) for i in range(len(steps) - 1)], "grows to the cap and stops"
    assert tr["final"]["block_granules"] == rr.GRANULES


def test_the_early_reset_returns_to_block_0():
    """Blocks that stay at 8 granules: pivot 1 025 is found in block 0 and would advance to block 1; the reset makes it 0 again."""
    tr = ri.trajectory("flips_1100_fixed")
    assert _kinds(tr, "early_reset") == [rr.WLIST_CAP + 1] and not _kinds(tr, "tuner") and _granule_steps(tr) == [8]
    assert tr["snaps"][rr.WLIST_CAP]["block_index"] == 0 and tr["snaps"][rr.WLIST_CAP + 1]["block_index"] == 0
    assert tr["snaps"][rr.WLIST_CAP + 2]["block_index"] == 1
    assert (tr["snaps"][rr.WLIST_CAP + 1]["weights"] == 1).all()


def test_a_tuner_step_wraps_the_block_index():
    assert _kinds(ri.trajectory("flips_1100"), "wrap") or _kinds(ri.trajectory("shrink_to_1"), "wrap")


@pytest.mark.parametrize("cid", ("swaps_200", "swaps_200_stay", "swaps_200_fixed"))
def test_swaps_reset_the_weights_three_times(cid):
    tr = ri.trajectory(cid)
    swap_no = np.cumsum(~tr["flip"])                             # basis swaps up to and including pivot k = swap_no[k - 1]
    assert swap_no[-1] >= 200
    resets = _kinds(tr, "reset")
    assert len(resets) == 3 and not _kinds(tr, "early_reset")
    # swaps 1 .. 64 are counted, the 65th resets and is not counted: resets at swaps 65, 130, 195
    assert [int(swap_no[k - 1]) for k in resets] == [65, 130, 195] and not any(tr["flip"][k - 1] for k in resets)
    assert tr["flip"][:resets[0]].any() and resets[0] > 65, "a bound flip inside the first window: the first reset comes later than pivot 65"
    for k in resets:
        assert tr["snaps"][k]["reset"] and (tr["snaps"][k]["weights"] == 1).all() and tr["snaps"][k]["block_index"] == 0
        assert (tr["snaps"][k - 1]["weights"] != 1).any()
    assert bool(_kinds(tr, "tuner")) == (cid != "swaps_200_fixed"), "a caller's block size switches the tuner off"


def test_generic_supplies_shrink_the_block_to_one_granule():
    tr = ri.trajectory("shrink_to_1")
    assert tr["total"] >= 400
    steps = _kinds(tr, "tuner")
    assert _granule_steps(tr) == [16, 12, 9, 6, 4, 3, 2, 1] and steps == [50 * (i + 1) for i in range(7)]
    for k in steps:
        assert 10 * int((tr["degenerate"] | tr["flip"])[k - 50:k].sum()) < 50


def test_the_search_walks_empty_blocks():
    for cid, least in (("empty_blocks", 63), ("empty_blocks_stay", 16)):
        tr = ri.trajectory(cid)
        assert _granule_steps(tr) == [1] and not _kinds(tr, "tuner")
        walk, last = _walks(tr)
        assert walk >= least and last == rr.GRANULES == 64, (cid, walk, last)
    assert _walks(ri.trajectory("swaps_200"))[1] == 1, "one block of 64 granules: one empty pass is the verdict"


def test_stay_and_cyclic_part_ways_early():
    a, b = ri.trajectory("stay_vs_cyclic")["entering"], ri.trajectory("stay_vs_cyclic_stay")["entering"]
    assert not np.array_equal(a[:20], b[:20])
    assert ri.trajectory("stay_vs_cyclic")["objective"] == ri.trajectory("stay_vs_cyclic_stay")["objective"]


@pytest.mark.parametrize("cid", ("direction_ties", "direction_ties_stay"))
def test_a_forward_and_a_backward_arc_share_the_largest_merit(cid):
    tr = ri.trajectory(cid)
    ties = _kinds(tr, "direction_tie")
    assert ties
    state_before = tr["snaps"][ties[0] - 1]["state"]
    assert state_before[tr["entering"][ties[0] - 1]] == -1, "the backward arc enters"


def test_width_switch_instances_straddle_128_tree_nodes():
    assert ri.instance("devex_nodes_128").n + 1 == 128 and ri.instance("devex_nodes_129").n + 1 == 129


@pytest.mark.parametrize("pb", (8, 16, 64))
def test_list_periods_of_every_kind(pb):
    tr = ri.trajectory(f"list_periods_{pb}")
    name, rule, opt = ri.CASES[f"list_periods_{pb}"]
    inst = ri.instance(name)
    # list length and minor pivots per sweep from the emulation's step-wise handle
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCF_EMUL_PRICE_BLOCKS", str(pb))
        st = oracle.EmulStepper(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)
        try:
            assert st.set_shards(1) == (tr["list_len"], tr["minor_cap"]) == (pb, {8: 3, 16: 3, 64: 8}[pb])
        finally:
            st.close()
    periods = tr["periods"]
    assert any(p[:2] == (tr["minor_cap"], "full") for p in periods), "a period that uses all its minor pivots"
    assert any(p[1] == "emptied" and 0 < p[0] < tr["minor_cap"] for p in periods), "a list that empties early"
    assert any(p[2] for p in periods), "a listed arc that was basic by its turn"
    assert any(p[3] for p in periods), "a listed arc that was no longer eligible by its turn"
    assert tr["final"]["major_sweeps"] == len(periods) + 1 and tr["status"] == "optimal", "the last full sweep finds nothing"
    assert tr["final"]["minor_pivots"] == sum(p[0] for p in periods) == tr["total"] - len(periods)


def test_the_workgroup_count_changes_the_list():
    seqs = [ri.trajectory(f"list_periods_{pb}")["entering"] for pb in (8, 16, 64)]
    assert not np.array_equal(seqs[0][:len(seqs[1])], seqs[1][:len(seqs[0])]), "the first bucket's second run of 1 024 arcs has a workgroup of its own"
    assert not np.array_equal(seqs[1][:len(seqs[2])], seqs[2][:len(seqs[1])])
    assert len({ri.trajectory(f"list_periods_{pb}")["objective"] for pb in (8, 16, 64)}) == 1


def test_first_pivots_of_swaps_200_from_the_raw_arrays():
    """The first 6 Devex pivots of ``swaps_200`` with nothing but the arrays and the written rule: engine order by sorting, the
    64 x 8 granule table, blocks of 16 granules advancing after every pivot, merit viol^2 / w in doubles, backward before forward
    and then the lowest index among equal merits, the weight of the entering arc = tree arcs of its cycle."""
    inst = ri.instance("swaps_200")
    tr = ri.trajectory("swaps_200")
    n, m = inst.n, inst.m
    T, H, C = inst.tail.tolist(), inst.head.tolist(), inst.cost.tolist()
    U = [MCF_INF if c < 0 else int(c) for c in inst.cap.tolist()]
    bigm = (max(abs(c) for c in C) + 1) * (n + 2)
    per = -(-n // 8)
    buckets = [sorted((i for i in range(m) if H[i] // per == x), key=lambda i: (T[i], i)) for x in range(8)]
    assert m < 1000 and ((m // 4) * 64 + m // 2) // m == 16
    bg, nb, block = 16, 4, 0
    flow, state, w = [0] * m, [1] * m, [1.0] * m
    # the tree: parent and tree arc per node (the root is n; arc m + v is v's artificial arc, which points up iff supply >= 0)
    parent, tarc = [n] * n + [-1], [m + v for v in range(n)] + [-1]
    art_flow, art_up = [abs(int(s)) for s in inst.supply.tolist()], [int(s) >= 0 for s in inst.supply.tolist()]

    def potential(v):
        total = 0
        while v != n:
            a = tarc[v]
            c, up = (bigm, art_up[v]) if a >= m else (C[a], T[a] == v)
            total += -c if up else c
            v = parent[v]
        return total

    def up_path(v):
        out = []
        while v != n:
            out.append(v)
            v = parent[v]
        return out + [n]

    for k in range(1, ri.FIRST + 1):
        pi = [potential(v) for v in range(n)]
        arcs = [i for L in buckets for i in L[len(L) * (block * bg) // 64:len(L) * min(block * bg + bg, 64) // 64]]
        best = None
        for i in arcs:
            viol = -state[i] * (C[i] + pi[T[i]] - pi[H[i]])
            if viol > 0:
                key = (float(viol) * float(viol) / w[i], state[i] < 0, -i)       # larger merit, then backward, then the lower index
                if best is None or key > best[0]:
                    best = (key, i)
        assert best is not None, "the first blocks of a cold start hold eligible arcs"
        e = best[1]
        assert e == tr["entering"][k - 1], (k, e)
        block = (block + 1) % nb
        first, second = (T[e], H[e]) if state[e] > 0 else (H[e], T[e])
        p1, p2 = up_path(first), up_path(second)
        join = next(v for v in p1 if v in set(p2))
        side1, side2 = p1[:p1.index(join)], p2[:p2.index(join)]

        def item(v, gains_if_up):
            a = tarc[v]
            up, cap, f = (art_up[v], MCF_INF, art_flow[v]) if a >= m else (T[a] == v, U[a], flow[a])
            gains = up == gains_if_up
            return (v, gains, (MCF_INF if cap >= MCF_INF else cap - f) if gains else f)
        route = [item(v, False) for v in reversed(side1)] + [(-1, state[e] > 0, U[e])] + [item(v, True) for v in side2]
        theta = min(r for _, _, r in route)
        leave = max(j for j, it in enumerate(route) if it[2] == theta)      # the last blocking arc from the join
        for v, gains, _ in route:
            d = theta if gains else -theta
            if v < 0:
                flow[e] += d
            elif tarc[v] >= m:
                art_flow[v] += d
            else:
                flow[tarc[v]] += d
        w[e] = float(max(len(side1) + len(side2), 1))
        lv, lgains, _ = route[leave]
        if lv < 0:
            state[e] = -state[e]
        else:
            if tarc[lv] < m:
                state[tarc[lv]] = -1 if lgains else 1
            state[e] = 0
            # re-hang: the nodes from the entering arc's end point inside the cut subtree up to lv turn round
            inside = first if lv in side1 else second
            outside = second if inside == first else first
            chain = up_path(inside)
            chain = chain[:chain.index(lv) + 1]
            old = [(parent[v], tarc[v]) for v in chain]
            parent[inside], tarc[inside] = outside, e
            for j in range(1, len(chain)):
                parent[chain[j]], tarc[chain[j]] = chain[j - 1], old[j - 1][1]
        s = tr["snaps"][k]
        assert flow == s["flow"].tolist() and state == s["state"].tolist(), k
        assert w == s["weights"].astype(np.float64).tolist(), k
        assert [potential(v) for v in range(n)] == s["potential"][:n].tolist(), k
        assert parent[:n] == s["parent"][:n].tolist(), k
