"""Single planted pivots on every engine path, across the capacities built into the pivot and update kernels.

Every case of ``planted_pivots.cases()`` is ``McfEngine(...)``, ``set_basis(in_tree, at_upper)`` -- which has to return ``True``
and to arrive at the planted tree, in the planted preorder -- and then ``solve(1)`` K times next to ``RefSimplex.step()``: flows,
potentials, states, the tree arrays, the stats' deltas, the resident reduced costs and key codes and the handle's own
``certify()`` after every pivot, all exact; then ``solve()`` to the end.  ``test_planted_pivots_cpu.py`` checks the cases and the
reference themselves.

``solve(1)`` is less than a batch, and ``mcf_solve`` launches a budget below a batch eagerly -- also on a handle that has
captured a graph.  The captured graph (and ``k_pivot_run``, which exists in a graph only) is replayed for a budget of at least
one batch, so the ``*_replay`` paths make ONE ``solve(budget)`` of a whole batch and compare what it arrives at: K Dantzig
pivots against the reference's K-th snapshot, or, under the candidate-list rule, a ``lone_*`` case, whose planted pivot is the
whole solve whatever the rule.  No stat says "this pivot was replayed": the proof is the host's arithmetic, budget >= batch.

Which branch a case reaches follows from its arithmetic (``DESIGN.md``, "In-kernel capacities of the pivot and update
kernels"): |T2| against kBplListMember 32 / kBplT2Cap 8 192 -- and, where k_pivot_run makes the pivot, kRunMaxSubtree 64, behind
which its other capacities cannot be reached --, the stem's 2 * stem + 1 segments against kBplSegLds 1 024, the cycle's tree arcs against kSmallPath 512 / kHitsLds 4 096, the end
points' depth against the climb gate (``cycle_scans`` says which way it went).  No stat exists for a list that overflowed: there
the proof is 2 * stem + 1 > 1 024, or more than 8 192 nodes of T2 in the list of ONE workgroup -- the ``t2cap_*`` cases on the
path ``bpl6_grid1``, where a single grid workgroup lists all of T2 but its first block of 64 -- on a handle with resident reduced
costs, which the test asserts it is."""

from __future__ import annotations

import numpy as np
import pytest

import planted_pivots as pp
from planted_trees import check_tree_arrays
from wide_range_instances import _vkey_code

pytestmark = pytest.mark.gpu

DENSE = dict(fused=False, mid_loop=-1, tree_blocks=-1)
# path -> (engine options, rule, pricing_mode or None, environment)
PATHS = {
    "grid_dense_graph": (dict(DENSE, use_graph=True), 0, 1, {}),                          # k_pivot, k_update: eager for solve(1), the graph in the closing solve()
    "grid_dense_replay": (dict(DENSE, use_graph=True, batch_pivots=pp.K_PIVOTS), 0, 1, {}),   # ... and K pivots as one replay of the captured graph
    "bpl6_replay": (dict(tree_blocks=6, use_graph=True, batch_pivots=pp.K_PIVOTS), 0, 1, {}),
    "grid_dense_eager": (dict(DENSE, use_graph=False, batch_pivots=7), 0, 1, {}),
    "bpl2": (dict(tree_blocks=2), 0, 1, {}),                                              # k_update_bpl, blocks of 4 slots
    "bpl6": (dict(tree_blocks=6), 0, 1, {}),
    "bpl10": (dict(tree_blocks=10), 0, 1, {}),
    "bpl3_rebuild": (dict(tree_blocks=3, tree_pool=-1), 0, 1, {}),                        # no spare blocks: the whole list rewritten on every swap
    "bpl2_grid1": (dict(tree_blocks=2), 0, 1, {"MCF_BPL_GRID": "1"}),                     # one workgroup asked for: mcf_create has to double the grid
    "bpl2_grid1_rebuild": (dict(tree_blocks=2, tree_pool=-1), 0, 1, {"MCF_BPL_GRID": "1"}),
    "bpl6_grid1": (dict(tree_blocks=6), 0, 1, {"MCF_BPL_GRID": "1"}),                     # ONE grid workgroup lists all of T2 but its first block
    "gather": (dict(DENSE, resident_rc=False), 0, 0, {}),                                 # no resident reduced costs
    "bpl4_rc_drop": (dict(tree_blocks=4, rc_drop=1), 0, 1, {}),                           # armed to drop the reduced costs; mcf_solve looks every 4 096 pivots, so still resident here
    "bpl4_gather": (dict(tree_blocks=4, resident_rc=False), 0, 0, {}),                    # k_update_bpl<false, false>
    "key_codes_dense": (dict(DENSE, compressed_keys=1), 0, 1, {}),
    "key_codes_bpl5": (dict(tree_blocks=5, compressed_keys=1), 0, 1, {}),
    "persistent_loop": (dict(fused=False, mid_loop=1), 0, 3, {}),                         # k_solve_mid
    "fused_lds": (dict(fused=True), 0, 2, {}),                                            # k_solve_small
    "pivot_run": (dict(tree_blocks=3, pivot_run=4), 2, 1, {}),                            # first pivot by k_pivot (eager); k_pivot_run in the closing solve()
    "pivot_run_replay": (dict(tree_blocks=3, pivot_run=4, use_graph=True), 2, 1, {}),     # k_pivot_run makes the planted pivot
    "pivot_run_replay_gather": (dict(tree_blocks=3, pivot_run=4, use_graph=True, resident_rc=False), 2, 0, {}),   # k_pivot_run<false, false>
    "candidate_bpl3_replay": (dict(tree_blocks=3, use_graph=True), 2, 1, {}),             # the same graph in pair shape: k_pivot, k_update_bpl
    "candidate_dense": (dict(DENSE), 2, 1, {}),
    "candidate_bpl6": (dict(tree_blocks=6), 2, 1, {}),
}
TINY_SET = [c for c in pp.CASE_IDS if (c.startswith(("backward", "theta0", "leave_", "equal_violation", "through_root", "artificial_")) and c != "artificial_leaves_theta0")
            or (c.startswith("ties_") and not c.endswith("_long"))]          # fewer than 100 nodes each
SMALL_SET = TINY_SET + ["artificial_leaves_theta0"]                         # (2 100 nodes: a whole component re-hung by a degenerate pivot)


def _ids(*prefixes):
    return [c for c in pp.CASE_IDS if c.startswith(prefixes)]


# the full list where the issue asks for it; elsewhere the cases that straddle the path's own constants, and the small set
PATH_CASES = {
    "grid_dense_graph": pp.CASE_IDS,
    "bpl2": pp.CASE_IDS,
    "bpl6": pp.CASE_IDS,
    "bpl10": pp.CASE_IDS,
    "grid_dense_eager": SMALL_SET + _ids("cycle_", "depth_", "t2_1") + ["t2_2"],
    "bpl3_rebuild": SMALL_SET + _ids("t2_31", "t2_32", "t2_33", "align_", "tail_end", "same_block", "t2_8193"),
    "bpl2_grid1": ["blocks_2049", "t2_8193", "t2_8193_second_after", "t2_2049", "leave_first", "leave_second"],
    "bpl2_grid1_rebuild": ["blocks_2049", "t2_8193", "leave_first", "leave_entering"],
    "bpl6_grid1": _ids("t2cap_", "t2_819") + ["leave_first", "leave_second", "through_root"],
    "gather": SMALL_SET + _ids("t2_819", "stem_51", "cycle_409"),
    "bpl4_rc_drop": SMALL_SET + _ids("t2_819", "t2_31", "t2_32", "t2_33", "stem_51", "t2_1"),
    "bpl4_gather": SMALL_SET + _ids("t2_819", "t2_31", "t2_32", "t2_33", "stem_51", "t2_1"),
    "key_codes_dense": SMALL_SET + _ids("t2_819", "t2_1"),
    "key_codes_bpl5": SMALL_SET + _ids("t2_819", "t2_1", "t2_3", "stem_51"),
    # the persistent loop takes any size when asked for (mid_loop = 1); it shares pivot_core with k_pivot (kSmallPath, kHitsLds,
    # the climb gate) and patches the reduced costs of T2 itself
    "persistent_loop": TINY_SET + _ids("cycle_", "stem_", "depth_", "t2_3", "t2_6", "t2_1", "align_5", "ties_"),
    # the fused path needs m_pad * 21 + (m + n) * 16 + (n + 1) * 112 + 4 096 < 150 KiB of LDS: the cases of fewer than 100 nodes
    "fused_lds": TINY_SET + _ids("depth_", "t2_1", "align_5") + ["t2_2"],
    "pivot_run": _ids("t2_63", "t2_64", "t2_65", "stem_127", "stem_128", "stem_129", "t2_2047", "t2_2048", "t2_2049") + SMALL_SET,
    "pivot_run_replay": _ids("lone_"),
    "pivot_run_replay_gather": _ids("lone_"),
    "candidate_bpl3_replay": _ids("lone_"),
    "grid_dense_replay": SMALL_SET + _ids("lone_", "cycle_51", "cycle_409", "depth_", "t2_1", "t2_819") + ["t2_2"],
    "bpl6_replay": SMALL_SET + _ids("lone_", "t2_1", "t2_3", "t2_819", "stem_51", "align_", "same_block") + ["t2_2"],
    "candidate_dense": SMALL_SET + _ids("t2_64", "stem_128"),
    "candidate_bpl6": SMALL_SET + _ids("t2_64", "stem_128"),
}
# path -> budget of its one compared solve: at least a batch, so that mcf_solve replays the captured graph.  Dantzig: batch_pivots =
# K, exactly; candidate list: 64 rounded to whole list periods of at most 33 slots, at most 82 (the lone pivot ends the solve)
REPLAY = {"grid_dense_replay": pp.K_PIVOTS, "bpl6_replay": pp.K_PIVOTS, "pivot_run_replay": 1000, "pivot_run_replay_gather": 1000, "candidate_bpl3_replay": 1000}
PATH_CASE_PARAMS = [pytest.param(p, c, id=f"{p}-{c}") for p, cs in PATH_CASES.items() for c in dict.fromkeys(cs)]
CERT_ZERO = ("tree_shape_count", "tree_rc_count", "state_flow_count", "basic_count_mismatch", "rc_mismatch_count", "key_mismatch_count")
STAT_KEYS = ("pivots", "degenerate", "bound_flips", "cycle_arcs", "subtree_nodes", "cycle_scans", "tree_rebuilds")


def _compare(cid, j, eng, inst, s, res, tree, bigm):
    """The resident state after pivot j against the reference's snapshot."""
    n = inst.n
    tag = (cid, j)
    assert np.array_equal(res.flow, s["flow"]), tag
    assert np.array_equal(res.in_tree, s["state"] == 0), tag
    assert np.array_equal(tree["state"], s["state"]), tag
    assert np.array_equal(res.potential, s["potential"][:n]) and np.array_equal(tree["pi"], s["potential"]), tag
    for k in ("parent", "pred_arc", "depth", "size"):
        assert np.array_equal(tree[k], s[k]), tag + (k,)
    check_tree_arrays(n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
    assert res.stats["artificial_flow"] == int(s["art_flow"].sum()), tag
    want_rc = inst.cost + s["potential"][inst.tail] - s["potential"][inst.head]
    rc, resident = eng.reduced_costs()
    if resident:
        assert np.array_equal(rc, want_rc), tag
    keys, present = eng.pricing_keys()
    if present:
        assert np.array_equal(keys, _vkey_code(-s["state"] * want_rc, bigm, 1 << 28)), tag
    cert = eng.certify()
    assert {k: cert[k] for k in CERT_ZERO} == dict.fromkeys(CERT_ZERO, 0), tag
    return resident


def _run(e, path, cid):
    """One case on one engine path, every check; returns the preorders it went through."""
    kw, rule, mode, env = PATHS[path]
    with pytest.MonkeyPatch.context() as mp:         # (mcf_create reads the environment)
        for k, v in env.items():
            mp.setenv(k, v)
        return _run_in_env(e, path, cid, kw, rule, mode)


def _run_in_env(e, path, cid, kw, rule, mode):
    p = pp.planted(cid)
    pl, inst = p.pl, p.inst
    n = inst.n
    snaps, objective, status, total = pp.trajectory(cid)
    case_kw = pp.BY_ID[cid][4]
    climb_depth = case_kw.get("climb_depth", 3)          # (automatic: 3 up to 32 768 nodes)
    bigm = pp.big_m(inst)
    orders = []
    with e.McfEngine(n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **dict(kw, **case_kw)) as eng:
        assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
        res, tree = eng.result(), eng.tree()
        assert np.array_equal(res.flow, pl.flow) and np.array_equal(tree["state"], pl.state)
        assert np.array_equal(tree["parent"][:n], pl.parent) and np.array_equal(tree["pred_arc"][:n], pl.tree_arc)
        assert np.array_equal(tree["pos"][:n], np.arange(1, n + 1)), "labels are the preorder"
        orders.append(tree["order"].copy())
        st = res.stats
        if mode is not None:
            assert st["pricing_mode"] == mode, (path, cid, st["pricing_mode"])
        assert st["tree_blocks"] == max(kw.get("tree_blocks", -1 if mode in (2, 3) else 0), 0), (path, cid, st["tree_blocks"])
        prev = {k: st[k] for k in STAT_KEYS}
        if kw.get("pivot_run"):
            assert st["run_pairs"] == kw["pivot_run"], "mcf_create took the run shape"
        if path in REPLAY:
            # one solve of a whole batch: the captured graph, replayed once, makes the pivots
            used = snaps[: min(REPLAY[path], pp.K_PIVOTS)]
            assert rule == 0 or (p.args["lone"] and total == 1), "the reference follows a candidate list no further than its first pivot"
            assert rule != 0 or (kw["batch_pivots"] == REPLAY[path] and total >= len(used))
            eng.solve(REPLAY[path])
            res, tree = eng.result(), eng.tree()
            _compare(cid, len(used), eng, inst, used[-1], res, tree, bigm)
            st = res.stats
            delta = {k: st[k] - prev[k] for k in STAT_KEYS}
            want = dict(pivots=len(used), degenerate=sum(int(s["degenerate"]) for s in used), bound_flips=sum(int(s["flip"]) for s in used),
                        cycle_arcs=sum(s["cycle_len"] for s in used), subtree_nodes=sum(s["t2"] for s in used),
                        cycle_scans=sum(int(s["deep"] > climb_depth) for s in used))
            assert {k: delta[k] for k in want} == want, (cid, delta)
            if kw.get("pivot_run"):
                assert st["run_pairs"] == kw["pivot_run"] and st["run_left_at"] == 0, "the run shape was kept"
            orders.append(tree["order"].copy())
            snaps = []
        # (candidate list: the first pivot is Dantzig's; the minor pivots that follow are the list's own business)
        for j, s in enumerate(snaps[: 1 if rule == 2 else pp.K_PIVOTS], 1):
            eng.solve(1)
            res, tree = eng.result(), eng.tree()
            resident = _compare(cid, j, eng, inst, s, res, tree, bigm)
            st = res.stats
            delta = {k: st[k] - prev[k] for k in STAT_KEYS}
            prev = {k: st[k] for k in STAT_KEYS}
            want = dict(pivots=1, degenerate=int(s["degenerate"]), bound_flips=int(s["flip"]), cycle_arcs=s["cycle_len"], subtree_nodes=s["t2"])
            assert {k: delta[k] for k in want} == want, (cid, j, delta)
            # the depth gate: end points no deeper than climb_depth are climbed, the others found by the scan (the fused loop
            # finds every cycle in LDS and never scans)
            assert delta["cycle_scans"] == (0 if mode == 2 else int(s["deep"] > climb_depth)), (cid, j, s["deep"], delta)
            if kw.get("tree_pool") == -1:
                assert delta["tree_rebuilds"] == int(not s["flip"]), (cid, j, delta)
            if j == 1 and kw.get("rc_drop", 0) == 0 and kw.get("resident_rc", True) and mode == 1:
                assert resident, "the arithmetic proves the overflow branches only where the reduced costs are resident"
            orders.append(tree["order"].copy())
        eng.solve()
        res = eng.result()
        assert res.status == status and res.objective == objective, (cid, res.status, status)
        if rule == 0:
            assert res.stats["pivots"] == total
        cert = eng.certify()
        assert cert["verdict"] == status and cert["proves_status"]
        assert {k: cert[k] for k in CERT_ZERO} == dict.fromkeys(CERT_ZERO, 0)
    return orders


@pytest.fixture(scope="module")
def run_case(gpu_engine_module):
    """(path, case) -> the preorders of that run, every check of ``_run`` made; each pair runs once in this module."""
    done = {}

    def run(path, cid):
        if (path, cid) not in done:
            done[(path, cid)] = _run(gpu_engine_module, path, cid)
        return done[(path, cid)]
    return run


@pytest.mark.parametrize("path, cid", PATH_CASE_PARAMS)
def test_planted_pivot(run_case, path, cid):
    run_case(path, cid)


@pytest.mark.parametrize("cid", pp.CASE_IDS)
def test_blocked_list_keeps_the_dense_preorder(run_case, cid):
    """include/mcf.h: "same logical preorder, same pivots" -- the order array after every pivot, dense array against blocks of
    4, 64 and 1 024 slots."""
    dense = run_case("grid_dense_graph", cid)
    for path in ("bpl2", "bpl6", "bpl10"):
        got = run_case(path, cid)
        assert len(got) == len(dense)
        for j, (a, b) in enumerate(zip(dense, got)):
            assert np.array_equal(a, b), (cid, path, j)


def test_grid_doubling_case_is_sized_for_it():
    """MCF_BPL_GRID=1 on blocks of four slots: the pool of the case holds more than 2 048 blocks (kBplTouchedCap per workgroup),
    and its T2 alone spans more than 2 048 of them."""
    p = pp.planted("blocks_2049")
    dense = (p.inst.n + 1 + 3) // 4
    assert dense > 2048 and p.t2 // 4 > 2048
