"""The state of the Devex and candidate-list rules on every engine path, against ``rule_reference.py`` -- plain Python from the
written rule (``DESIGN.md`` section 4, "State of the pricing rules") -- on the instances of ``rule_instances.py``.
``test_rule_reference_cpu.py`` checks those references and instances without a GPU.

Protocol of a case on a path: from a cold start ``solve(1)`` for the first 6 pivots and for every pivot from 2 before to 2 after
each event (reset, early reset, tuner step, wrap; candidate list: the chosen period ends), ONE ``solve(budget)`` across each gap
between those windows, then ``solve()`` to the end.  At every stop flow, state, potential, parent, ``pred_arc``, depth and size,
the Devex weights (all 1.0 right after a reset pivot) and the deltas of ``pivots``, ``degenerate``, ``bound_flips`` and
``arcs_priced`` equal the reference's, exactly: every quantity is an integer, or one IEEE operation on identical operands.  Then
a second handle makes ONE uninterrupted ``solve()``: budgets must not change the sequence.

The fused LDS loop keeps a candidate list of one entry per head bucket whatever ``price_blocks`` asks for: there the reference of
8 pricing workgroups holds for 16 and 64 too."""

from __future__ import annotations

import numpy as np
import pytest

import rule_instances as ri

pytestmark = pytest.mark.gpu

DENSE = dict(fused=False, mid_loop=-1, tree_blocks=-1)
W256, W1024 = {"MCF_SMALL_THREADS": "256"}, {"MCF_SMALL_THREADS": "1024"}
# path -> (engine options, pricing_mode or None, environment, halts only after jumps)
PATHS = {
    "fused_256": (dict(fused=True), 2, W256, False),                                  # k_solve_small<256>
    "fused_1024": (dict(fused=True), 2, W1024, False),
    "fused_auto": (dict(fused=True), 2, {}, False),                                   # the width mcf_create chooses
    "mid_loop": (dict(fused=False, mid_loop=1), 3, {}, False),                        # k_solve_mid
    "grid_graph": (dict(DENSE, use_graph=True), 1, {}, False),                        # eager below a batch, the graph in the jumps
    "grid_eager7": (dict(DENSE, use_graph=False, batch_pivots=7), 1, {}, False),
    "gather": (dict(DENSE, resident_rc=False), 0, {}, False),
    "bpl4": (dict(tree_blocks=4), 1, {}, False),
    "bpl4_rc_drop": (dict(tree_blocks=4, rc_drop=1), 1, {}, False),
    "overlap": (dict(DENSE, use_graph=True, overlap_update=1), 1, {}, False),
    "bpl3": (dict(tree_blocks=3), 1, {}, False),
    "bpl3_run": (dict(tree_blocks=3, pivot_run=4, use_graph=True), 1, {}, True),      # k_pivot_run exists in a replayed graph only
    "incremental": (dict(DENSE, full_sweeps=-1), 1, {}, False),
    "key_codes": (dict(DENSE, compressed_keys=1), 1, {}, False),
}
ALL_DEVEX = [c for c, v in ri.CASES.items() if v[1] == ri.DEVEX]
NOT_WIDTH = [c for c in ALL_DEVEX if not c.startswith("devex_nodes")]
# the events a path's own code handles -- the weight reset pass over the touched list, the block's bounds from the granule
# table, the walk over empty blocks -- plus swaps_200
SOME_DEVEX = ["swaps_200", "flips_1100", "flips_1100_fixed", "shrink_to_1", "empty_blocks_stay", "direction_ties"]
ALL_LIST = [c for c, v in ri.CASES.items() if v[1] == ri.LIST]
PATH_CASES = {
    "fused_256": ALL_DEVEX + ALL_LIST,
    "fused_1024": ALL_DEVEX + ALL_LIST,
    "fused_auto": ["devex_nodes_128", "devex_nodes_129"],
    "mid_loop": NOT_WIDTH,
    "grid_graph": NOT_WIDTH + ALL_LIST,
    "grid_eager7": SOME_DEVEX,
    "gather": SOME_DEVEX + ALL_LIST,
    "bpl4": SOME_DEVEX,
    "bpl4_rc_drop": SOME_DEVEX,
    "overlap": SOME_DEVEX,
    "bpl3": ALL_LIST,
    "bpl3_run": ALL_LIST,
    "incremental": ALL_LIST,
    "key_codes": ALL_LIST,
}
PARAMS = [pytest.param(p, c, id=f"{p}-{c}") for p, cs in PATH_CASES.items() for c in cs]
COUNTERS = ("pivots", "degenerate", "bound_flips", "arcs_priced")
CERT_ZERO = ("tree_shape_count", "tree_rc_count", "state_flow_count", "basic_count_mismatch", "rc_mismatch_count", "key_mismatch_count")
RUN_GAP = 70          # a budget of at least one batch of 64 pivots: mcf_solve replays the captured graph


def _reference_case(path: str, cid: str) -> str:
    """The case whose trajectory the handle has to follow (see the module docstring)."""
    if path.startswith("fused") and cid.startswith("list_periods_"):
        return "list_periods_8"
    return cid


def _engine(e, path, cid):
    kw, _, _, _ = PATHS[path]
    name, rule, opt = ri.CASES[cid]
    inst = ri.instance(name)
    eng_kw = dict(kw)
    for ours, theirs in (("block_size", "block_size"), ("tuner", "devex_tuner"), ("stay", "devex_stay"), ("price_blocks", "price_blocks")):
        if ours in opt:
            eng_kw[theirs] = opt[ours]
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **eng_kw)


def _compare(eng, rule, n, s, prev, tag, reset=None):
    res, tree = eng.result(), eng.tree()
    assert np.array_equal(res.flow, s["flow"]), tag
    assert np.array_equal(tree["state"], s["state"]) and np.array_equal(res.in_tree, s["state"] == 0), tag
    assert np.array_equal(res.potential, s["potential"][:n]) and np.array_equal(tree["pi"], s["potential"]), tag
    for k in ("parent", "pred_arc", "depth", "size"):
        assert np.array_equal(tree[k], s[k]), tag + (k,)
    if rule == ri.DEVEX:
        w = eng.weights()
        assert w.dtype == np.float32 and np.array_equal(w, s["weights"]), tag + ("weights", np.flatnonzero(w != s["weights"])[:8])
        if reset:
            assert (w == 1.0).all(), tag
    now = {k: res.stats[k] for k in COUNTERS}
    print(tag, {k: now[k] - prev[k] for k in COUNTERS})
    assert {k: now[k] - prev[k] for k in COUNTERS} == {k: s[k] - prev["ref"][k] for k in COUNTERS}, tag
    now["ref"] = {k: s[k] for k in COUNTERS}
    return now


def _final(eng, rule, n, tr, prev, tag):
    now = _compare(eng, rule, n, tr["final"], prev, tag)
    res = eng.result()
    assert res.status == tr["status"] == "optimal" and res.objective == tr["objective"] and res.stats["pivots"] == tr["total"], tag
    cert = eng.certify()
    assert cert["verdict"] == "optimal" and cert["proves_status"], tag
    assert {k: cert[k] for k in CERT_ZERO} == dict.fromkeys(CERT_ZERO, 0), tag
    return now


def _stops(tr, jumps_only: bool):
    if not jumps_only:
        return tr["stops"]
    out, at = [], 0
    for k in tr["stops"]:
        if k - at >= RUN_GAP:
            out.append(k)
            at = k
    return out


def _run(e, path, cid):
    kw, mode, env, jumps_only = PATHS[path]
    with pytest.MonkeyPatch.context() as mp:         # (mcf_create reads the environment)
        mp.delenv("MCF_SMALL_THREADS", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        _, rule, _ = ri.CASES[cid]
        tr = ri.trajectory(_reference_case(path, cid))
        n = ri.instance(ri.CASES[cid][0]).n
        zero = dict.fromkeys(COUNTERS, 0)
        with _engine(e, path, cid) as eng:
            st = eng.result().stats
            assert st["pricing_mode"] == mode, (path, cid, st["pricing_mode"])
            if kw.get("pivot_run"):
                assert st["run_pairs"] == kw["pivot_run"], "mcf_create took the run shape"
            prev, at, jumped = dict(zero, ref=zero), 0, False
            for k in _stops(tr, jumps_only):
                eng.solve(k - at)
                jumped |= k - at > 1
                s = tr["snaps"][k]
                prev = _compare(eng, rule, n, s, prev, (path, cid, k), reset=s.get("reset"))
                at = k
            assert jumped, "one solve(budget) across a gap between two windows"
            eng.solve()
            _final(eng, rule, n, tr, prev, (path, cid, "end"))
        with _engine(e, path, cid) as eng:           # budgets must not change the sequence
            eng.solve()
            _final(eng, rule, n, tr, dict(zero, ref=zero), (path, cid, "uninterrupted"))


@pytest.mark.parametrize("path, cid", PARAMS)
def test_rule_state_follows_the_reference(gpu_engine_module, path, cid):
    _run(gpu_engine_module, path, cid)


@pytest.mark.parametrize("path", ("fused_256", "fused_1024", "mid_loop", "grid_graph", "bpl4", "gather"))
def test_budget_that_ends_on_a_reset_pivot(gpu_engine_module, path):
    """solve(k) with pivot k the first reset, then solve(): the weights read 1.0 in between and the sequence goes on as if uncut."""
    cid = "swaps_200"
    tr = ri.trajectory(cid)
    k = next(p for p, w in tr["events"] if w == "reset")
    n = ri.instance(ri.CASES[cid][0]).n
    zero = dict.fromkeys(COUNTERS, 0)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MCF_SMALL_THREADS", raising=False)
        for key, v in PATHS[path][2].items():
            mp.setenv(key, v)
        with _engine(gpu_engine_module, path, cid) as eng:
            eng.solve(k)
            prev = _compare(eng, ri.DEVEX, n, tr["snaps"][k], dict(zero, ref=zero), (path, cid, k), reset=True)
            eng.solve()
            _final(eng, ri.DEVEX, n, tr, prev, (path, cid, "end"))


@pytest.mark.parametrize("path", ("fused_256", "fused_1024", "grid_graph", "bpl3", "bpl3_run", "incremental", "key_codes", "gather"))
def test_budget_that_ends_inside_a_list_period(gpu_engine_module, path):
    """solve(k) with pivot k the first minor pivot of the first period that takes all its minor pivots, then solve()."""
    cid = "list_periods_8"
    tr = ri.trajectory(cid)
    full = next(i for i, p in enumerate(tr["periods"]) if p[1] == "full")
    ends = [p for p, w in tr["events"] if w == "period_end"]
    k = ends[full] - tr["minor_cap"] + 1
    assert (ends[full - 1] if full else 0) + 1 < k < ends[full] and k in tr["snaps"]
    n = ri.instance(ri.CASES[cid][0]).n
    zero = dict.fromkeys(COUNTERS, 0)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MCF_SMALL_THREADS", raising=False)
        for key, v in PATHS[path][2].items():
            mp.setenv(key, v)
        with _engine(gpu_engine_module, path, cid) as eng:
            eng.solve(k)
            prev = _compare(eng, ri.LIST, n, tr["snaps"][k], dict(zero, ref=zero), (path, cid, k))
            eng.solve()
            _final(eng, ri.LIST, n, tr, prev, (path, cid, "end"))


BATCH = ("swaps_200", "swaps_200_stay", "flips_1100", "shrink_to_1", "empty_blocks", "devex_nodes_128", "devex_nodes_129", "swaps_200_list",
         "list_periods_8")


@pytest.mark.parametrize("path", ("fused_256", "fused_1024", "mid_loop"))
def test_batch_of_instances_in_one_launch(gpu_engine_module, path):
    """mcf_solve_batch of the small and of the mid kernels: every handle up to its own first event in one launch, compared there,
    then all of them to the end in a second one."""
    e = gpu_engine_module
    zero = dict.fromkeys(COUNTERS, 0)
    with pytest.MonkeyPatch.context() as mp:         # (mcf_solve_batch reads the environment at the call)
        mp.delenv("MCF_SMALL_THREADS", raising=False)
        for key, v in PATHS[path][2].items():
            mp.setenv(key, v)
        engines = [_engine(e, path, cid) for cid in BATCH]
        try:
            assert all(eng.stats()["pricing_mode"] == PATHS[path][1] for eng in engines)
            trs = [ri.trajectory(cid) for cid in BATCH]
            first = [next(p for p, _ in tr["events"] if p in tr["snaps"]) for tr in trs]
            e.solve_batch(engines, max_pivots=first)
            prevs = []
            for eng, cid, tr, k in zip(engines, BATCH, trs, first):
                n = ri.instance(ri.CASES[cid][0]).n
                prevs.append(_compare(eng, ri.CASES[cid][1], n, tr["snaps"][k], dict(zero, ref=zero), (path, "batch", cid, k), reset=tr["snaps"][k].get("reset")))
            e.solve_batch(engines)
            for eng, cid, tr, prev in zip(engines, BATCH, trs, prevs):
                n = ri.instance(ri.CASES[cid][0]).n
                _final(eng, ri.CASES[cid][1], n, tr, prev, (path, "batch", cid, "end"))
        finally:
            for eng in engines:
                eng.close()
