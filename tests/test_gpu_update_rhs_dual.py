"""Dual pivots on the device after supply and capacity changes (``mcf_update_rhs_dual``, ``-m gpu``).

Everything goes through the C ABI.  The reference is ``dual_reference.DualRef``, a plain Python dual network simplex written
from the rule text in include/mcf.h: it starts from the basis the handle holds before the call and must make the same pivots,
one by one (the log), and end on the same basis, array by array.  Every comparison is exact."""

import ctypes

import numpy as np
import pytest

import network_flow_solver_amd as nfs
import verdict_instances as vi
import wide_range_instances as wri
from dual_reference import DualRef
from network_flow_solver_amd import generators
from network_flow_solver_amd.data import SoAProblem
from network_flow_solver_amd.generators import ArcSoA
from test_gpu_update_costs import PATHS, TREE_KEYS, _engine, _fresh, _same_optimum, _snapshot
from test_gpu_update_rhs import _after_repair, _edited, _first_pair, _resolve_equals_fresh

pytestmark = pytest.mark.gpu
INF = 1 << 60
BIG = 1 << 40            # a budget no test reaches
GRID = dict(fused=False, mid_loop=-1)

DUAL_PATHS = {p: PATHS[p] for p in ("grid_dense", "grid_blocked_4", "grid_blocked_7", "key_codes", "gather")}
DUAL_PATHS["blocked_rebuild"] = (dict(tree_blocks=2, tree_pool=-1), (0, 2), 1, (1500, 12000))      # every pivot rebuilds the list
DUAL_CASES = [(p, r) for p, (_, rules, _, _) in DUAL_PATHS.items() for r in rules]
DUAL_IDS = [f"{p}-r{r}" for p, r in DUAL_CASES]


def _cap_inf(cap):
    cap = np.asarray(cap, np.int64)
    return np.where((cap < 0) | (cap >= INF), INF, cap)


def _reference(inst, tree, supply, cap):
    """The reference on the handle's basis (`tree`: mcf_get_tree before the call) under the edited data."""
    n, m = inst.n, inst.m
    state = tree["state"].astype(np.int64).copy()
    old, new = _cap_inf(inst.cap), _cap_inf(cap)
    state[(state == -1) & (old != new) & ((new == 0) | (new >= INF))] = 1          # back to the lower bound (mcf_update_rhs)
    art_basic = tree["pred_arc"][:n] >= m
    art_up = tree["pi"][:n] < tree["pi"][n]                                         # pi[v] = pi[root] - big-M on an up arc
    return DualRef(n, inst.tail, inst.head, inst.cost, cap, supply, state, art_basic, art_up,
                   bigm=wri.big_m_of(n, int(np.abs(inst.cost).max())))


def _expected_start(ref):
    """(violations_before, reason or 0) as the first census and the checks in front of the phase see the reference's start."""
    turned = ref.art_basic & (ref.art_flow < 0)
    before = int((ref.violations()[~turned] > 0).sum())
    if before == 0:
        return before, 1
    if turned.any():
        return before, 4
    if (ref.state * ref.reduced_costs() < 0).any():
        return before, 3
    return before, 0


def _call(eng, inst, supply, cap, **opt):
    ns = np.nonzero(supply != inst.supply)[0]
    na = np.nonzero(np.asarray(cap, np.int64) != inst.cap)[0]
    return eng.update_rhs_dual(ns, supply[ns], na, np.asarray(cap, np.int64)[na], **opt)


def _dual_matches(e, eng, inst, supply, cap, rule, kw, budget=BIG, enter_walk=0, resolve=True, out=None):
    """One call on a solved handle against the reference; returns (rhs report, dual report, log, reference)."""
    tree0, stats0 = eng.tree(), eng.stats()
    ref = _reference(inst, tree0, supply, cap)
    before, reason = _expected_start(ref)
    rep, drep, log = _call(eng, inst, supply, cap, max_pivots=budget, enter_walk=enter_walk, log_cap=4096)
    if out is not None:
        out.update(rep=rep, drep=drep, log=log, ref=ref)
    assert drep["violations_before"] == before, (drep, before)
    cur = _edited(inst, supply, cap)
    st1 = eng.stats()
    for k in ("pivots", "degenerate", "bound_flips", "arcs_priced"):
        assert st1[k] == stats0[k], k
    if reason:
        assert (drep["ended"], drep["reason"], drep["dual_pivots"], drep["log_written"]) == (3, reason, 0, 0), drep
    else:
        want_end = ref.run(budget)
        assert (drep["ended"], drep["reason"], drep["dual_pivots"]) == (want_end, 0, len(ref.log)), (drep, want_end, len(ref.log))
        assert drep["sweeps"] + drep["walks"] == drep["dual_pivots"]
        keep = min(len(ref.log), 4096)
        assert drep["log_written"] == keep and log.tolist() == [list(t) for t in ref.log[:keep]]
        turned = ref.art_basic & (ref.art_flow < 0)
        assert drep["violations_after"] == int((ref.violations()[~turned] > 0).sum())
        assert drep["wrong_way_after"] == ref.wrong_way()
        if want_end == 0 and drep["wrong_way_after"] == 0 and not turned.any():
            # ---- path 0 on the basis the phase left: the reference's final basis, array by array
            assert rep["path"] == 0 and rep["tree_violations"] == 0, rep
            tree, res = eng.tree(), eng.result()
            n = inst.n
            for k, want in (("parent", ref.parent), ("pred_arc", ref.pred_arc), ("size", ref.size), ("depth", ref.depth)):
                assert np.array_equal(tree[k][:n], want[:n]), k
            assert np.array_equal(tree["state"], ref.state) and np.array_equal(res.flow, ref.flow)
            assert np.array_equal(eng.reduced_costs()[0], ref.reduced_costs())
            _after_repair(eng, cur)
            if resolve:
                _resolve_equals_fresh(e, eng, cur, rule, kw, stats0["pivots"], expect_pivots=0)
            return rep, drep, log, ref
    # ---- the repair of mcf_update_rhs picked up the rest (or all of it)
    if rep["path"] == 1:
        _after_repair(eng, cur)
    if resolve:
        _resolve_equals_fresh(e, eng, cur, rule, kw, stats0["pivots"])
    return rep, drep, log, ref


def _edit(inst, r0, tree, case):
    """The three edits of test_path1_repairs_and_resolves."""
    supply, cap = inst.supply.astype(np.int64).copy(), inst.cap.astype(np.int64).copy()
    if case == "cut_capacity":
        a = int(np.nonzero((tree["state"] == 0) & (r0.flow > 1))[0][0])
        cap[a] = int(r0.flow[a]) // 2
    elif case == "move_too_much":
        u, w, dmax = _first_pair(tree, inst, r0)
        supply[u] -= dmax + 5; supply[w] += dmax + 5
    else:
        rng = np.random.default_rng(5)
        idx = rng.choice(inst.n, max(2, inst.n // 20), replace=False)
        new = rng.integers(-50, 51, idx.size)
        new[-1] -= int(new.sum()) - int(supply[idx].sum())
        supply[idx] = new
    return supply, cap


# ------------------------------------------------------------------ every path, the three edits
@pytest.mark.parametrize("case", ("cut_capacity", "move_too_much", "redraw"))
@pytest.mark.parametrize("path,rule", DUAL_CASES, ids=DUAL_IDS)
def test_dual_phase_on_every_path(gpu_engine_module, path, rule, case, capsys):
    e = gpu_engine_module
    kw, _, mode, (n, m) = DUAL_PATHS[path]
    inst = generators.netgen_style(n, m, seed=11)
    with _engine(e, inst, rule, **kw) as eng:
        eng.solve()
        r0, tree = eng.result(), eng.tree()
        assert r0.status == "optimal" and r0.stats["pricing_mode"] == mode
        supply, cap = _edit(inst, r0, tree, case)
        rep, drep, log, ref = _dual_matches(e, eng, inst, supply, cap, rule, kw)
        with capsys.disabled():
            print(f"\n  [update_rhs_dual {path} rule {rule} {case}] ended {drep['ended']} reason {drep['reason']}: {drep['violations_before']} "
                  f"violations, {drep['dual_pivots']} dual pivots ({drep['sweeps']} sweeps, {drep['walks']} walks), path {rep['path']}", flush=True)


# ------------------------------------------------------------------ sweep and walk choose the same arcs
@pytest.mark.parametrize("path", ("grid_dense", "grid_blocked_4", "blocked_rebuild", "gather"))
def test_sweep_and_walk_write_the_same_log(gpu_engine_module, path):
    e = gpu_engine_module
    kw, rules, _, (n, m) = DUAL_PATHS[path]
    inst = generators.netgen_style(n, m, seed=11)
    logs = []
    for walk in (-1, 1 << 30, 8):
        with _engine(e, inst, rules[0], **kw) as eng:
            eng.solve()
            r0, tree = eng.result(), eng.tree()
            supply, cap = _edit(inst, r0, tree, "move_too_much")
            out = {}
            _dual_matches(e, eng, inst, supply, cap, rules[0], kw, enter_walk=walk, resolve=False, out=out)
            d = out["drep"]
            assert d["dual_pivots"] >= 1
            assert (d["walks"] == 0) if walk < 0 else ((d["sweeps"] == 0) if walk > 8 else True)
            logs.append(out["log"].tolist())
    assert logs[0] == logs[1] == logs[2]


# ------------------------------------------------------------------ budgets: the log is a prefix, path 1 takes over
@pytest.mark.parametrize("budget", (1, 2, 3))
@pytest.mark.parametrize("path", ("grid_dense", "grid_blocked_7"))
def test_budget_hands_over_to_the_repair(gpu_engine_module, path, budget):
    e = gpu_engine_module
    kw, rules, _, (n, m) = DUAL_PATHS[path]
    inst = generators.netgen_style(n, m, seed=11)
    with _engine(e, inst, 2, **kw) as eng:
        eng.solve()
        r0, tree = eng.result(), eng.tree()
        supply, cap = _edit(inst, r0, tree, "cut_capacity")
        full = _reference(inst, tree, supply, cap)
        full.run(BIG)
        assert len(full.log) > 3
        rep, drep, log, ref = _dual_matches(e, eng, inst, supply, cap, 2, kw, budget=budget)
        assert (drep["ended"], drep["dual_pivots"]) == (2, budget) and log.tolist() == [list(t) for t in full.log[:budget]]
        assert rep["path"] == 1


# ------------------------------------------------------------------ one planted case per `ended` and per `reason`
def test_reason_1_no_violations(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(700, 6000, seed=11)
    with _engine(e, inst, 0, **GRID) as eng, _engine(e, inst, 0, **GRID) as twin:
        eng.solve(); twin.solve()
        r0, tree = eng.result(), eng.tree()
        u, w, dmax = _first_pair(tree, inst, r0)
        supply = inst.supply.astype(np.int64).copy()
        supply[u] -= 1; supply[w] += 1
        rep, drep, log = eng.update_rhs_dual([u, w], [supply[u], supply[w]], log_cap=4)
        want = twin.update_rhs([u, w], [supply[u], supply[w]])
        assert (drep["ended"], drep["reason"], drep["dual_pivots"]) == (3, 1, 0) and log.shape == (0, 4)
        _same_handle(eng, twin, rep, want)


def _same_handle(eng, twin, rep, want):
    """`eng` after mcf_update_rhs_dual is exactly what mcf_update_rhs left of `twin`."""
    assert {k: v for k, v in rep.items() if k != "device_ms"} == {k: v for k, v in want.items() if k != "device_ms"}
    a, b = _snapshot(eng), _snapshot(twin)
    for k in TREE_KEYS + ("pi",):
        assert np.array_equal(a["tree"][k], b["tree"][k]), k
    assert np.array_equal(a["res"].flow, b["res"].flow) and a["res"].objective == b["res"].objective
    assert np.array_equal(eng.reduced_costs()[0], twin.reduced_costs()[0]) and np.array_equal(eng.pricing_keys()[0], twin.pricing_keys()[0])
    sa, sb = eng.stats(), twin.stats()
    assert {k: v for k, v in sa.items() if not k.endswith("seconds") and not k.endswith("_ms")} == \
           {k: v for k, v in sb.items() if not k.endswith("seconds") and not k.endswith("_ms")}


@pytest.mark.parametrize("path", ("small", "mid"))
def test_reason_2_persistent_loops(gpu_engine_module, path):
    e = gpu_engine_module
    kw, _, mode, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=11)
    with _engine(e, inst, 0, **kw) as eng, _engine(e, inst, 0, **kw) as twin:
        eng.solve(); twin.solve()
        r0, tree = eng.result(), eng.tree()
        assert r0.stats["pricing_mode"] == mode
        supply, cap = _edit(inst, r0, tree, "cut_capacity")
        rep, drep, _ = _call(eng, inst, supply, cap, log_cap=8)
        a = np.nonzero(cap != inst.cap)[0]
        want = twin.update_rhs(arcs=a, caps=cap[a])
        assert (drep["ended"], drep["reason"], drep["dual_pivots"]) == (3, 2, 0) and drep["violations_before"] >= 1
        _same_handle(eng, twin, rep, want)
        _resolve_equals_fresh(e, eng, _edited(inst, supply, cap), 0, kw, r0.stats["pivots"])


def test_reason_3_not_dual_feasible(gpu_engine_module):
    """An arc at capacity with a negative reduced cost is closed (capacity 0): it goes back to its lower bound, where its slack
    is negative.  A cut capacity in the same call makes sure there is a violation to begin with."""
    e = gpu_engine_module
    inst = generators.netgen_style(700, 6000, seed=11)
    with _engine(e, inst, 0, **GRID) as eng, _engine(e, inst, 0, **GRID) as twin:
        eng.solve(); twin.solve()
        r0, tree = eng.result(), eng.tree()
        rc = eng.reduced_costs()[0]
        supply, cap = _edit(inst, r0, tree, "cut_capacity")
        closed = int(np.nonzero((tree["state"] == -1) & (rc < 0))[0][0])
        cap[closed] = 0
        ref = _reference(inst, tree, supply, cap)
        assert _expected_start(ref)[1] == 3
        rep, drep, _ = _call(eng, inst, supply, cap, log_cap=8)
        a = np.nonzero(cap != inst.cap)[0]
        want = twin.update_rhs(arcs=a, caps=cap[a])
        assert (drep["ended"], drep["reason"], drep["dual_pivots"]) == (3, 3, 0), drep
        _same_handle(eng, twin, rep, want)
        _resolve_equals_fresh(e, eng, _edited(inst, supply, cap), 0, GRID, r0.stats["pivots"])


def test_reason_4_artificial_arc_turned(gpu_engine_module):
    """Supply moved between two nodes that hang on the root turns an artificial arc round; a capacity cut below the flow of a
    basic arc in the same call is the violation the phase would otherwise start on."""
    e = gpu_engine_module
    inst = generators.netgen_style(700, 6000, seed=11)
    with _engine(e, inst, 0, **GRID) as eng, _engine(e, inst, 0, **GRID) as twin:
        eng.solve(150); twin.solve(150)                       # mid-solve: subtrees still hang on artificial arcs with flow
        r0, tree = eng.result(), eng.tree()
        hanging = np.nonzero(tree["pred_arc"][:inst.n] >= inst.m)[0]
        assert hanging.size >= 2
        supply, cap = inst.supply.astype(np.int64).copy(), inst.cap.astype(np.int64).copy()
        big = int(np.abs(inst.supply).sum()) + 1
        supply[hanging[0]] -= big; supply[hanging[1]] += big  # both subtree sums change sign or grow: at least one arc turns
        a = int(np.nonzero((tree["state"] == 0) & (r0.flow > 1))[0][0])
        cap[a] = int(r0.flow[a]) // 2
        rep, drep, _ = eng.update_rhs_dual(hanging[:2], supply[hanging[:2]], [a], [cap[a]], log_cap=8)
        want = twin.update_rhs(hanging[:2], supply[hanging[:2]], [a], [cap[a]])
        assert want["tree_violations"] >= 1 and want["art_flips"] >= 1, want
        assert (drep["ended"], drep["reason"], drep["dual_pivots"]) == (3, 4, 0), drep
        assert drep["violations_before"] == want["tree_violations"]
        _same_handle(eng, twin, rep, want)
        _resolve_equals_fresh(e, eng, _edited(inst, supply, cap), 0, GRID, r0.stats["pivots"])


@pytest.mark.parametrize("rule", (0, 2))
def test_ended_1_starved_sink(gpu_engine_module, rule):
    """Starving in the manner of verdict_instances' "starved" variant, by supply: the node whose incoming arcs hold the least
    capacity is asked to take 5 units more than all of them carry.  The edited instance needs artificial flow; the phase
    saturates arc after arc into the sink, stops at the cut without an entering arc, and the repair takes over.  (Closing the
    arcs instead, as the variant itself does, flips arcs at capacity to a negative slack: that is reason 3, planted below.)"""
    e = gpu_engine_module
    inst = generators.netgen_style(120, 900, seed=11)
    assert ((inst.cap > 0) & (inst.cap < INF)).all()
    into = np.zeros(inst.n, np.int64)
    np.add.at(into, inst.head, inst.cap)
    sink, src = int(np.argmin(into)), int(np.argmax(inst.supply))
    supply = inst.supply.astype(np.int64).copy()
    d = int(into[sink]) + 5 + int(supply[sink])
    supply[sink] -= d; supply[src] += d
    with _engine(e, inst, rule, **GRID) as eng:
        eng.solve()
        r0 = eng.result()
        assert r0.status == "optimal" and r0.stats["pricing_mode"] in (0, 1)
        out = {}
        _dual_matches(e, eng, inst, supply, inst.cap.astype(np.int64), rule, GRID, out=out)
        assert out["drep"]["ended"] == 1 and out["drep"]["dual_pivots"] >= 1 and out["rep"]["path"] == 1, out["drep"]
        assert eng.result().status == "infeasible"


# ------------------------------------------------------------------ deep trees: cycles longer than the LDS buffers
def _chain(n, span):
    """A chain 0 -> 1 -> ... -> n-1 that carries 10 units, and chords i -> i + span that cost more than the chain they skip:
    the optimal tree is the chain, and the arc that relieves a cut chain arc closes a cycle of `span` + 1 arcs."""
    tail = list(range(n - 1)); head = list(range(1, n))
    cost = [1] * (n - 1); cap = [100] * (n - 1)
    for i in range(0, n - span, max(1, span // 3)):
        tail.append(i); head.append(i + span); cost.append(span + 5 + (i % 7)); cap.append(100)
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = 10, -10
    return ArcSoA(n, np.array(tail, np.int32), np.array(head, np.int32), np.array(cost, np.int64), np.array(cap, np.int64), supply, f"chain_{n}_{span}")


@pytest.mark.parametrize("cycle_scan", (1, -1))
@pytest.mark.parametrize("n,span", ((1600, 700), (9000, 5000)))
def test_deep_trees(gpu_engine_module, n, span, cycle_scan):
    """1 600 nodes: the cycle exceeds the 512 path entries kept in LDS; 9 000: it exceeds the 4 096 LDS hit entries."""
    e = gpu_engine_module
    inst = _chain(n, span)
    kw = dict(fused=False, mid_loop=-1, cycle_scan=cycle_scan)
    with _engine(e, inst, 0, **kw) as eng:
        # the chain is the optimal basis: installed, not pivoted to (a cold start climbs n arcs deep n times)
        in_tree = np.zeros(inst.m, np.int8)
        in_tree[:n - 1] = 1
        assert eng.set_basis(in_tree, np.zeros(inst.m, np.int8))
        eng.solve()
        r0 = eng.result()
        assert r0.status == "optimal" and r0.stats["pivots"] == 0 and int(eng.tree()["depth"].max()) >= n // 2
        cap = inst.cap.astype(np.int64).copy()
        cap[n // 2] = 4                                           # the chain arc n/2 -> n/2 + 1 carried 10
        out = {}
        _dual_matches(e, eng, inst, inst.supply.astype(np.int64), cap, 0, kw, resolve=False, out=out)
        d = out["drep"]
        assert d["ended"] == 0 and d["dual_pivots"] >= 1 and out["rep"]["path"] == 0, d
        ent = out["log"][:, 1]
        assert (inst.head[ent] - inst.tail[ent] == span).all()      # chords entered: cycles of span + 1 arcs
        eng.solve()
        got = eng.result()
        assert got.status == "optimal" and got.stats["pivots"] == 0 and got.objective == int((out["ref"].flow * inst.cost).sum())
        cert = eng.certify()
        assert cert["verdict"] == "optimal" and cert["proves_status"]
        # ... and equals a fresh cold solve of the edited instance (that handle with the scan on whatever `cycle_scan` is here:
        # a climb-only cold start of the 9 000 chain walks n arcs n times, half a minute)
        want = _fresh(e, _edited(inst, cap=cap), 0, dict(fused=False, mid_loop=-1, cycle_scan=1))
        _same_optimum(_edited(inst, cap=cap), got, want)


# ------------------------------------------------------------------ geometry and magnitudes
@pytest.mark.parametrize("n,m", ((257, 1501), (513, 4099)))
def test_just_over_a_workgroup_and_odd_arc_counts(gpu_engine_module, n, m):
    """n just over one / two workgroups of k_dual_leave; arc counts that are no multiple of 4 or 8, so that bucket boundaries
    fall inside groups of arcs."""
    e = gpu_engine_module
    inst = generators.netgen_style(n, m, seed=5)
    for case in ("cut_capacity", "move_too_much"):
        with _engine(e, inst, 0, **GRID) as eng:
            eng.solve()
            r0, tree = eng.result(), eng.tree()
            assert r0.stats["pricing_mode"] in (0, 1)
            supply, cap = _edit(inst, r0, tree, case)
            _dual_matches(e, eng, inst, supply, cap, 0, GRID)


def test_wide_range_magnitudes(gpu_engine_module):
    e = gpu_engine_module
    inst = wri.make(1, *wri.SIZES["small"])
    with _engine(e, inst, 0, **GRID) as eng:
        eng.solve()
        r0, tree = eng.result(), eng.tree()
        assert r0.status == "optimal"
        supply, cap = inst.supply.astype(np.int64).copy(), inst.cap.astype(np.int64).copy()
        basic = np.nonzero((tree["state"] == 0) & (r0.flow > (1 << 20)))[0]
        assert basic.size
        cap[basic[0]] = int(r0.flow[basic[0]]) // 3                # a violation of the instance's own magnitude
        out = {}
        _dual_matches(e, eng, inst, supply, cap, 0, GRID, out=out)
        assert out["drep"]["violations_before"] >= 1 and out["drep"]["ended"] in (0, 1, 2)
        if out["log"].size:
            assert int(out["log"][:, 2].max()) > (1 << 20)


# ------------------------------------------------------------------ refusals leave the handle as it was
def test_refusals_change_nothing(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(700, 6000, seed=4)
    with _engine(e, inst, 2, **GRID) as eng, _engine(e, inst, 2, **GRID) as twin:
        eng.solve(200); twin.solve(200)
        before, rc0, st0 = _snapshot(eng), eng.reduced_costs()[0], eng.stats()
        big = np.zeros(inst.n, np.int64)
        big[0], big[1] = INF, -INF
        bad = [
            (dict(nodes=[0], supplies=[int(inst.supply[0]) + 1]), -5),                       # unbalanced
            (dict(nodes=np.arange(inst.n), supplies=big), -5),                               # positive part reaches 2^60
            (dict(nodes=[inst.n], supplies=[0]), -1), (dict(nodes=[-1], supplies=[0]), -1),  # index out of range
            (dict(arcs=[inst.m], caps=[1]), -1),
        ]
        for args, code in bad:
            with pytest.raises(e.EngineError) as err:
                eng.update_rhs_dual(**args)
            assert err.value.code == code
        i64p = ctypes.POINTER(ctypes.c_int64)
        call = eng._lib.mcf_update_rhs_dual
        assert call(eng._h, 1, i64p(), i64p(), 0, i64p(), i64p(), None, None, 0, None, None) == -1      # null arrays
        assert call(eng._h, -1, i64p(), i64p(), 0, i64p(), i64p(), None, None, 0, None, None) == -1
        assert call(eng._h, 0, i64p(), i64p(), 0, i64p(), i64p(), None, None, 4, None, None) == -1      # a log capacity without a log
        assert call(eng._h, 0, i64p(), i64p(), 0, i64p(), i64p(), None, None, -1, None, None) == -1
        assert call(None, 0, i64p(), i64p(), 0, i64p(), i64p(), None, None, 0, None, None) == -1
        after = _snapshot(eng)
        assert np.array_equal(after["res"].flow, before["res"].flow) and after["res"].objective == before["res"].objective
        for k in TREE_KEYS + ("pi",):
            assert np.array_equal(after["tree"][k], before["tree"][k]), k
        assert np.array_equal(eng.reduced_costs()[0], rc0)
        st1 = eng.stats()
        assert {k: v for k, v in st1.items() if not k.endswith("seconds")} == {k: v for k, v in st0.items() if not k.endswith("seconds")}
        eng.solve(); twin.solve()
        a, b = eng.result(), twin.result()
        assert a.stats["pivots"] == b.stats["pivots"] and a.objective == b.objective and np.array_equal(a.flow, b.flow)
    with _engine(e, inst, 0, shard=(0, 2)) as sh:
        with pytest.raises(e.EngineError) as err:
            sh.update_rhs_dual([0, 1], [1, -1])
        assert err.value.code == -6


# ------------------------------------------------------------------ the shim
def test_shim_on_an_object_problem(gpu_engine_module):
    options = nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True)
    nodes = [dict(id="a", supply=10.5), dict(id="b", supply=0.0), dict(id="c", supply=-4.0), dict(id="d", supply=-6.5)]
    arcs = [dict(tail="a", head="b", capacity=8.0, cost=1.25, lower=1.5), dict(tail="a", head="c", capacity=6.0, cost=4.0, lower=0.0),
            dict(tail="b", head="c", capacity=5.0, cost=1.0, lower=0.0), dict(tail="b", head="d", capacity=9.0, cost=2.5, lower=0.5),
            dict(tail="c", head="d", capacity=None, cost=1.0, lower=0.0), dict(tail="a", head="d", capacity=3.0, cost=9.0, lower=0.0)]
    solver = nfs.NetworkSimplex(nfs.build_problem(nodes, arcs, True, 1e-6), options)
    assert solver.solve().status == "optimal"
    plain = solver.update_supplies({"a": 10.5, "d": -6.5})
    assert "dual" not in plain
    rep = solver.update_supplies({"a": 12.5, "d": -8.5}, dual=True)
    # four nodes: the handle runs as a persistent loop, where the phase is not attempted (the call is then update_supplies)
    d = rep["dual"]
    assert rep["path"] in (0, 1) and (d["ended"], d["dual_pivots"]) == (3, 0) and d["reason"] == (2 if d["violations_before"] else 1), d
    rep = solver.update_capacities({("a", "b"): 6.5, ("c", "d"): 4.0, ("a", "d"): None}, dual=True)
    assert rep["dual"]["ended"] == 3 and rep["dual"]["reason"] in (1, 2)
    second = solver.solve()
    new_nodes = [dict(nd) for nd in nodes]
    new_nodes[0]["supply"], new_nodes[3]["supply"] = 12.5, -8.5
    new_arcs = [dict(a) for a in arcs]
    new_arcs[0]["capacity"], new_arcs[4]["capacity"], new_arcs[5]["capacity"] = 6.5, 4.0, None
    rebuilt = nfs.build_problem(new_nodes, new_arcs, True, 1e-6)
    assert solver.problem == rebuilt
    want = nfs.NetworkSimplex(rebuilt, options).solve()
    assert second.status == want.status == "optimal" and second.objective == want.objective
    assert solver.certify().verdict == "optimal"


def test_shim_on_an_soa_problem(gpu_engine_module):
    inst = generators.netgen_style(3000, 24000, seed=8)            # (large enough for a grid handle: the phase runs)
    lower = np.zeros(inst.m, np.int64)
    lower[::7] = 1
    cap = np.where(inst.cap >= 0, inst.cap + lower, inst.cap)
    problem = SoAProblem(inst.n, inst.tail, inst.head, inst.cost, cap, inst.supply, lower)
    options = nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True)
    solver = nfs.NetworkSimplex(problem, options)
    first = solver.solve()
    assert first.status == "optimal"
    # capacities first, on the optimal (dual feasible) state: five basic arcs cut to half their flow -- the phase has to run
    res0, state0 = solver.engine.result(), solver.engine.tree()["state"]
    assert res0.stats["pricing_mode"] in (0, 1)
    arcs = np.nonzero((state0 == 0) & (res0.flow > 1))[0][:5]
    assert arcs.size == 5
    new_cap = cap.copy()
    new_cap[arcs] = lower[arcs] + res0.flow[arcs] // 2
    rep = solver.update_capacities((arcs, new_cap[arcs]), dual=True)
    d = rep["dual"]
    assert d["violations_before"] >= 1 and d["reason"] == 0 and d["ended"] in (0, 1, 2) and d["dual_pivots"] >= 1, d
    supply = problem.supply.copy()
    src, dst = int(np.argmax(supply)), int(np.argmin(supply))
    supply[src] += 40; supply[dst] -= 40
    rep2 = solver.update_supplies(([src, dst], [supply[src], supply[dst]]), dual=True)
    assert rep2["dual"]["ended"] in (0, 1, 2, 3)
    second = solver.solve()
    want = nfs.NetworkSimplex(SoAProblem(inst.n, inst.tail, inst.head, inst.cost, new_cap, supply, lower), options).solve()
    assert second.status == want.status and second.objective == want.objective
