"""Adding arcs to a resident handle (``mcf_add_arcs``, ``-m gpu``).

Everything goes through the C ABI.  A fresh handle that received arcs is held against a handle created with the extended
instance (every introspection array, then the whole solve: same pivots); a solved handle is checked clause by clause against
what it held before the call; re-solves are held against the oracle.  Every comparison is exact.  ``price_blocks`` (and
``block_size`` for Devex) are pinned wherever two handles are compared: their automatic values depend on m."""

import numpy as np
import pytest

import oracle
import verdict_instances as vi
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

pytestmark = pytest.mark.gpu
INF = 1 << 60
PIN = dict(price_blocks=16, block_size=300)
GRAPH = dict(fused=False, mid_loop=-1)
FAMILIES = {
    "lds": ((64, 512), dict()),
    "mid": ((256, 2048), dict(mid_loop=1)),
    "graph": ((1000, 8000), dict(GRAPH)),
    "blocked": ((1000, 8000), dict(GRAPH, tree_blocks=6)),
    "keycodes": ((1000, 8000), dict(GRAPH, compressed_keys=1, full_sweeps=-1)),
    "gather": ((1000, 8000), dict(GRAPH, resident_rc=False)),
    "priority": ((1000, 8000), dict(GRAPH, key_mode=2)),
}
RULES = {"dantzig": 0, "devex": 1, "candidate": 2}
CASES = [(f, r) for f in FAMILIES for r in RULES if not (f == "priority" and r == "devex")]
IDS = [f"{f}-{r}" for f, r in CASES]
TREE_KEYS = ("parent", "size", "pos", "order", "depth", "psize")


def _inst(family, seed=3):
    (n, m), _ = FAMILIES[family]
    return generators.netgen_style(n, m, seed=seed)


def _prio(m, seed=9):
    return np.random.default_rng([31, seed, m]).integers(0, 4, m).astype(np.int8)


def _engine(e, inst, family, rule, prio=None, **extra):
    kw = dict(FAMILIES[family][1], **PIN)
    kw.update(extra)
    if kw.get("key_mode") == 2:
        kw["arc_priority"] = _prio(inst.m) if prio is None else prio
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=RULES[rule], **kw)


def _extra(inst, k, seed=1, parallel=0):
    """k new arcs: random end points, costs and capacities drawn like the instance's; the first `parallel` repeat existing pairs."""
    rng = np.random.default_rng([41, seed, inst.n, k])
    t = rng.integers(0, inst.n, k).astype(np.int32)
    h = ((t + 1 + rng.integers(0, inst.n - 1, k)) % inst.n).astype(np.int32)
    if parallel:
        pick = rng.choice(inst.m, parallel)
        t[:parallel], h[:parallel] = inst.tail[pick], inst.head[pick]
    cost = rng.choice(inst.cost, k).astype(np.int64) if inst.m else rng.integers(1, 100, k)
    cap = rng.choice(inst.cap, k).astype(np.int64) if inst.m else rng.integers(1, 100, k)
    return t, h, cost, cap


def _one_per_bucket(inst):
    per = (inst.n + 7) // 8
    h = (np.arange(8) * per).astype(np.int32)
    h = np.minimum(h, inst.n - 1).astype(np.int32)
    t = ((h + 3) % inst.n).astype(np.int32)
    return t, h, np.arange(1, 9, dtype=np.int64), np.full(8, 5, np.int64)


def _extended(inst, t, h, c, cp, name="extended"):
    return ArcSoA(inst.n, np.concatenate([inst.tail, t]).astype(np.int32), np.concatenate([inst.head, h]).astype(np.int32),
                  np.concatenate([inst.cost, c]).astype(np.int64), np.concatenate([inst.cap, cp]).astype(np.int64), inst.supply,
                  inst.name + "_" + name)


def _introspect(eng):
    rc, resident = eng.reduced_costs()
    keys, present = eng.pricing_keys()
    return {"tree": eng.tree(), "rc": rc, "resident": resident, "keys": keys, "present": present, "weights": eng.weights()}


def _assert_same_introspection(a, b):
    for k in a["tree"]:
        assert np.array_equal(a["tree"][k], b["tree"][k]), k
    assert a["resident"] == b["resident"] and a["present"] == b["present"]
    assert np.array_equal(a["rc"], b["rc"]) and np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["weights"], b["weights"])


def _assert_same_solve(a, b):
    ra, rb = a.result(), b.result()
    assert ra.status == rb.status and ra.objective == rb.objective
    assert ra.stats["pivots"] == rb.stats["pivots"] and ra.stats["degenerate"] == rb.stats["degenerate"]
    assert ra.stats["pricing_mode"] == rb.stats["pricing_mode"]
    assert np.array_equal(ra.flow, rb.flow) and np.array_equal(ra.potential, rb.potential) and np.array_equal(ra.in_tree, rb.in_tree)
    return ra


def _fresh_equals_create(e, family, rule, inst, lists, prio_new=None):
    """`lists`: successive mcf_add_arcs calls on one fresh handle, against one mcf_create of the base plus all of them."""
    t, h, c, cp = (np.concatenate([x[i] for x in lists]) for i in range(4))
    ext = _extended(inst, t, h, c, cp)
    is_prio = FAMILIES[family][1].get("key_mode") == 2
    pr_old = _prio(inst.m) if is_prio else None
    pr_new = _prio(len(t), seed=17) if is_prio else None
    with _engine(e, inst, family, rule, prio=pr_old) as a, \
            _engine(e, ext, family, rule, prio=np.concatenate([pr_old, pr_new]) if is_prio else None) as b:
        at, top = 0, int(np.abs(inst.cost).max()) if inst.m else 0
        reports = []
        for x in lists:
            k = len(x[0])
            rep = a.add_arcs(*x, priority=pr_new[at:at + k] if is_prio else None)
            assert rep["first_index"] == inst.m + at and rep["m"] == inst.m + at + k
            assert rep["bigm_grew"] == int(int(np.abs(x[2]).max()) > top)      # big-M = (max|cost| + 1) * (n + 2)
            top = max(top, int(np.abs(x[2]).max()))
            at += k
            reports.append(rep)
        assert a.m == ext.m
        _assert_same_introspection(_introspect(a), _introspect(b))
        a.solve(); b.solve()
        res = _assert_same_solve(a, b)
        res.stats["add_reports"] = reports
        return res


# ------------------------------------------------------------------ fresh handle equals create
@pytest.mark.parametrize("family,rule", CASES, ids=IDS)
def test_fresh_handle_plus_arcs_equals_create(gpu_engine_module, family, rule):
    inst = _inst(family)
    k = 40 if family == "lds" else 300
    res = _fresh_equals_create(gpu_engine_module, family, rule, inst, [_extra(inst, k, parallel=k // 4)])
    assert res.status == "optimal"
    assert res.objective == int(round(oracle.solve_soa(_extended(inst, *_extra(inst, k, parallel=k // 4)), "dantzig")["objective"]))


SHAPES = [(f, s) for f in ("lds", "graph", "blocked") for s in ("one", "one_per_bucket", "k_gt_m", "pad_crossing", "parallel", "two_calls")]
SHAPES.append(("lds", "empty_base"))   # (a graph-path handle created without arcs keeps no reduced costs: not what create would build)


@pytest.mark.parametrize("family,shape", SHAPES, ids=[f"{f}-{s}" for f, s in SHAPES])
def test_fresh_handle_shapes(gpu_engine_module, family, shape):
    inst = _inst(family)
    if shape == "one":
        lists = [_extra(inst, 1)]
    elif shape == "one_per_bucket":
        lists = [_one_per_bucket(inst)]
    elif shape == "k_gt_m":
        inst = generators.netgen_style(60, 300, seed=4)
        lists = [_extra(inst, 420, seed=2)]
    elif shape == "pad_crossing":
        inst = generators.netgen_style(60, 1020, seed=5)     # m_pad goes from 1024 to 2048
        assert inst.m == 1020
        lists = [_extra(inst, 10)]
    elif shape == "parallel":
        lists = [_extra(inst, 64, parallel=64)]
    elif shape == "two_calls":
        lists = [_extra(inst, 33, seed=5), _extra(inst, 47, seed=6, parallel=10)]
    else:
        base = generators.netgen_style(60, 300, seed=4)
        inst = ArcSoA(base.n, base.tail[:0], base.head[:0], base.cost[:0], base.cap[:0], base.supply, "no_arcs")
        lists = [(base.tail, base.head, base.cost, base.cap)]
    reports = _fresh_equals_create(gpu_engine_module, family, "candidate", inst, lists).stats["add_reports"]
    # chunks of 1 024 old arcs whose offset is the same at both ends take the shifted-copy path and are counted
    if shape == "one":
        chunks = -(-inst.m // 1024)
        assert inst.m - 1024 <= reports[0]["shifted_only"] <= inst.m and (chunks < 8 or reports[0]["shifted_only"] >= 6 * 1024)
    if shape == "pad_crossing":
        # one chunk; its first and its last old arc keep apart unless every new arc sorts before or after all of them
        t0, tn = _extra(inst, 10)[0:2]
        per = (inst.n + 7) // 8
        keys_new = (tn // per).astype(np.int64) << 32 | t0
        keys_old = (inst.head // per).astype(np.int64) << 32 | inst.tail
        split = ((keys_new >= keys_old.min()) & (keys_new < keys_old.max())).any()
        assert reports[0]["shifted_only"] == (0 if split else inst.m) and split
    if shape in ("two_calls", "pad_crossing"):
        _fresh_equals_create(gpu_engine_module, family, "devex", inst, lists)


# ------------------------------------------------------------------ solved handle: every clause of "afterwards"
def _check_after(e, eng, inst, before, extra, rep, bigm_grew=False):
    t, h, c, cp = extra
    k, m = len(t), inst.m
    ext = _extended(inst, t, h, c, cp)
    after = _introspect(eng)
    tb, ta = before["tree"], after["tree"]
    for key in TREE_KEYS:
        assert np.array_equal(tb[key], ta[key]), key
    pred_b, pred_a = tb["pred_arc"].astype(np.int64), ta["pred_arc"].astype(np.int64)
    assert np.array_equal(np.where(pred_b >= m, pred_b + k, pred_b), pred_a)
    assert np.array_equal(ta["state"][:m], tb["state"][:m]) and (ta["state"][m:] == 1).all()
    if not bigm_grew:
        assert np.array_equal(ta["pi"], tb["pi"])
        assert np.array_equal(after["rc"][:m], before["rc"][:m])
        assert np.array_equal(after["keys"][:m], before["keys"][:m])
    assert after["resident"] == before["resident"] and after["present"] == before["present"]
    want_rc = ext.cost + ta["pi"][ext.tail] - ta["pi"][ext.head]
    assert np.array_equal(after["rc"], want_rc)
    assert rep["eligible"] == int((want_rc[m:] < 0).sum())
    assert (after["weights"] == 1.0).all()
    res = eng.result()
    assert np.array_equal(res.flow[:m], before["flow"]) and not res.flow[m:].any()
    cert = eng.certify()
    for key in ("basic_count_mismatch", "tree_rc_count", "state_flow_count", "tree_shape_count", "strong_count", "rc_mismatch_count",
                "key_mismatch_count", "negative_flow_count", "over_capacity_count", "imbalance_count"):
        assert cert[key] == 0, key
    assert cert["basic_arcs"] == inst.n and cert["checks"] == 63 and cert["status"] == "running"
    if after["resident"]:
        assert cert["rc_compared"] == ext.m
    if after["present"]:
        assert cert["key_compared"] == ext.m
    return ext


@pytest.mark.parametrize("family,rule", CASES, ids=IDS)
def test_solved_handle_keeps_its_basis_and_resolves(gpu_engine_module, family, rule):
    inst = _inst(family)
    extra = _extra(inst, 25 if family == "lds" else 200, seed=8, parallel=5)
    is_prio = FAMILIES[family][1].get("key_mode") == 2
    with _engine(gpu_engine_module, inst, family, rule) as eng:
        eng.solve()
        r0 = eng.result()
        assert r0.status == "optimal"
        before = _introspect(eng)
        before["flow"] = r0.flow.copy()
        rep = eng.add_arcs(*extra, priority=_prio(len(extra[0]), seed=2) if is_prio else None)
        assert rep["first_index"] == inst.m and rep["m"] == inst.m + len(extra[0]) and rep["bigm_grew"] == 0
        ext = _check_after(gpu_engine_module, eng, inst, before, extra, rep)
        eng.solve()
        r1 = eng.result()
        cert = eng.certify()
        assert r1.status == "optimal" and cert["proves_status"] and cert["verdict"] == "optimal"
        assert r1.stats["pivots"] >= r0.stats["pivots"]          # the counters keep counting
        assert r1.objective == int(round(oracle.solve_soa(ext, "dantzig")["objective"]))


# ------------------------------------------------------------------ no pivot / must pivot
def _priced_out(inst, res, d):
    """For each basic real arc a -> b of cost c: a parallel arc of cost c + d and a reverse arc of cost -c + d (reduced cost d)."""
    basic = np.nonzero(res.in_tree)[0]
    assert len(basic) >= 8
    t = np.concatenate([inst.tail[basic], inst.head[basic]]).astype(np.int32)
    h = np.concatenate([inst.head[basic], inst.tail[basic]]).astype(np.int32)
    c = np.concatenate([inst.cost[basic], -inst.cost[basic]]).astype(np.int64)
    return t, h, c + d, np.full(len(t), 7, np.int64)


@pytest.mark.parametrize("family", ["lds", "mid", "graph", "blocked", "keycodes", "gather"])
def test_no_pivot_and_must_pivot(gpu_engine_module, family):
    inst = _inst(family)
    for rule in RULES:
        with _engine(gpu_engine_module, inst, family, rule) as eng:
            eng.solve()
            r0 = eng.result()
            t, h, c, cp = _priced_out(inst, r0, np.arange(2 * int(r0.in_tree.sum())) % 2)
            rep = eng.add_arcs(t, h, c, cp)
            assert rep["eligible"] == 0
            eng.solve()
            r1 = eng.result()
            cert = eng.certify()
            assert r1.stats["pivots"] == r0.stats["pivots"] and r1.status == "optimal" and r1.objective == r0.objective
            assert cert["proves_status"] and cert["verdict"] == "optimal"
            ext = _extended(inst, t, h, c, cp)
            # one more arc of reduced cost -1 parallel to a basic arc that carries flow below its capacity
            basic = np.nonzero(r1.in_tree[:inst.m])[0]
            a = int(basic[0])
            rep = eng.add_arcs([inst.tail[a]], [inst.head[a]], [inst.cost[a] - 1], [3])
            assert rep["eligible"] == 1
            eng.solve()
            r2 = eng.result()
            assert r2.stats["pivots"] >= r1.stats["pivots"] + 1 and r2.status == "optimal"
            ext2 = _extended(ext, np.array([inst.tail[a]]), np.array([inst.head[a]]), np.array([inst.cost[a] - 1]), np.array([3]))
            assert r2.objective == int(round(oracle.solve_soa(ext2, "dantzig")["objective"]))
            assert eng.certify()["proves_status"]


# ------------------------------------------------------------------ verdict changes
@pytest.mark.parametrize("rule", list(RULES))
def test_infeasible_repaired_by_new_arcs(gpu_engine_module, rule):
    # (quantities up to 2^16: the oracle's objective is a double and has to hold the exact value)
    inst = vi.infeasible(3, 60, 500, "isolated", qmax=1 << 16)
    whole = vi.uncapacitated(3, 60, 500, qmax=1 << 16)
    sink = int(np.argmin(inst.supply))
    gone = np.nonzero(whole.head == sink)[0]
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=RULES[rule], **PIN) as eng:
        eng.solve()
        assert eng.result().status == "infeasible"
        eng.add_arcs(whole.tail[gone], whole.head[gone], whole.cost[gone], whole.cap[gone])
        eng.solve()
        res = eng.result()
        ext = _extended(inst, whole.tail[gone], whole.head[gone], whole.cost[gone], whole.cap[gone])
        assert res.status == "optimal" and res.objective == int(round(oracle.solve_soa(ext, "dantzig")["objective"]))
        assert eng.certify()["proves_status"]


@pytest.mark.parametrize("rule", list(RULES))
def test_optimal_becomes_unbounded_with_a_proven_ray(gpu_engine_module, rule):
    full = vi.unbounded(2, 60, 500, cycle_len=5)
    cyc = vi.planted(full, 5)
    base = ArcSoA(full.n, full.tail[:-5], full.head[:-5], full.cost[:-5], full.cap[:-5], full.supply, "bounded")
    with gpu_engine_module.McfEngine(base.n, base.tail, base.head, base.cost, base.cap, base.supply, rule=RULES[rule], **PIN) as eng:
        eng.solve()
        assert eng.result().status == "optimal"
        eng.add_arcs(full.tail[cyc], full.head[cyc], full.cost[cyc], full.cap[cyc])
        eng.solve()
        assert eng.result().status == "unbounded"
        ray = eng.certify_ray()
        assert ray["proven"] and ray["cost"] < 0


@pytest.mark.parametrize("family,rule", [("lds", "dantzig"), ("mid", "devex"), ("graph", "candidate"), ("blocked", "dantzig"), ("gather", "devex")])
def test_mid_solve_handle_resumes_to_the_optimum(gpu_engine_module, family, rule):
    inst = _inst(family)
    extra = _extra(inst, 120, seed=12)
    with _engine(gpu_engine_module, inst, family, rule) as eng:
        eng.solve(max_pivots=inst.n // 2)
        assert eng.result().status == "iteration_limit"
        before = _introspect(eng)
        before["flow"] = eng.result().flow.copy()
        rep = eng.add_arcs(*extra)
        ext = _check_after(gpu_engine_module, eng, inst, before, extra, rep)
        eng.solve()
        res = eng.result()
        assert res.status == "optimal" and res.objective == int(round(oracle.solve_soa(ext, "dantzig")["objective"]))
        assert eng.certify()["proves_status"]


# ------------------------------------------------------------------ big-M
@pytest.mark.parametrize("family", ["lds", "graph", "blocked", "keycodes"])
def test_a_new_cost_that_raises_big_m(gpu_engine_module, family):
    inst = _inst(family)
    extra = list(_extra(inst, 50, seed=13))
    extra[2] = extra[2].copy()
    extra[2][7] = 50 * int(np.abs(inst.cost).max())
    with _engine(gpu_engine_module, inst, family, "candidate") as eng:
        eng.solve(max_pivots=inst.n // 3)                        # artificial arcs are still basic
        assert eng.result().status == "iteration_limit"
        assert (eng.tree()["pred_arc"][:inst.n] >= inst.m).any()
        before = _introspect(eng)
        before["flow"] = eng.result().flow.copy()
        rep = eng.add_arcs(*extra)
        assert rep["bigm_grew"] == 1
        ext = _check_after(gpu_engine_module, eng, inst, before, tuple(extra), rep, bigm_grew=True)
        assert eng.certify()["big_m"] == (int(extra[2][7]) + 1) * (inst.n + 2)
        eng.solve()
        res = eng.result()
        assert res.status == "optimal" and res.objective == int(round(oracle.solve_soa(ext, "dantzig")["objective"]))


# ------------------------------------------------------------------ interplay with the other resident calls
@pytest.mark.parametrize("family", ["lds", "graph", "blocked", "gather"])
def test_interplay_with_the_other_calls(gpu_engine_module, family):
    inst = _inst(family)
    t, h, c, cp = _extra(inst, 90, seed=14)
    with _engine(gpu_engine_module, inst, family, "dantzig") as eng:
        eng.solve()
        n_before = eng.bottlenecks()[1]
        cut_before = eng.certify_cut()
        assert not cut_before["proven"]
        eng.update_costs([3], [int(inst.cost[3])])               # builds the caller's-index map for the old m
        eng.add_arcs(t, h, c, cp)
        ext = _extended(inst, t, h, c, cp)
        assert eng.bottlenecks()[1] == n_before                  # the new arcs carry nothing
        assert eng.certify_cut()["nodes_in_S"] == cut_before["nodes_in_S"]
        cost = ext.cost.copy()
        old_arc, new_arc = 5, inst.m + 11
        cost[old_arc] += 2; cost[new_arc] -= 1
        eng.update_costs([old_arc, new_arc], [cost[old_arc], cost[new_arc]])
        cap = ext.cap.copy()
        cap[inst.m + 4] = 1
        eng.update_rhs(arcs=[inst.m + 4], caps=[1])
        ext2 = ArcSoA(ext.n, ext.tail, ext.head, cost, cap, ext.supply, "edited")
        tree = eng.tree()
        rc, _ = eng.reduced_costs()
        assert np.array_equal(rc, cost + tree["pi"][ext.tail] - tree["pi"][ext.head])
        eng.solve()
        res = eng.result()
        want = int(round(oracle.solve_soa(ext2, "dantzig")["objective"]))
        assert res.status == "optimal" and res.objective == want and eng.certify()["proves_status"]
        idx, count = eng.bottlenecks()
        assert count == int(((res.flow == cap) & (cap > 0) & (cap < INF)).sum()) and len(idx) == count
        eng.reset()
        eng.solve()
        with _engine(gpu_engine_module, ext2, family, "dantzig") as fresh:
            fresh.solve()
            _assert_same_solve(eng, fresh)


# ------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_handle_as_it_was(gpu_engine_module):
    e = gpu_engine_module
    inst = _inst("graph")
    with _engine(e, inst, "graph", "candidate") as eng, _engine(e, inst, "graph", "candidate") as twin:
        eng.solve(max_pivots=200); twin.solve(max_pivots=200)
        before = _introspect(eng)
        ok = ([1], [2], [5], [9])
        bad = {
            -1: [([inst.n], [0], [1], [1]), ([0], [-1], [1], [1]), ([4], [4], [1], [1])],
            -5: [([1], [2], [1 << 31], [1]), ([1], [2], [-(1 << 31)], [1])],
        }
        for code, calls in bad.items():
            for args in calls:
                with pytest.raises(e.EngineError) as err:
                    eng.add_arcs(*args)
                assert err.value.code == code, args
        one32, one64 = np.ones(1, np.int32), np.ones(1, np.int64)
        p32, p64 = one32.ctypes.data_as(e.ctypes.POINTER(e.ctypes.c_int32)), one64.ctypes.data_as(e.ctypes.POINTER(e.ctypes.c_int64))
        # m + count + n >= 2^30 is refused on the count alone, before an array is read
        assert eng._lib.mcf_add_arcs(eng._h, (1 << 30) - inst.n - inst.m, p32, p32, p64, p64, None, None) == -5
        assert eng._lib.mcf_add_arcs(None, 0, None, None, None, None, None, None) == -1
        assert eng._lib.mcf_add_arcs(eng._h, -1, None, None, None, None, None, None) == -1
        assert eng._lib.mcf_add_arcs(eng._h, 1, None, None, None, None, None, None) == -1
        assert eng.m == inst.m
        _assert_same_introspection(before, _introspect(eng))
        eng.solve(); twin.solve()
        _assert_same_solve(eng, twin)
        assert eng.add_arcs([], [], [], [])["m"] == inst.m       # count == 0 is valid


def test_big_m_limit_is_a_range_error(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(9000, 18000, seed=1)          # INT32_MAX is admissible up to n = 8 189 only
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2, **PIN) as eng:
        before = _introspect(eng)
        with pytest.raises(e.EngineError) as err:
            eng.add_arcs([1], [2], [(1 << 31) - 1], [1])
        assert err.value.code == -5 and eng.m == inst.m
        _assert_same_introspection(before, _introspect(eng))


def test_lds_handle_grown_past_its_capacity_and_sharded_handle(gpu_engine_module):
    e = gpu_engine_module
    inst = _inst("lds")
    with _engine(e, inst, "lds", "dantzig") as eng:
        eng.solve()
        assert eng.result().stats["pricing_mode"] == 2
        before = _introspect(eng)
        big = _extra(inst, 9000, seed=3)
        with pytest.raises(e.EngineError) as err:
            eng.add_arcs(*big)
        assert err.value.code == -6 and "LDS" in str(err.value)
        _assert_same_introspection(before, _introspect(eng))
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, shard=(0, 2), fused=False) as eng:
        with pytest.raises(e.EngineError) as err:
            eng.add_arcs([1], [2], [1], [1])
        assert err.value.code == -6


# ------------------------------------------------------------------ handles that gave their resident reduced costs up
@pytest.mark.parametrize("rule", ["devex", "candidate"])
def test_handle_that_dropped_its_reduced_costs(gpu_engine_module, rule):
    e = gpu_engine_module
    inst = generators.netgen_style(3000, 24000, seed=3)
    extra = _extra(inst, 400, seed=21, parallel=20)
    kw = dict(tree_blocks=4, rc_drop=1, **PIN)
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=RULES[rule], **kw) as eng:
        eng.solve()
        r0 = eng.result()
        assert r0.status == "optimal" and r0.stats["rc_dropped_at"] > 0 and r0.stats["pricing_mode"] == 0
        before = _introspect(eng)
        assert not before["resident"]
        before["flow"] = r0.flow.copy()
        rep = eng.add_arcs(*extra)
        ext = _check_after(e, eng, inst, before, extra, rep)
        assert eng.certify()["rc_compared"] == 0                         # it stays dropped
        eng.solve()
        r1 = eng.result()
        assert r1.status == "optimal" and r1.stats["pricing_mode"] == 0 and eng.certify()["proves_status"]
        assert r1.objective == int(round(oracle.solve_soa(ext, "dantzig")["objective"]))
        eng.reset()                                                      # a fresh start keeps them again, at the new size
        assert eng.reduced_costs()[1] and eng.certify()["rc_compared"] == ext.m and eng.certify()["rc_mismatch_count"] == 0
        eng.solve()
        assert eng.result().objective == r1.objective


# ------------------------------------------------------------------ past 4 M arcs: the non-temporal variant of the re-layout pass
def test_relayout_with_non_temporal_loads_from_4m_arcs(gpu_engine_module):
    e = gpu_engine_module
    n, m, k = 1 << 15, (1 << 22) + 3000, 2000
    rng = np.random.default_rng(7)
    t = rng.integers(0, n, m + k).astype(np.int32)
    h = ((t + 1 + rng.integers(0, n - 1, m + k)) % n).astype(np.int32)
    c = rng.integers(-50, 1000, m + k).astype(np.int64)
    c[m:] = rng.integers(-50, 1000, k)                                   # (big-M stays: |cost| <= 1000 already occurs)
    c[0] = 1000
    cp = rng.integers(0, 100, m + k).astype(np.int64)
    supply = np.zeros(n, np.int64)
    supply[:100], supply[100:200] = 7, -7
    kw = dict(rule=2, price_blocks=64)
    with e.McfEngine(n, t[:m], h[:m], c[:m], cp[:m], supply, **kw) as a, e.McfEngine(n, t, h, c, cp, supply, **kw) as b:
        rep = a.add_arcs(t[m:], h[m:], c[m:], cp[m:])
        assert rep["m"] == m + k and rep["bigm_grew"] == 0
        chunks = -(-m // 1024)
        assert (chunks - k) * 1024 - 1024 <= rep["shifted_only"] <= m   # at most k chunks receive a new arc
        _assert_same_introspection(_introspect(a), _introspect(b))
        cert = a.certify()
        assert cert["rc_mismatch_count"] == 0 and cert["rc_compared"] == m + k and cert["tree_shape_count"] == 0
        a.solve(max_pivots=300); b.solve(max_pivots=300)
        ra, rb = a.result(), b.result()
        assert ra.stats["pivots"] == rb.stats["pivots"] == 300 and np.array_equal(ra.flow, rb.flow) and np.array_equal(ra.potential, rb.potential)


# ------------------------------------------------------------------ the shim
PLANT_NODES = [{"id": "plant", "supply": 100.0}, {"id": "dist_center", "supply": 0.0}, {"id": "market", "supply": -100.0}]
PLANT_ARCS = [{"tail": "plant", "head": "dist_center", "capacity": 100.0, "cost": 5.0},
              {"tail": "dist_center", "head": "market", "capacity": 100.0, "cost": 4.0}]
DIRECT = {"tail": "plant", "head": "market", "capacity": 60.0, "cost": 8.0}


def test_shim_scenario_4_topology_change(gpu_engine_module):
    """examples/incremental_resolving_example.py, scenario 4, in its own numbers: one solver, solve, add the direct route, solve."""
    import network_flow_solver_amd as nfs
    from network_flow_solver_amd.exceptions import InvalidProblemError

    solver = nfs.NetworkSimplex(nfs.build_problem(PLANT_NODES, PLANT_ARCS, True, 1e-6))
    first = solver.solve()
    assert first.status == "optimal" and first.objective == 900.0
    rep = solver.add_arcs([DIRECT])
    assert rep["path"] == 0 and rep["first_index"] == 2 and rep["count"] == 1 and rep["eligible"] == 1
    second = solver.solve()
    assert second.status == "optimal" and second.objective == 840.0
    assert second.flows[("plant", "market")] == 60.0 and second.flows[("plant", "dist_center")] == 40.0
    cold = nfs.NetworkSimplex(nfs.build_problem(PLANT_NODES, PLANT_ARCS + [DIRECT], True, 1e-6)).solve()
    assert cold.objective == 840.0 and second.iterations < cold.iterations
    assert solver.certify().proves_status
    assert len(solver.problem.arcs) == 3 and solver.problem.arcs[2].capacity == 60.0
    solver.update_costs({("plant", "market"): 7.0})                      # keyed updates see the new arc
    assert solver.solve().objective == 60 * 7.0 + 40 * 9.0
    solver.close_arcs([("plant", "market")])
    back = solver.solve()
    assert back.status == "optimal" and back.objective == 900.0
    # a lower bound on a new arc: its supply shift goes through in the same call
    rep = solver.add_arcs([{"tail": "plant", "head": "market", "capacity": 30.0, "cost": 20.0, "lower": 10.0}])
    forced = solver.solve()
    assert forced.objective == 90 * 9.0 + 10 * 20.0 and forced.flows[("plant", "market")] == 10.0
    with pytest.raises(InvalidProblemError, match="has the lower bound 10 and cannot be closed"):
        solver.close_arcs([("plant", "market")])
    # an edge of an undirected problem cannot be closed either: its shift -C is fixed in the resident instance
    und = nfs.NetworkSimplex(nfs.build_problem(PLANT_NODES, PLANT_ARCS, False, 1e-6))
    assert und.solve().objective == 900.0
    und.add_arcs([{"tail": "plant", "head": "market", "capacity": 60.0, "cost": 8.0}])
    assert und.solve().objective == 840.0
    with pytest.raises(InvalidProblemError, match="is an undirected edge .* and cannot be closed"):
        und.close_arcs([("plant", "market")])


def test_shim_new_handle_when_the_lds_path_cannot_grow(gpu_engine_module):
    import network_flow_solver_amd as nfs
    from network_flow_solver_amd.data import SoAProblem

    inst = _inst("lds")
    solver = nfs.NetworkSimplex(SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply))
    solver.solve()
    assert solver.stats["pricing_mode"] == 2
    t, h, c, cp = _extra(inst, 9000, seed=3)
    rep = solver.add_arcs((t, h, c, cp))
    assert rep["path"] == 2 and rep["first_index"] == inst.m and rep["count"] == 9000
    res = solver.solve()
    ext = _extended(inst, t, h, c, cp)
    assert res.status == "optimal" and res.objective == float(int(round(oracle.solve_soa(ext, "dantzig")["objective"])))
    assert solver.problem.m == ext.m and solver.certify().proves_status
    solver.close_arcs(np.arange(inst.m, ext.m))
    assert solver.solve().objective == float(int(round(oracle.solve_soa(inst, "dantzig")["objective"])))
