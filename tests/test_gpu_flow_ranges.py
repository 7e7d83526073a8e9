"""mcf_supply_ranges / mcf_capacity_ranges on the device, against ``flow_ranges_yardsticks.walk`` (``test_flow_ranges_cpu.py``
holds it against the interval yardstick and against the host restatement of the same logic).

  a. planted trees (``mcf_set_basis``, no pivot) on the dense array and the blocked list: the boundary sweep of
     ``planted_trees``, the depths round the powers of two (the number of table levels), an index list, two calls;
  b. past the caps: more nodes than lanes of a node pass, more arcs than lanes of the arc pass, more pairs than lanes of the
     pair pass;
  c. the contract on solved goldens: an edit below the limit keeps the basis and pivots nothing, at the limit no tree flow is
     out of bounds, one unit past it one is (or an artificial arc turns round); the objective moves by rate * d exactly;
  d. every engine path, Devex, dropped reduced costs, both ranks of a sharded pair; e. read-only; f. errors, the Python layer.

Nothing has a tolerance: the calls are exact integer arithmetic."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import flow_ranges_yardsticks as fy
import network_flow_solver_amd as nfs
import planted_trees as pt
from conftest import load_synthetic
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

pytestmark = pytest.mark.gpu

INF = fy.INF
FIELDS = fy.REPORT + ("big_m",)
# k_frng_arcs has the grid of k_rng_arcs (csrc/mcf_passes_dev.h): at most 2 048 workgroups of 256 lanes, reached from
# 8 * 255 * 2 048 arcs on -- the constants of test_gpu_cost_ranges.py; k_frng_pairs: at most 2 048 workgroups of 256 lanes
ARC_LANE_CAP = 2048 * 256
ARC_GRID_FULL_FROM = 8 * 255 * 2048 + 1
PAIR_LANE_CAP = 2048 * 256


def _engine(e, inst, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, **kw)


def _install(e, pl, **kw):
    """A handle holding the planted basis, its tree, and the state the yardstick reads."""
    eng = _engine(e, pl.inst, **kw)
    if pl.in_tree.any():
        assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
    tree = eng.tree()
    assert np.array_equal(tree["parent"][: pl.n], pl.parent) and np.array_equal(tree["pred_arc"][: pl.n], pl.tree_arc)
    assert np.array_equal(tree["state"], pl.state)
    return eng, tree, fy.planted_state(pl, tree)


def _resident(eng, inst):
    """(state of the yardstick, tree) from what the handle reports: mcf_get_tree and the flows of mcf_get_result."""
    tree = eng.tree()
    return fy.resident_state(inst, tree, eng.result().flow, supply=eng.supply, cap=eng.cap), tree


def _assert_same(got, want, big_m):
    *ga, grep = got
    *wa, wrep = want
    for i, (g, w) in enumerate(zip(ga, wa)):
        assert np.array_equal(g, w), (i, np.flatnonzero(g != w)[:8], g[g != w][:4], w[g != w][:4])
    assert set(grep) == set(FIELDS) | {"device_ms"}
    wrep = dict(wrep, big_m=big_m)
    assert {k: grep[k] for k in FIELDS} == wrep, {k: (grep[k], wrep[k]) for k in FIELDS if grep[k] != wrep[k]}


def _check(eng, st, pi, state, cost, big_m, rng, extra=200):
    """Both calls of the handle against the yardstick; returns the two answers."""
    xs, ys = fy.pair_list(st, rng, extra)
    sup = eng.supply_ranges(xs, ys)
    _assert_same(sup, fy.supply_ranges(st, pi, xs, ys), big_m)
    cap = eng.capacity_ranges()
    _assert_same(cap, fy.capacity_ranges(st, state, cost, pi), big_m)
    return sup, cap


def _check_resident(eng, inst, seed=1, extra=2000):
    st, tree = _resident(eng, inst)
    return _check(eng, st, tree["pi"], tree["state"], eng.cost, pt.big_m(inst, eng.cost), np.random.default_rng(seed), extra)


# ------------------------------------------------------------------ a. planted trees
@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("n,shape,m", [(c[1], c[2], c[4]) for c in pt.sweep_cases()], ids=[f"n{c[1]}-{c[2]}-m{c[4]}" for c in pt.sweep_cases()])
def test_boundary_sweep(gpu_engine_module, n, shape, m, tree_blocks):
    pl = pt.sweep_plant(n, shape, m)
    eng, tree, st = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        sup, _ = _check(eng, st, tree["pi"], pl.state, pl.inst.cost, pt.big_m(pl), np.random.default_rng(n))
        assert (sup[0][sup[0] != INF] > 0).all()                   # planted flows are non-degenerate


@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("d", pt.DEPTHS)
def test_depths_around_powers_of_two(gpu_engine_module, d, tree_blocks):
    pl = pt.cold_plant() if d == 1 else pt.depth_plant(d)
    eng, tree, st = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        sup, cap = _check(eng, st, tree["pi"], pl.state, pl.inst.cost, pt.big_m(pl), np.random.default_rng(d))
        for rep in (sup[4], cap[5]):
            assert rep["max_depth"] == d and rep["levels"] == max(1, d.bit_length())
        if d > 1:                                                  # the deepest node against the top of the path, both ways
            xs, ys = np.array([d - 1, 0], np.int32), np.array([0, d - 1], np.int32)
            _assert_same(eng.supply_ranges(xs, ys), fy.supply_ranges(st, tree["pi"], xs, ys), pt.big_m(pl))


@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
def test_an_index_list_with_duplicates_an_empty_list_and_a_second_call(gpu_engine_module, tree_blocks):
    pl = pt.sweep_plant(2047, "forest", 4097)
    eng, tree, st = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        bigm = pt.big_m(pl)
        full = eng.capacity_ranges()
        want = fy.capacity_ranges(st, pl.state, pl.inst.cost, tree["pi"])
        _assert_same(full, want, bigm)
        rng = np.random.default_rng(12)
        idx = rng.integers(0, pl.m, 300)
        idx[10:20] = idx[0]                                        # duplicates, next to each other and apart
        idx[-1] = idx[5]
        part = eng.capacity_ranges(idx)
        _assert_same(part, (*(a[idx] for a in want[:5]), fy.list_report(want[5], want[0][idx], want[1][idx])), bigm)
        none = eng.capacity_ranges(np.zeros(0, np.int64))         # an empty list: an empty answer
        assert all(len(a) == 0 for a in none[:5]) and none[5]["inf_count"] == none[5]["zero_count"] == 0
        _assert_same(eng.capacity_ranges(), want, bigm)            # the second full call: identical arrays
        xs, ys = fy.pair_list(st, rng)
        first = eng.supply_ranges(xs, ys)
        _assert_same(first, fy.supply_ranges(st, tree["pi"], xs, ys), bigm)
        assert (first[3] > 0).any() and (first[3] == 0).any()      # a forest: some paths cross the root
        _assert_same(eng.supply_ranges(xs, ys), first[:4] + ({k: first[4][k] for k in fy.REPORT},), bigm)
        empty = eng.supply_ranges(np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert all(len(a) == 0 for a in empty[:4]) and empty[4]["inf_count"] == 0


# ------------------------------------------------------------------ b. past the caps
def test_past_the_lane_cap_of_the_node_passes(gpu_engine_module):
    pl = pt.large_plant("random")
    assert pl.n + 1 > pt.LANE_CAP and (pl.n + 1) % 256 != 0 and pl.m > ARC_LANE_CAP
    eng, tree, st = _install(gpu_engine_module, pl)
    with eng:
        sup, cap = _check(eng, st, tree["pi"], pl.state, pl.inst.cost, pt.big_m(pl), np.random.default_rng(5), extra=20000)
        assert cap[5]["basic_artificial"] == 65                    # the shape's top and the 64 single nodes
        far = np.arange(pl.n - 64, pl.n, dtype=np.int32)           # nodes past the lane cap that hang on the root by themselves
        _assert_same(eng.supply_ranges(far, far[::-1]), fy.supply_ranges(st, tree["pi"], far, far[::-1]), pt.big_m(pl))


@pytest.mark.parametrize("m", (ARC_LANE_CAP + 257, ARC_GRID_FULL_FROM), ids=["above-one-grid", "grid-full"])
def test_past_the_lane_cap_of_the_arc_pass(gpu_engine_module, m):
    pl = pt.plant("binary", 63, m, seed=41)
    assert pl.m > ARC_LANE_CAP and pl.m % 256 != 0
    eng, tree, st = _install(gpu_engine_module, pl)
    with eng:
        _assert_same(eng.capacity_ranges(), fy.capacity_ranges(st, pl.state, pl.inst.cost, tree["pi"]), pt.big_m(pl))


def test_past_the_lane_cap_of_the_pair_pass(gpu_engine_module):
    pl = pt.sweep_plant(4096, "random", 4097)
    eng, tree, st = _install(gpu_engine_module, pl)
    with eng:
        rng = np.random.default_rng(9)
        k = PAIR_LANE_CAP + 257
        xs, ys = rng.integers(0, pl.n, k).astype(np.int32), rng.integers(0, pl.n, k).astype(np.int32)
        _assert_same(eng.supply_ranges(xs, ys), fy.supply_ranges(st, tree["pi"], xs, ys), pt.big_m(pl))


# ------------------------------------------------------------------ c. the contract, on solved goldens
CONTRACT_GOLDENS = ("netgen_8_10a_syn.npz", "gridgen_8_10a_syn.npz", "goto_8_10a_syn.npz")


def _golden(file):
    return next(inst for s, inst in load_synthetic() if s["file"] == file)


def _solved(e, inst):
    eng = _engine(e, inst, rule=e.RULE_DANTZIG)
    eng.solve()
    assert eng.result().status == "optimal"
    return eng


def _objective(eng):
    cert = eng.certify()
    return cert["primal"] + cert["bigm_term"]


def _try_edit(e, inst, edit, d, limit, limit_arc, rate):
    """One edit of size d on a fresh solved handle (the solve is deterministic: the same basis every time), the contract
    asserted.  edit(eng, d) applies it and returns the report of update_rhs; rate is per unit of d."""
    m = inst.m
    with _solved(e, inst) as eng:
        old, pivots = _objective(eng), eng.stats()["pivots"]
        rep = edit(eng, d)
        note = (d, limit, limit_arc, rep)
        if d < limit:
            assert rep["path"] == 0 and rep["tree_violations"] == 0 and rep["art_flips"] == 0 and rep["wrong_way"] == 0, note
            assert _objective(eng) == old + rate * d, note
            eng.solve()
            assert eng.stats()["pivots"] == pivots and eng.stats()["status"] == "optimal", note
            assert eng.certify()["verdict"] == "optimal" and _objective(eng) == old + rate * d, note
        elif d == limit:
            assert rep["tree_violations"] == 0 and rep["path"] in (0, 1), note
            eng.solve()
            assert eng.result().status == "optimal" and _objective(eng) == old + rate * d, note
        else:
            assert (rep["tree_violations"] >= 1) if limit_arc < m else (rep["art_flips"] >= 1), note


@pytest.mark.parametrize("file", CONTRACT_GOLDENS)
def test_the_contract_of_capacity_ranges(gpu_engine_module, file):
    e = gpu_engine_module
    inst = _golden(file)
    with _solved(e, inst) as eng:
        (_, (down, up, down_arc, up_arc, rate, rep)) = _check_resident(eng, inst)
        state = eng.tree()["state"]
    assert rep["at_capacity"] == int((state == -1).sum()) and (down >= 0).all() and (up >= 0).all()
    ups = np.flatnonzero((state == -1) & (up >= 1) & (up < INF))
    downs = np.flatnonzero((down >= 2) & (down < INF))
    assert len(ups) >= 8 and len(downs) >= 8, (len(ups), len(downs))   # fewer: the test fails rather than shrinks
    rng = np.random.default_rng(2026)
    # most arcs sit at their lower bound and may fall to 0, where nothing lies one unit past the limit: of the 8, three are
    # basic with flow, three sit at capacity and are limited by a tree arc, two are limited by their own capacity
    inner = (down >= 2) & (down < inst.cap)
    kinds = [np.flatnonzero(inner & (state == 0)), np.flatnonzero(inner & (state == -1)), np.flatnonzero((down >= 2) & (down == inst.cap))]
    assert len(kinds[0]) >= 3 and len(kinds[1]) >= 3 and len(kinds[2]) >= 2, [len(k) for k in kinds]
    downs = np.concatenate([rng.choice(k, c, replace=False) for k, c in zip(kinds, (3, 3, 2))])
    past = 0
    for a in rng.choice(ups, 8, replace=False).tolist():          # more capacity on an arc that sits at its capacity
        cap = int(inst.cap[a])
        for d in (int(up[a]) - 1, int(up[a]), int(up[a]) + 1):
            if d > 0:
                _try_edit(e, inst, lambda eng, d: eng.update_rhs(arcs=[a], caps=[cap + d]), d, int(up[a]), int(up_arc[a]), int(rate[a]))
    for a in downs.tolist():                                       # less capacity: the objective moves by rate * (-d)
        cap = int(inst.cap[a])
        for d in (int(down[a]) - 1, int(down[a]), int(down[a]) + 1):
            if d > cap:                                            # (a capacity cannot fall below 0: where down == cap nothing lies past it)
                assert down[a] == cap and down_arc[a] in (a, -1)
                continue
            past += d > down[a]
            _try_edit(e, inst, lambda eng, d: eng.update_rhs(arcs=[a], caps=[cap - d]), d, int(down[a]), int(down_arc[a]), -int(rate[a]))
    assert past == 6                                               # one unit past the limit was tried on the falling side too


@pytest.mark.parametrize("file", CONTRACT_GOLDENS)
def test_the_contract_of_supply_ranges(gpu_engine_module, file):
    e = gpu_engine_module
    inst = _golden(file)
    rng = np.random.default_rng(2027)
    xs, ys = rng.integers(0, inst.n, 4000).astype(np.int32), rng.integers(0, inst.n, 4000).astype(np.int32)
    with _solved(e, inst) as eng:
        st, tree = _resident(eng, inst)
        got = eng.supply_ranges(xs, ys)
        _assert_same(got, fy.supply_ranges(st, tree["pi"], xs, ys), pt.big_m(inst))
    limit, arc, rate, rising, _ = got
    ok = np.flatnonzero((limit >= 2) & (limit < INF) & (rising == 0))
    assert len(ok) >= 8, len(ok)
    for i in ok[:8].tolist():
        x, y = int(xs[i]), int(ys[i])

        def edit(eng, d):
            return eng.update_rhs(nodes=[x, y], supplies=[int(inst.supply[x]) + d, int(inst.supply[y]) - d])
        for d in (int(limit[i]) - 1, int(limit[i]), int(limit[i]) + 1):
            _try_edit(e, inst, edit, d, int(limit[i]), int(arc[i]), int(rate[i]))


def test_a_shift_that_raises_artificial_flow_ends_infeasible(gpu_engine_module):
    """A golden plus a component of its own (two nodes, one arc, no supply): its basis hangs on the root by two artificial arcs,
    and a shift from one component to the other has to cross them."""
    e = gpu_engine_module
    base = _golden("netgen_8_10a_syn.npz")
    n = base.n
    inst = ArcSoA(n + 2, np.append(base.tail, n).astype(np.int32), np.append(base.head, n + 1).astype(np.int32), np.append(base.cost, 1),
                  np.append(base.cap, 5), np.append(base.supply, [0, 0]), base.name + "+island")
    with _solved(e, inst) as eng:
        st, tree = _resident(eng, inst)
        xs, ys = np.array([0, n, 0, n + 1], np.int32), np.array([n, 0, n + 1, 0], np.int32)
        got = eng.supply_ranges(xs, ys)
        _assert_same(got, fy.supply_ranges(st, tree["pi"], xs, ys), pt.big_m(inst))
        assert got[4]["basic_artificial"] >= 2 and (got[3] > 0).any()
        i = int(np.flatnonzero(got[3] > 0)[0])
        x, y = int(xs[i]), int(ys[i])
        eng.update_rhs(nodes=[x, y], supplies=[int(inst.supply[x]) + 1, int(inst.supply[y]) - 1])
        eng.solve()
        assert eng.result().status == "infeasible"


# ------------------------------------------------------------------ d. every engine path
PATHS = {
    "small": (dict(), 0, (200, 1500)),                                             # k_solve_small (LDS)
    "mid": (dict(fused=False, mid_loop=1), 2, (700, 6000)),                        # k_solve_mid
    "graphs": (dict(fused=False, mid_loop=-1, tree_blocks=-1), 0, (1500, 12000)),   # captured graphs of three kernels per pivot
    "blocked": (dict(tree_blocks=2), 2, (1500, 12000)),
    "gather": (dict(fused=False, mid_loop=-1, resident_rc=False), 0, (700, 6000)),  # no resident reduced costs at all (no_rcache)
    "devex": (dict(fused=False, mid_loop=-1), 1, (1500, 12000)),
}


@pytest.mark.parametrize("path", PATHS)
def test_solved_handles_on_every_engine_path(gpu_engine_module, path):
    e = gpu_engine_module
    kw, rule, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=3)
    with _engine(e, inst, rule=rule, **kw) as eng:
        eng.solve()
        assert eng.result().status == "optimal"
        sup, cap = _check_resident(eng, inst)
        assert (sup[0] >= 0).all() and (cap[0] >= 0).all() and (cap[1] >= 0).all()
        assert eng.certify()["verdict"] == "optimal"


def test_a_handle_solved_by_solve_batch(gpu_engine_module):
    e = gpu_engine_module
    insts = [generators.netgen_style(200, 1500, seed=s) for s in (3, 4)]
    engines = [_engine(e, i, rule=2) for i in insts]
    try:
        e.solve_batch(engines)
        for eng, inst in zip(engines, insts):
            assert eng.result().status == "optimal"
            _check_resident(eng, inst)
    finally:
        for eng in engines:
            eng.close()


def test_a_handle_that_dropped_its_reduced_costs(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(3000, 24000, seed=3)
    with _engine(e, inst, rule=2, tree_blocks=4, rc_drop=1) as eng:
        eng.solve()
        res = eng.result()
        assert res.status == "optimal" and res.stats["rc_dropped_at"] > 0
        _check_resident(eng, inst)


def test_both_ranks_of_a_sharded_pair(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(1500, 12000, seed=8)
    with _engine(e, inst, rule=0, fused=False, mid_loop=-1) as eng:
        eng.solve()
        res = eng.result()
    answers = []
    for rank in (0, 1):
        with _engine(e, inst, rule=0, shard=(rank, 2), fused=False, mid_loop=-1) as eng:
            sup, cap = _check_resident(eng, inst)                  # the cold start: every node on its artificial arc
            assert cap[5]["basic_real"] == 0 and cap[5]["basic_artificial"] == inst.n and cap[5]["at_capacity"] == 0
            assert eng.set_basis(res.in_tree, (res.flow == inst.cap) & ~res.in_tree & (inst.cap > 0))
            answers.append(_check_resident(eng, inst))
    for a, b in zip(answers[0][0][:4] + answers[0][1][:5], answers[1][0][:4] + answers[1][1][:5]):
        assert np.array_equal(a, b)
    assert {k: answers[0][1][5][k] for k in FIELDS} == {k: answers[1][1][5][k] for k in FIELDS}


# ------------------------------------------------------------------ e. read-only
@pytest.mark.parametrize("path", ("small", "mid", "graphs", "blocked", "devex"))
def test_the_calls_change_no_later_pivot(gpu_engine_module, path):
    e = gpu_engine_module
    kw, rule, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=5)
    runs = []
    for ranging in (False, True):
        with _engine(e, inst, rule=rule, **kw) as eng:
            eng.solve(150)
            if ranging:
                _check_resident(eng, inst, extra=500)              # mid-solve: artificial arcs carry flow, reported as it is
                eng.capacity_ranges(np.arange(0, inst.m, 7))
            eng.solve(37)
            if ranging:
                eng.supply_ranges(np.arange(inst.n, dtype=np.int32), np.arange(inst.n, dtype=np.int32)[::-1])
                eng.capacity_ranges()
            eng.solve()
            res, tree = eng.result(), eng.tree()
            rc, weights = eng.reduced_costs(), eng.weights()
        stats = {k: res.stats[k] for k in ("pivots", "degenerate", "bound_flips", "cycle_arcs", "subtree_nodes", "arcs_priced")}
        runs.append((res.status, res.objective, stats, rc[1], res.flow, res.potential, tree["order"], tree["parent"], tree["pred_arc"], tree["state"],
                     rc[0], weights))
    a, b = runs
    assert a[:4] == b[:4]
    for x, y in zip(a[4:], b[4:]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ f. errors, the Python layer
def test_bad_arguments_are_refused_and_leave_the_handle_alone(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(200, 1500, seed=3)
    drop = ("arc_pass_ms", "node_pass_ms")
    with _engine(e, inst, rule=0) as eng:
        eng.solve()
        before = {k: v for k, v in eng.certify().items() if k not in drop}
        good = eng.capacity_ranges()
        for bad in ([inst.m], [-1], [0, 5, inst.m + 3]):
            with pytest.raises(e.EngineError) as err:
                eng.capacity_ranges(bad)
            assert err.value.code == -1 and "index" in str(err.value)
        for bad in (([inst.n], [0]), ([0], [inst.n]), ([-1], [0]), ([0, 1], [2, -5]), ([1 << 32], [0]), ([0], [(1 << 32) + 1])):
            with pytest.raises(e.EngineError) as err:
                eng.supply_ranges(*bad)
            assert err.value.code == -1 and "index" in str(err.value)
        lib, h = eng._lib, eng._h
        i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        buf, idx, nodes = np.zeros(inst.m, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int32)
        p64, p32 = (lambda a: a.ctypes.data_as(i64p)), (lambda a: a.ctypes.data_as(i32p))
        assert lib.mcf_capacity_ranges(h, 4, None, p64(buf), p64(buf), None, None, None, None) == -1     # a count without a list
        assert lib.mcf_capacity_ranges(h, -1, p64(idx), p64(buf), p64(buf), None, None, None, None) == -1  # a list with count < 0
        assert lib.mcf_capacity_ranges(None, -1, None, p64(buf), p64(buf), None, None, None, None) == -1
        assert lib.mcf_capacity_ranges(h, 0, None, None, None, None, None, None, None) == 0              # nothing to return: fine
        assert lib.mcf_capacity_ranges(h, -1, None, None, p64(buf), None, None, None, None) == 0         # every output may be NULL
        assert np.array_equal(buf, good[1])
        assert lib.mcf_supply_ranges(h, 4, None, p32(nodes), None, None, None, None, None) == -1
        assert lib.mcf_supply_ranges(h, 4, p32(nodes), None, None, None, None, None, None) == -1
        assert lib.mcf_supply_ranges(h, -1, None, None, None, None, None, None, None) == -1
        assert lib.mcf_supply_ranges(None, 0, None, None, None, None, None, None, None) == -1
        assert lib.mcf_supply_ranges(h, 0, None, None, None, None, None, None, None) == 0
        assert lib.mcf_supply_ranges(h, 4, p32(nodes), p32(nodes), None, None, None, None, None) == 0
        assert {k: v for k, v in eng.certify().items() if k not in drop} == before
        again = eng.capacity_ranges()
        assert all(np.array_equal(x, y) for x, y in zip(again[:5], good[:5]))
    with e.McfEngine(1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64)) as eng:
        *arrays, rep = eng.capacity_ranges()                      # n == 1, m == 0: an empty answer
        assert all(len(a) == 0 for a in arrays) and rep["basic_real"] == rep["at_capacity"] == rep["inf_count"] == 0
        limit, arc, rate, rising, rep = eng.supply_ranges([0], [0])
        assert (limit[0], arc[0], rate[0], rising[0]) == (INF, -1, 0, 0) and rep["inf_count"] == 1


def _object_problem():
    nodes = [dict(id="a", supply=10.5), dict(id="b", supply=0.0), dict(id="c", supply=-4.0), dict(id="d", supply=-6.5)]
    arcs = [dict(tail="a", head="b", capacity=8.0, cost=1.25, lower=1.5), dict(tail="a", head="c", capacity=6.0, cost=4.0, lower=0.0),
            dict(tail="b", head="c", capacity=5.0, cost=1.0, lower=0.0), dict(tail="b", head="d", capacity=9.0, cost=2.5, lower=0.5),
            dict(tail="c", head="d", capacity=None, cost=1.0, lower=0.0), dict(tail="a", head="d", capacity=3.0, cost=9.0, lower=0.0),
            dict(tail="a", head="d", capacity=2.0, cost=9.5, lower=0.0)]                            # parallel to the arc before: the last one answers
    return nodes, arcs


def test_shim_on_an_object_problem_with_lower_bounds_scales_and_parallel_arcs(gpu_engine_module):
    options = nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True)
    nodes, arcs = _object_problem()
    solver = nfs.NetworkSimplex(nfs.build_problem(nodes, arcs, True, 1e-6), options)
    first = solver.solve()
    assert first.status == "optimal"
    f = solver.flat
    assert f.flow_scale > 1 and f.cost_scale > 1                   # halves and quarters: a scaled instance
    ranges = solver.capacity_ranges()
    assert set(ranges) == set(f.keys) and len(ranges) == len(arcs) - 1
    down, up, down_arc, up_arc, rate, _ = solver.engine.capacity_ranges()
    caps = {(a["tail"], a["head"]): a for a in arcs}               # (of parallel arcs the last)
    last = {key: i for i, key in enumerate(f.keys)}
    for key, (lowest, highest, r, arc_down, arc_up) in ranges.items():
        i, arc = last[key], caps[key]
        if arc["capacity"] is None:
            assert (lowest, highest, r, arc_down, arc_up) == (None, None, 0.0, None, None)
            continue
        assert lowest == arc["capacity"] - down[i] / f.flow_scale and lowest >= arc["lower"]       # lower bounds added back
        assert highest is None if up[i] == INF else highest == arc["capacity"] + up[i] / f.flow_scale
        assert r == rate[i] / f.cost_scale and lowest <= arc["capacity"]
        for name, index in ((arc_down, down_arc[i]), (arc_up, up_arc[i])):
            assert name == (None if index < 0 else f.keys[index] if index < len(f.keys) else ("artificial", f.node_ids[index - len(f.keys)]))
    assert solver.capacity_ranges([("a", "d")]) == {("a", "d"): ranges[("a", "d")]}
    with pytest.raises(nfs.InvalidProblemError):
        solver.capacity_ranges([("d", "a")])
    # a capacity moved strictly inside its range re-solves in 0 iterations and moves the objective by rate * change
    tried = 0
    for key, (lowest, highest, r, _, _) in ranges.items():
        cap = caps[key]["capacity"]
        if cap is None:
            continue
        for new in (lowest + 0.5 if lowest + 0.5 < cap else None, cap + 0.5 if highest is None or cap + 0.5 < highest else None):
            if new is None:
                continue
            solver.update_capacities({key: new})
            again = solver.solve()
            assert again.status == "optimal" and again.iterations == 0 and again.objective == first.objective + r * (new - cap), (key, new)
            solver.update_capacities({key: cap})
            assert solver.solve().iterations == 0
            tried += 1
    assert tried >= 4
    pairs = [("a", "d"), ("d", "a"), ("b", "c"), ("a", "a")]
    answers = solver.supply_ranges(pairs)
    assert all(isinstance(x, nfs.SupplyRange) for x in answers) and len(answers) == 4
    assert answers[3] == nfs.SupplyRange(None, 0.0, None, False)
    supplies = {nd["id"]: nd["supply"] for nd in nodes}
    tried = 0
    for (a, b), ans in zip(pairs[:3], answers[:3]):
        assert not ans.creates_artificial_flow and (ans.limit is None or ans.limit >= 0)
        if ans.limit is None or ans.limit > 0.5:
            solver.update_supplies({a: supplies[a] + 0.5, b: supplies[b] - 0.5})
            again = solver.solve()
            assert again.status == "optimal" and again.iterations == 0 and again.objective == first.objective + ans.rate * 0.5, (a, b)
            solver.update_supplies({a: supplies[a], b: supplies[b]})
            assert solver.solve().iterations == 0
            tried += 1
    assert tried >= 1
    with pytest.raises(nfs.InvalidProblemError):
        solver.supply_ranges([("a", "zz")])


def test_shim_on_an_soa_problem(gpu_engine_module):
    from network_flow_solver_amd.data import SoAProblem

    inst = generators.netgen_style(300, 2400, seed=8)
    lower = np.zeros(inst.m, np.int64)
    lower[::7] = 1
    cap = np.where(inst.cap >= 0, inst.cap + lower, inst.cap)
    solver = nfs.NetworkSimplex(SoAProblem(inst.n, inst.tail, inst.head, inst.cost, cap, inst.supply, lower),
                                nfs.SolverOptions(pricing_strategy="candidate_list", explicit_pricing_strategy=True))
    assert solver.solve().status == "optimal"
    lowest, highest, rate, arc_down, arc_up = solver.capacity_ranges()
    down, up, da, ua, r, _ = solver.engine.capacity_ranges()
    assert lowest.dtype == highest.dtype == np.int64
    assert np.array_equal(lowest, np.where(down == INF, -1, cap - np.where(down == INF, 0, down)))
    assert np.array_equal(highest, np.where(up == INF, INF, cap + np.where(up == INF, 0, up)))
    assert np.array_equal(rate, r) and np.array_equal(arc_down, da) and np.array_equal(arc_up, ua)
    capped = cap >= 0
    assert (lowest[capped] >= lower[capped]).all() and (lowest[capped] <= cap[capped]).all() and (highest >= cap).all()
    idx = np.array([5, 5, 17, 0])
    part = solver.capacity_ranges(idx)
    assert all(np.array_equal(p, w[idx]) for p, w in zip(part, (lowest, highest, rate, arc_down, arc_up)))
    xs, ys = np.arange(0, 300, 7), np.arange(0, 300, 7)[::-1].copy()
    limit, srate, arc, infeasible = solver.supply_ranges((xs, ys))
    want = solver.engine.supply_ranges(xs, ys)
    assert np.array_equal(limit, want[0]) and np.array_equal(srate, want[2]) and np.array_equal(arc, want[1])
    assert np.array_equal(infeasible, want[3] > 0) and infeasible.dtype == bool
    with pytest.raises(nfs.InvalidProblemError):
        solver.supply_ranges(([0], [300]))
