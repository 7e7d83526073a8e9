"""mcf_supply_ranges / mcf_capacity_ranges without a device: the ABI surface, and their logic (csrc/mcf_core.h: mcf_frng_*)
through its host restatement (csrc/mcf_flow_ranges_host.cpp) on planted trees and on end states of the CPU emulation, held
against the yardsticks of ``flow_ranges_yardsticks`` -- which are held against each other first.  Every comparison is exact."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import flow_ranges_yardsticks as fy
import oracle
import planted_trees as pt
import ranges_yardsticks as ry
from conftest import load_synthetic
from network_flow_solver_amd import engine

INF = fy.INF


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_flow_ranges_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    lib.mcf_supply_ranges_host.argtypes = [i32, i64, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int, i64, i32p, i32p, i64p, i64p, i64p, i32p, i64p]
    lib.mcf_capacity_ranges_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i8p, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int,
                                             i64p, i64p, i64p, i64p, i64p, i64p]
    lib.mcf_supply_ranges_host.restype = lib.mcf_capacity_ranges_host.restype = ctypes.c_int
    return lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _tree_args(st):
    """The node arrays the restatement reads: the orientation, flow and capacity of every node's tree arc."""
    n, m = st.n, st.m
    a = np.asarray(st.pred_arc, np.int64)[:n]
    art = a >= m
    ar = np.where(art, 0, a)
    tail, cap, flow = (np.append(np.asarray(x, np.int64), 0) for x in (st.tail, st.cap, st.flow))
    up = np.append(np.where(art, st.art_up, tail[ar] == np.arange(n)), 0).astype(np.int8)
    tflow = np.append(np.where(art, st.art_flow, flow[ar]), 0).astype(np.int64)
    tcap = np.append(np.where(art, -1, cap[ar]), 0).astype(np.int64)
    arr = lambda x, d: np.ascontiguousarray(x, d)                                                 # noqa: E731
    return (arr(st.parent, np.int32), arr(st.pred_arc, np.int32), up, arr(st.depth, np.int32), tflow, tcap)


def supply_host(lib, st, pi, xs, ys, order=1):
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    parent, pred, up, depth, tflow, tcap = _tree_args(st)
    xs, ys, pi = np.ascontiguousarray(xs, np.int32), np.ascontiguousarray(ys, np.int32), np.ascontiguousarray(pi, np.int64)
    k = len(xs)
    limit, arc, rate = (np.full(max(k, 1), -7, np.int64) for _ in range(3))
    rising, rep = np.full(max(k, 1), -7, np.int32), np.zeros(10, np.int64)
    rc = lib.mcf_supply_ranges_host(st.n, st.m, _p(parent, i32), _p(pred, i32), _p(up, i8), _p(depth, i32), _p(tflow, i64), _p(tcap, i64), _p(pi, i64),
                                    order, k, _p(xs, i32), _p(ys, i32), _p(limit, i64), _p(arc, i64), _p(rate, i64), _p(rising, i32), _p(rep, i64))
    assert rc == 0
    return limit[:k], arc[:k], rate[:k], rising[:k], dict(zip(fy.REPORT, (int(x) for x in rep)))


def capacity_host(lib, st, state, cost, pi, order=1):
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    parent, pred, up, depth, tflow, tcap = _tree_args(st)
    arr = lambda x, d: np.ascontiguousarray(x, d)                                                 # noqa: E731
    m = st.m
    outs = [np.full(max(m, 1), -7, np.int64) for _ in range(5)]
    rep = np.zeros(10, np.int64)
    rc = lib.mcf_capacity_ranges_host(st.n, m, _p(arr(st.tail, np.int32), i32), _p(arr(st.head, np.int32), i32), _p(arr(cost, np.int64), i64),
                                      _p(arr(st.cap, np.int64), i64), _p(arr(st.flow, np.int64), i64), _p(arr(state, np.int8), i8),
                                      _p(parent, i32), _p(pred, i32), _p(up, i8), _p(depth, i32), _p(tflow, i64), _p(tcap, i64), _p(arr(pi, np.int64), i64),
                                      order, *(_p(o, i64) for o in outs), _p(rep, i64))
    assert rc == 0
    return (*(o[:m] for o in outs), dict(zip(fy.REPORT, (int(x) for x in rep))))


def _same(got, want):
    *ga, grep = got
    *wa, wrep = want
    for i, (g, w) in enumerate(zip(ga, wa)):
        assert np.array_equal(g, w), (i, np.flatnonzero(g != w)[:8])
    assert grep == wrep, {k: (grep[k], wrep[k]) for k in wrep if grep.get(k) != wrep[k]}


def _planted(pl):
    tree = ry.planted_tree(pl)
    pi = pt.potentials(pl, tree, pl.inst.cost, pt.big_m(pl))
    return fy.planted_state(pl, tree), pi


def _check_planted(host, pl, seed=0, intervals=24):
    st, pi = _planted(pl)
    xs, ys = fy.pair_list(st, np.random.default_rng([77, seed, pl.n]))
    want = fy.supply_ranges(st, pi, xs, ys)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, want)
    if pl.m:
        _same(capacity_host(host, st, pl.state, pl.inst.cost, pi), fy.capacity_ranges(st, pl.state, pl.inst.cost, pi))
    same = xs == ys
    assert (got[0][same] == INF).all() and (got[1][same] == -1).all() and (got[2][same] == 0).all()
    res = st.residuals()
    for i in range(min(intervals, len(xs))):                     # the second yardstick holds the first to account
        one = fy.by_intervals(st, int(xs[i]), int(ys[i]), res)
        assert one == fy.walk_one(st, int(xs[i]), int(ys[i]), res) == (int(want[0][i]), int(want[1][i]), int(want[3][i])), (i, xs[i], ys[i])
    return st, pi, got


# ------------------------------------------------------------------ the ABI surface
def test_library_exports_the_entry_points_and_refuses_a_null_handle():
    lib = engine.load_library()
    for name in ("mcf_supply_ranges", "mcf_capacity_ranges"):
        assert name in engine.ABI_SYMBOLS and name in ge.declared_symbols()
    assert lib.mcf_abi_version() == 3 == engine.ABI_VERSION
    rep = engine.McfFlowRangesReport()
    assert ctypes.sizeof(rep) == 9 * 8 + 8
    assert [name for name, _ in rep._fields_] == ["basic_real", "basic_artificial", "at_capacity", "max_depth", "levels", "inf_count", "zero_count",
                                                  "art_rising_count", "big_m", "device_ms"]
    assert lib.mcf_supply_ranges(None, 0, None, None, None, None, None, None, ctypes.byref(rep)) == -1
    assert lib.mcf_capacity_ranges(None, -1, None, None, None, None, None, None, ctypes.byref(rep)) == -1


# ------------------------------------------------------------------ the yardsticks against each other
@pytest.mark.parametrize("shape", pt.SHAPES)
def test_walk_equals_the_interval_yardstick_on_small_trees(host, shape):
    """All 1 600 pairs of a 40-node tree: the two yardsticks hold each other to account (test infrastructure against test
    infrastructure), and the host restatement answers every pair as they do."""
    pl = pt.plant(shape, 40, m=120, seed=5)
    st, pi = _planted(pl)
    res = st.residuals()
    xs, ys = np.divmod(np.arange(40 * 40), 40)
    limit, arc, rising = fy.walk(st, xs, ys)
    _same(supply_host(host, st, pi, xs, ys), fy.supply_ranges(st, pi, xs, ys))
    for i in range(0, 1600, 3):
        want = fy.by_intervals(st, int(xs[i]), int(ys[i]), res)
        assert want == fy.walk_one(st, int(xs[i]), int(ys[i]), res) == (int(limit[i]), int(arc[i]), int(rising[i])), (xs[i], ys[i])
    assert (limit[xs != ys] > 0).all()                             # planted flows are non-degenerate


# ------------------------------------------------------------------ shapes and sizes
@pytest.mark.parametrize("n,shape,m", [(c[1], c[2], c[4]) for c in pt.sweep_cases()], ids=[f"n{c[1]}-{c[2]}-m{c[4]}" for c in pt.sweep_cases()])
def test_host_restatement_on_the_boundary_sweep(host, n, shape, m):
    pl = pt.sweep_plant(n, shape, m)
    st, _, got = _check_planted(host, pl, intervals=12)
    assert (got[0][got[0] != INF] > 0).all()
    if shape == "forest" and n >= 63:                              # paths across the root: artificial arcs in both orientations
        assert (pl.art > 0).any() and (pl.art < 0).any() and (got[3] > 0).any()


@pytest.mark.parametrize("d", pt.DEPTHS)
def test_host_restatement_across_the_levels_of_the_tables(host, d):
    """Greatest depths 1, 2^k, 2^k +- 1: K = bit_length(d) changes at 1 -> 2, 3 -> 4, 31 -> 32, 1023 -> 1024."""
    pl = pt.cold_plant() if d == 1 else pt.depth_plant(d)
    st, pi, got = _check_planted(host, pl, seed=d, intervals=8)
    assert got[4]["max_depth"] == d and got[4]["levels"] == max(1, d.bit_length())
    if d > 1:                                                      # the deepest node against the top of the path, both ways
        xs, ys = np.array([d - 1, 0], np.int32), np.array([0, d - 1], np.int32)
        _same(supply_host(host, st, pi, xs, ys), fy.supply_ranges(st, pi, xs, ys))


@pytest.mark.parametrize("shape", ("random", "path", "forest"))
def test_the_order_of_the_level_build_changes_nothing(host, shape):
    pl = pt.plant(shape, 257, m=700, seed=23)
    st, pi = _planted(pl)
    xs, ys = fy.pair_list(st, np.random.default_rng(3))
    _same(supply_host(host, st, pi, xs, ys, order=0), supply_host(host, st, pi, xs, ys, order=1))
    _same(capacity_host(host, st, pl.state, pl.inst.cost, pi, order=0), capacity_host(host, st, pl.state, pl.inst.cost, pi, order=1))


# ------------------------------------------------------------------ hand-made degenerate cases
def _hand(parent, arcs, flows, caps, in_tree, art=None):
    """A tree state of one's own: arcs (tail, head) in the caller's order, parent[v] (-1: hangs on the root)."""
    n, m = len(parent), len(arcs)
    tail, head = (np.array(x, np.int32) for x in zip(*arcs))
    par = np.array([n if p < 0 else p for p in parent] + [-1], np.int32)
    depth = np.zeros(n + 1, np.int32)
    for v in range(n):
        depth[v] = depth[par[v]] + 1                               # parent[v] < v
    pred = np.full(n + 1, -1, np.int32)
    for v in range(n):
        pred[v] = m + v
    for a in np.flatnonzero(in_tree):
        t, h = int(tail[a]), int(head[a])
        pred[t if par[t] == h else h] = a
    art = np.zeros(n, np.int64) if art is None else np.array(art, np.int64)
    st = fy.TreeState(n, m, tail, head, np.array(caps, np.int64), np.array(flows, np.int64), par, depth, pred, np.abs(art), art >= 0)
    size = np.ones(n + 1, np.int64)
    for v in range(n - 1, -1, -1):
        size[par[v]] += size[v]
    pos, nxt = np.zeros(n + 1, np.int64), np.ones(n + 1, np.int64)
    for v in range(n):
        pos[v] = nxt[par[v]]
        nxt[par[v]] += size[v]
        nxt[v] = pos[v] + 1
    st.pos, st.size = pos, size
    return st


def test_a_tree_arc_on_a_bound_gives_limit_zero_with_that_arc(host):
    # path 0 - 1 - 2 - 3 below the root; arc 0: 1 -> 0 at flow 0, arc 1: 2 -> 1 at flow == cap, arc 2: 3 -> 2 strictly inside
    st = _hand([-1, 0, 1, 2], [(1, 0), (2, 1), (3, 2)], [0, 9, 4], [7, 9, 10], np.ones(3, bool))
    pi = np.zeros(5, np.int64)
    xs, ys = np.array([3, 0, 3, 2, 1, 0], np.int32), np.array([0, 3, 2, 3, 0, 1], np.int32)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, fy.supply_ranges(st, pi, xs, ys))
    # upwards the full arc 1 stops the push (arc 2 has room 6 before it), downwards the empty arc 0 does, first from the top
    assert got[0].tolist() == [0, 0, 6, 4, 7, 0] and got[1].tolist() == [1, 0, 2, 2, 0, 0]
    assert got[4]["zero_count"] == 3 and got[4]["inf_count"] == 0


def test_ties_on_opposite_sides_of_the_join_go_to_the_x_side_and_to_the_first_arc_in_push_order(host):
    # two chains below node 0: 0 - 1 - 2 and 0 - 3 - 4, every tree arc child -> parent
    arcs = [(1, 0), (2, 1), (3, 0), (4, 3)]
    st = _hand([-1, 0, 1, 0, 3], arcs, [5, 5, 5, 5], [10, 10, 10, 10], np.ones(4, bool))
    pi = np.zeros(6, np.int64)
    xs, ys = np.array([2, 4], np.int32), np.array([4, 2], np.int32)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, fy.supply_ranges(st, pi, xs, ys))
    # every residual is 5: the first arc in push order is the tree arc of x itself
    assert got[0].tolist() == [5, 5] and got[1].tolist() == [1, 3]
    # downward ties alone: x == the join; the first arc from the top is that of node 1 / node 3
    xs, ys = np.array([0, 0], np.int32), np.array([2, 4], np.int32)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, fy.supply_ranges(st, pi, xs, ys))
    assert got[1].tolist() == [0, 2]
    for x, y in ((2, 4), (0, 2), (4, 1)):
        assert fy.by_intervals(st, x, y) == fy.walk_one(st, x, y)


def test_a_capacity_smaller_than_the_push_limits_its_own_fall(host):
    # tree 0 - 1 - 2 (arcs 0, 1 child -> parent, wide); arc 2: 2 -> 0 non-basic at capacity 3; arc 3: 0 -> 2 at capacity 50
    arcs = [(1, 0), (2, 1), (2, 0), (0, 2), (0, 1), (1, 2)]
    st = _hand([-1, 0, 1], arcs, [20, 20, 3, 50, 0, 0], [100, 100, 3, 50, 8, -1], np.array([1, 1, 0, 0, 0, 0], bool))
    state = np.array([0, 0, -1, -1, 1, 1], np.int8)
    cost, pi = np.array([1, 2, 3, 4, 5, 6], np.int64), np.array([0, -1, -3, 0], np.int64)
    got = capacity_host(host, st, state, cost, pi)
    _same(got, fy.capacity_ranges(st, state, cost, pi))
    down, up, down_arc, up_arc, rate, rep = got
    assert (down[2], down_arc[2], up[2], up_arc[2]) == (3, 2, 20, 0)       # push(2 -> 0) = 80 > cap 3: the arc itself; back down 0 -> 2: flow 20, first from the top
    assert (down[3], down_arc[3], up[3], up_arc[3]) == (20, 0, 80, 1)      # push(0 -> 2) = 20 < cap 50: the tree arc
    assert rate.tolist() == [0, 0, 3 - 3 - 0, 4 + 0 + 3, 0, 0]
    assert (down[0], down_arc[0], up[0], up_arc[0]) == (80, 0, INF, -1) and (down[4], down_arc[4], up[4]) == (8, -1, INF)
    assert (down[5], up[5], down_arc[5], up_arc[5]) == (INF, INF, -1, -1) and rep["at_capacity"] == 2


def test_artificial_arcs_in_both_orientations(host):
    # two single nodes on the root: node 0 sends 5 to the root, node 1 takes 5 from it
    st = _hand([-1, -1], [(0, 1)], [0], [4], np.zeros(1, bool), art=[5, -5])
    pi = np.array([-30, 30, 0], np.int64)
    xs, ys = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, fy.supply_ranges(st, pi, xs, ys))
    # 0 -> 1 raises both artificial flows and nothing limits it; 1 -> 0 lowers both: 5, and the first arc is that of node 1
    assert got[0].tolist() == [INF, 5] and got[1].tolist() == [-1, 1 + 1] and got[3].tolist() == [2, 0] and got[2].tolist() == [60, -60]
    assert got[4]["art_rising_count"] == 1 and got[4]["basic_artificial"] == 2


# ------------------------------------------------------------------ end states of the CPU emulation
CONTRACT_GOLDENS = ("netgen_8_10a_syn.npz", "gridgen_8_10a_syn.npz", "goto_8_10a_syn.npz")


def _emulated(file):
    inst = next(inst for s, inst in load_synthetic() if s["file"] == file)
    r = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0)
    assert r["status"] == "optimal"
    in_tree = r["in_tree"].astype(bool)
    capped = (inst.cap >= 0) & (inst.cap < fy.MCF_INF)
    state = np.where(in_tree, 0, np.where((r["flow"] == inst.cap) & capped & (inst.cap > 0), -1, 1)).astype(np.int8)
    tree = {k: r[k] for k in ("parent", "pred_arc", "depth", "pos", "size")}
    tree["pi"] = np.append(r["potential"], 0)
    return inst, state, tree, fy.resident_state(inst, tree, r["flow"])


def contract_picks(inst, state, st, pi, rng):
    """What tests/test_gpu_flow_ranges.py tries on a solved golden: at-capacity arcs with 1 <= up < INF, arcs with down >= 2,
    supply pairs with 2 <= limit < INF that raise no artificial flow."""
    down, up, _, _, _, _ = fy.capacity_ranges(st, state, inst.cost, pi)
    ups = np.flatnonzero((state == -1) & (up >= 1) & (up < INF))
    downs = np.flatnonzero((down >= 2) & (down < INF))
    xs, ys = rng.integers(0, inst.n, 4000), rng.integers(0, inst.n, 4000)
    limit, _, _, rising, _ = fy.supply_ranges(st, pi, xs, ys)
    ok = np.flatnonzero((limit >= 2) & (limit < INF) & (rising == 0))
    return ups, downs, xs[ok], ys[ok]


@pytest.mark.parametrize("file", ("netgen_8_08a_syn.npz", "gridgen_8_08a_syn.npz") + CONTRACT_GOLDENS)
def test_end_states_of_the_emulation(host, file):
    inst, state, tree, st = _emulated(file)
    pi = tree["pi"]
    xs, ys = fy.pair_list(st, np.random.default_rng(8), extra=2000)
    got = supply_host(host, st, pi, xs, ys)
    _same(got, fy.supply_ranges(st, pi, xs, ys))
    assert (got[0] >= 0).all()                                     # a feasible basis: no residual is negative
    _same(capacity_host(host, st, state, inst.cost, pi), fy.capacity_ranges(st, state, inst.cost, pi))
    res = st.residuals()
    for i in range(0, len(xs), 97):
        assert fy.by_intervals(st, int(xs[i]), int(ys[i]), res) == (int(got[0][i]), int(got[1][i]), int(got[3][i]))
    if file in CONTRACT_GOLDENS:                                   # the device contract test needs 8 of each kind
        ups, downs, px, _ = contract_picks(inst, state, st, pi, np.random.default_rng(2026))
        assert len(ups) >= 8 and len(downs) >= 8 and len(px) >= 8, (len(ups), len(downs), len(px))
        down = fy.capacity_ranges(st, state, inst.cost, pi)[0]
        inner = (down >= 2) & (down < inst.cap)                    # ... and of the falling capacities three of each kind that has a "one unit past"
        assert int((inner & (state == 0)).sum()) >= 3 and int((inner & (state == -1)).sum()) >= 3 and int(((down >= 2) & (down == inst.cap)).sum()) >= 2
