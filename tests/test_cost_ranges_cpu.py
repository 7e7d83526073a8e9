"""mcf_cost_ranges without a device: the ABI surface, and its per-arc / per-node logic (csrc/mcf_core.h: mcf_rng_*) through its
host restatement (csrc/mcf_ranges_host.cpp) on planted trees, held against the two yardsticks of ``ranges_yardsticks``.
Planted bases are not optimal -- the reduced costs of the non-tree arcs are whatever the random costs give -- so every case
is also a test of the signed semantics: negative slacks come through as they are.  Every comparison is exact."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle
import planted_trees as pt
import ranges_yardsticks as ry
from conftest import load_synthetic
from network_flow_solver_amd import engine, generators

REPORT = ("basic_real", "basic_artificial", "eligible", "max_depth", "levels", "inf_down", "inf_up")


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_ranges_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    lib.mcf_cost_ranges_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i8p, i32p, i32p, i32p, i64p, ctypes.c_int64,
                                         i64p, i64p, i64p]
    lib.mcf_cost_ranges_host.restype = ctypes.c_int
    return lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def ranges_host(lib, pl, tree, pi, chunk=64):
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    arr = lambda a, d: np.ascontiguousarray(a, d)                                                 # noqa: E731
    inst = pl.inst
    down, up, rep = np.full(max(pl.m, 1), -7, np.int64), np.full(max(pl.m, 1), -7, np.int64), np.zeros(8, np.int64)
    rc = lib.mcf_cost_ranges_host(pl.n, pl.m, _p(arr(inst.tail, np.int32), i32), _p(arr(inst.head, np.int32), i32), _p(arr(inst.cost, np.int64), i64),
                                  _p(arr(pl.state, np.int8), i8), _p(arr(tree["parent"], np.int32), i32), _p(arr(tree["pred_arc"], np.int32), i32),
                                  _p(arr(tree["depth"], np.int32), i32), _p(arr(pi, np.int64), i64), chunk, _p(down, i64), _p(up, i64), _p(rep, i64))
    assert rc == 0
    return down[: pl.m], up[: pl.m], dict(zip(REPORT, (int(x) for x in rep)))


def _state(pl):
    tree = ry.planted_tree(pl)
    pi = pt.potentials(pl, tree, pl.inst.cost, pt.big_m(pl))
    return tree, pi, ry.reduced_costs(pl.inst.tail, pl.inst.head, pl.inst.cost, pi)


def _brute(pl, tree, rc):
    return ry.brute(pl.n, pl.inst.tail, pl.inst.head, pl.state, rc, tree["pos"], tree["size"], tree["pred_arc"], tree["depth"])


def _climb(pl, tree, rc):
    return ry.climb(pl.n, pl.inst.tail, pl.inst.head, pl.state, rc, tree["parent"], tree["depth"], tree["pred_arc"])


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert {k: got[2][k] for k in REPORT} == {k: want[2][k] for k in REPORT}, (got[2], want[2])


# ------------------------------------------------------------------ the ABI surface
def test_library_exports_the_entry_point_and_refuses_bad_arguments_before_any_device_work():
    lib = engine.load_library()
    assert "mcf_cost_ranges" in engine.ABI_SYMBOLS and "mcf_cost_ranges" in ge.declared_symbols()
    assert lib.mcf_abi_version() == 3 == engine.ABI_VERSION
    rep = engine.McfRangesReport()
    assert ctypes.sizeof(rep) == 8 * 8 + 8
    assert [name for name, _ in rep._fields_] == ["basic_real", "basic_artificial", "eligible", "max_depth", "levels", "inf_down", "inf_up",
                                                  "big_m", "device_ms"]
    assert lib.mcf_cost_ranges(None, -1, None, None, None, ctypes.byref(rep)) == -1               # MCF_E_BAD_ARG: null handle
    assert "MCF_RANGE_INF INT64_MAX" in (ge.ROOT / "include" / "mcf.h").read_text()


# ------------------------------------------------------------------ shapes and sizes
@pytest.mark.parametrize("n", (1, 2, 3, 64, 257))
@pytest.mark.parametrize("shape", pt.SHAPES)
def test_host_restatement_equals_brute_on_every_shape(host, shape, n):
    pl = pt.plant(shape, n, seed=n)
    tree, pi, rc = _state(pl)
    want = _brute(pl, tree, rc)
    _same(ranges_host(host, pl, tree, pi), want)
    if pl.m:
        s = pl.state.astype(np.int64) * rc
        lower = pl.state == 1
        assert np.array_equal(want[0][lower], s[lower]) and (want[1][lower] == ry.INF).all()


@pytest.mark.parametrize("d", pt.DEPTHS)
def test_host_restatement_across_the_levels_of_the_tables(host, d):
    """Greatest depths 1, 2^k, 2^k +- 1: K = bit_length(d) changes at 1 -> 2, 3 -> 4, 31 -> 32, 1023 -> 1024."""
    pl = pt.cold_plant() if d == 1 else pt.depth_plant(d)
    tree, pi, rc = _state(pl)
    want = _climb(pl, tree, rc) if d >= 1023 else _brute(pl, tree, rc)
    got = ranges_host(host, pl, tree, pi)
    _same(got, want)
    assert got[2]["max_depth"] == d and got[2]["levels"] == max(1, d.bit_length())
    assert [max(1, x.bit_length()) for x in (1, 2, 3, 4, 31, 32, 1023, 1024)] == [1, 2, 2, 3, 5, 6, 10, 11]


# ------------------------------------------------------------------ chosen chords
def _chord_case(name):
    """(shape, n, k, chords, parent or None): parent[v] < v in every shape, so the pairs below are what their names say."""
    if name == "parallel":           # path 0 - 1 - 2 - ...: the tree arc of node 5 joins 4 and 5; both senses
        return "path", 12, 1, [(4, 5), (5, 4)], None
    if name == "ancestor":           # path: 2 is an ancestor of 9 -- the side of 2 is empty
        return "path", 12, 1, [(9, 2), (2, 9)], None
    if name == "siblings":           # star: 3 and 7 hang on the centre 0
        return "star", 12, 1, [(3, 7), (7, 3)], None
    if name == "equal_depth_root":   # two paths 0 .. 7 and 8 .. 15 hung on the root: 3 and 11 (4 and 12) have equal depths, the join is the root
        parent = np.arange(16) - 1
        parent[8] = -1
        return "forest", 16, 2, [(3, 11), (12, 4)], parent
    if name == "forest":             # three components over 0..3, 4..7, 8..11: the paths run over artificial tree arcs
        return "forest", 12, 3, [(2, 9), (10, 5)], None
    raise ValueError(name)


def want_root(pl, v):
    """The top of v's component."""
    while pl.parent[v] < pl.n:
        v = int(pl.parent[v])
    return v


@pytest.mark.parametrize("name", ("parallel", "ancestor", "siblings", "equal_depth_root", "forest"))
def test_chosen_chords(host, name):
    shape, n, k, chords, given = _chord_case(name)
    pl = pt.plant(shape, n, m=n + 6, seed=3, k=k, chords=chords, parent=given)
    tree, pi, rc = _state(pl)
    depth, parent = tree["depth"], tree["parent"]
    (a, b), _ = chords
    if name == "parallel":
        assert parent[5] == 4
    elif name == "ancestor":
        assert depth[9] > depth[2] and tree["pos"][2] <= tree["pos"][9] < tree["pos"][2] + tree["size"][2]
    elif name == "siblings":
        assert parent[a] == parent[b] == 0
    elif name == "equal_depth_root":
        assert depth[a] == depth[b] == 4 and want_root(pl, a) != want_root(pl, b) and (pl.tree_arc[[0, 8]] >= pl.m).all()
    else:
        tops = np.flatnonzero(pl.parent == pl.n)
        comp = lambda v: int(np.searchsorted(tops, v, side="right"))                              # noqa: E731
        assert len(tops) == 3 and comp(a) != comp(b) and (pl.tree_arc[tops] >= pl.m).all()
    want = _brute(pl, tree, rc)
    _same(ranges_host(host, pl, tree, pi), want)
    _same(_climb(pl, tree, rc), want)
    # the chords are the first non-tree arcs, the first at capacity (state -1), the second at zero (+1)
    ids = [int(np.flatnonzero(~pl.in_tree & (pl.inst.tail == t) & (pl.inst.head == h))[0]) for t, h in chords]
    if name == "parallel":
        # each chord crosses the cut of exactly one tree arc: that of node 5
        e = int(pl.tree_arc[5])
        others = np.setdiff1d(np.flatnonzero(pl.in_tree), [e])
        s = pl.state.astype(np.int64) * rc
        crossing = [f for f in np.flatnonzero(~pl.in_tree) if (min(pl.inst.tail[f], pl.inst.head[f]) <= 4) and (max(pl.inst.tail[f], pl.inst.head[f]) >= 5)]
        assert set(ids) <= set(crossing)
        assert min(int(want[0][e]), int(want[1][e])) == min(int(s[f]) for f in crossing)
        assert len(others) == pl.n - 2


# ------------------------------------------------------------------ the yardsticks against each other, merge orders
def test_brute_equals_climb_on_a_common_case():
    for shape in ("random", "forest", "caterpillar"):
        pl = pt.plant(shape, 300, m=900, seed=17)
        tree, _, rc = _state(pl)
        b, c = _brute(pl, tree, rc), _climb(pl, tree, rc)
        assert np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1]) and b[2] == c[2]
        assert (b[0] < 0).any() and (b[1] < 0).any() and (b[0] == ry.INF).any()


@pytest.mark.parametrize("shape", ("random", "path", "forest"))
def test_chunks_of_one_seven_and_all_arcs_give_identical_arrays(host, shape):
    pl = pt.plant(shape, 257, m=700, seed=23)
    tree, pi, rc = _state(pl)
    first = ranges_host(host, pl, tree, pi, chunk=1)
    for chunk in (7, pl.m):
        _same(ranges_host(host, pl, tree, pi, chunk=chunk), first)
    _same(first, _brute(pl, tree, rc))


# ------------------------------------------------------------------ the instances of the contract test on the device
@pytest.mark.parametrize("which", ("golden", "graph"))
def test_the_contract_instances_offer_enough_arcs(host, which):
    """tests/test_gpu_cost_ranges.py picks 16 basic arcs with a finite end and 16 non-basic ones that can be tried below the
    dear arc's cost: at the optimal basis of the CPU emulation both instances offer many more."""
    if which == "golden":
        base = next(inst for s, inst in load_synthetic() if s["file"] == "netgen_8_10a_syn.npz")
    else:
        base = generators.netgen_style(1500, 12000, seed=3)
    inst, dear = ry.with_a_dear_arc(base)
    r = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0)
    assert r["status"] == "optimal"
    in_tree = r["in_tree"].astype(bool)
    state = np.where(in_tree, 0, np.where((r["flow"] == inst.cap) & (inst.cap > 0), -1, 1)).astype(np.int8)
    pi = np.append(r["potential"], 0)
    rc = ry.reduced_costs(inst.tail, inst.head, inst.cost, pi)
    down, up, rep = ry.climb(inst.n, inst.tail, inst.head, state, rc, r["parent"], r["depth"], r["pred_arc"])
    assert rep["eligible"] == 0 and (down >= 0).all() and (up >= 0).all()
    try_up, try_down = ry.triable_sides(inst.cost, down, up, dear)
    usable = try_up | try_down
    assert int((usable & in_tree).sum()) >= 64 and int((usable & ~in_tree).sum()) >= 64
    # the host restatement on a solved basis: deep tree, optimal, no negative entry
    class _Pl:                                                    # what ranges_host reads of a planted instance
        pass
    pl = _Pl()
    pl.n, pl.m, pl.inst, pl.state = inst.n, inst.m, inst, state
    _same(ranges_host(host, pl, {"parent": r["parent"], "pred_arc": r["pred_arc"], "depth": r["depth"]}, pi), (down, up, rep))
