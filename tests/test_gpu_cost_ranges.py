"""mcf_cost_ranges on the device, against the two yardsticks of ``ranges_yardsticks`` (``test_cost_ranges_cpu.py`` holds them
against each other and against the host restatement of the same per-arc logic).

  a. planted trees (``mcf_set_basis``, no pivot) on the dense array and the blocked list: the boundary sweep of
     ``planted_trees``, the depths round the powers of two (the number of table levels), an index list, two calls;
  b. past the caps: more nodes than lanes of a node pass, more arcs than lanes of the arc pass at its greatest grid;
  c. the contract on solved instances: a cost moved to the end of its range prices nothing in and costs no pivot, one unit
     further prices exactly violation 1 in;
  d. every engine path, Devex, dropped reduced costs, both ranks of a sharded pair; read-only; errors; the Python layer.

Nothing has a tolerance: the call is exact integer arithmetic."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import network_flow_solver_amd as nfs
import planted_trees as pt
import ranges_yardsticks as ry
from conftest import CASES, load_synthetic
from network_flow_solver_amd import generators

pytestmark = pytest.mark.gpu

FIELDS = ("basic_real", "basic_artificial", "eligible", "max_depth", "levels", "inf_down", "inf_up", "big_m")
# k_rng_arcs (csrc/mcf_passes_dev.h): at most kRngMaxBlocks = 2 048 workgroups of kRngThreads = 256 lanes; the grid is
# mcf_price_blocks(m) = 8 * ceil(m / 8 / 2 048) workgroups, so it reaches that cap from 8 * 255 * 2 048 arcs on
ARC_LANE_CAP = 2048 * 256
ARC_GRID_FULL_FROM = 8 * 255 * 2048 + 1


def _engine(e, inst, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, **kw)


def _install(e, pl, **kw):
    """A handle holding the planted basis, and its tree."""
    eng = _engine(e, pl.inst, **kw)
    if pl.in_tree.any():
        assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
    tree = eng.tree()
    assert np.array_equal(tree["parent"][: pl.n], pl.parent) and np.array_equal(tree["pred_arc"][: pl.n], pl.tree_arc)
    assert np.array_equal(tree["state"], pl.state)
    return eng, tree


def _want_planted(pl, tree, how):
    """The yardstick on the planted instance: potentials from the construction, the tree from mcf_get_tree."""
    bigm = pt.big_m(pl)
    pi = pt.potentials(pl, tree, pl.inst.cost, bigm)
    assert np.array_equal(tree["pi"], pi)
    rc = ry.reduced_costs(pl.inst.tail, pl.inst.head, pl.inst.cost, pi)
    if how == "brute":
        return ry.brute(pl.n, pl.inst.tail, pl.inst.head, pl.state, rc, tree["pos"], tree["size"], tree["pred_arc"], tree["depth"], bigm)
    return ry.climb(pl.n, pl.inst.tail, pl.inst.head, pl.state, rc, tree["parent"], tree["depth"], tree["pred_arc"], bigm)


def _want_resident(eng, inst, cost=None):
    """The yardstick from the handle's own tree and potentials (solved handles: deep trees, so by climbing)."""
    cost = inst.cost if cost is None else cost
    tree = eng.tree()
    rc = ry.reduced_costs(inst.tail, inst.head, cost, tree["pi"])
    return ry.climb(inst.n, inst.tail, inst.head, tree["state"], rc, tree["parent"], tree["depth"], tree["pred_arc"], pt.big_m(inst, cost))


def _assert_same(got, want):
    down, up, rep = got
    assert np.array_equal(down, want[0]), np.flatnonzero(down != want[0])[:8]
    assert np.array_equal(up, want[1]), np.flatnonzero(up != want[1])[:8]
    assert set(rep) == set(FIELDS) | {"device_ms"}
    assert {k: rep[k] for k in FIELDS} == want[2], {k: (rep[k], want[2][k]) for k in FIELDS if rep[k] != want[2][k]}


# ------------------------------------------------------------------ a. planted trees
@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("n,shape,m", [(c[1], c[2], c[4]) for c in pt.sweep_cases()], ids=[f"n{c[1]}-{c[2]}-m{c[4]}" for c in pt.sweep_cases()])
def test_boundary_sweep(gpu_engine_module, n, shape, m, tree_blocks):
    pl = pt.sweep_plant(n, shape, m)
    eng, tree = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        _assert_same(eng.cost_ranges(), _want_planted(pl, tree, "brute"))


@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("d", pt.DEPTHS)
def test_depths_around_powers_of_two(gpu_engine_module, d, tree_blocks):
    pl = pt.cold_plant() if d == 1 else pt.depth_plant(d)
    eng, tree = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        got = eng.cost_ranges()
        _assert_same(got, _want_planted(pl, tree, "climb" if d >= 1023 else "brute"))
        assert got[2]["max_depth"] == d and got[2]["levels"] == max(1, d.bit_length())


@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
def test_an_index_list_with_duplicates_and_a_second_call(gpu_engine_module, tree_blocks):
    pl = pt.sweep_plant(2047, "random", 4097)
    eng, tree = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        down, up, rep = eng.cost_ranges()
        _assert_same((down, up, rep), _want_planted(pl, tree, "brute"))
        rng = np.random.default_rng(12)
        idx = rng.integers(0, pl.m, 300)
        idx[10:20] = idx[0]                                        # duplicates, next to each other and apart
        idx[-1] = idx[5]
        d2, u2, r2 = eng.cost_ranges(idx)
        assert np.array_equal(d2, down[idx]) and np.array_equal(u2, up[idx])
        assert r2["inf_down"] == int((down[idx] == ry.INF).sum()) and r2["inf_up"] == int((up[idx] == ry.INF).sum())
        assert {k: r2[k] for k in FIELDS if not k.startswith("inf_")} == {k: rep[k] for k in FIELDS if not k.startswith("inf_")}
        d0, u0, r0 = eng.cost_ranges(np.zeros(0, np.int64))       # an empty list: an empty answer
        assert len(d0) == len(u0) == 0 and r0["inf_down"] == r0["inf_up"] == 0 and r0["eligible"] == rep["eligible"]
        d3, u3, r3 = eng.cost_ranges()                             # the second full call: identical arrays
        assert np.array_equal(d3, down) and np.array_equal(u3, up) and {k: r3[k] for k in FIELDS} == {k: rep[k] for k in FIELDS}


# ------------------------------------------------------------------ b. past the caps
@pytest.mark.parametrize("tree_blocks", (-1, 0), ids=["dense", "auto"])
def test_past_the_lane_cap_of_the_node_passes(gpu_engine_module, tree_blocks):
    pl = pt.large_plant("random")
    assert pl.n + 1 > pt.LANE_CAP and (pl.n + 1) % 256 != 0 and pl.m > ARC_LANE_CAP
    eng, tree = _install(gpu_engine_module, pl, tree_blocks=tree_blocks)
    with eng:
        got = eng.cost_ranges()
        _assert_same(got, _want_planted(pl, tree, "climb"))
        assert got[2]["basic_artificial"] == 65                    # the shape's top and the 64 single nodes


def test_past_the_lane_cap_of_the_arc_pass(gpu_engine_module):
    """More arcs than the arc pass has lanes at its greatest grid (ARC_LANE_CAP), over a small shallow tree."""
    m = ARC_GRID_FULL_FROM + 4099
    pl = pt.plant("binary", 63, m, seed=41)
    assert pl.m >= ARC_GRID_FULL_FROM and pl.m > 7 * ARC_LANE_CAP and pl.m % 256 != 0
    eng, tree = _install(gpu_engine_module, pl)
    with eng:
        _assert_same(eng.cost_ranges(), _want_planted(pl, tree, "climb"))


# ------------------------------------------------------------------ c. the contract, on solved instances
def _contract_instances():
    golden = next(inst for s, inst in load_synthetic() if s["file"] == "netgen_8_10a_syn.npz")
    return {"golden": (golden, dict()), "graph": (generators.netgen_style(1500, 12000, seed=3), dict(fused=False, mid_loop=-1))}


@pytest.mark.parametrize("which", ("golden", "graph"))
def test_the_end_of_a_range_costs_no_pivot_and_one_unit_more_prices_one_in(gpu_engine_module, which):
    e = gpu_engine_module
    base, kw = _contract_instances()[which]
    inst, dear = ry.with_a_dear_arc(base)
    m = inst.m
    with _engine(e, inst, rule=e.RULE_DANTZIG, **kw) as eng:
        eng.solve()
        assert eng.result().status == "optimal"
        down, up, rep = eng.cost_ranges()
        _assert_same((down, up, rep), _want_resident(eng, inst))
        assert rep["eligible"] == 0 and (down >= 0).all() and (up >= 0).all() and rep["basic_artificial"] >= 1
        bigm = rep["big_m"]
        assert bigm == (dear + 1) * (inst.n + 2)
        state = eng.tree()["state"]
        cost = inst.cost.astype(np.int64)
        # the sides that can be tried: a finite end whose cost, and the cost one unit past it, stay below the dear arc's
        try_up, try_down = ry.triable_sides(cost, down, up, dear)
        usable = try_up | try_down
        rng = np.random.default_rng(2026)
        basic, nonbasic = np.flatnonzero((state == 0) & usable), np.flatnonzero((state != 0) & usable)
        assert len(basic) >= 16 and len(nonbasic) >= 16, (len(basic), len(nonbasic))   # fewer: the test fails rather than shrinks
        picks = np.concatenate((rng.choice(basic, 16, replace=False), rng.choice(nonbasic, 16, replace=False)))
        pivots = eng.stats()["pivots"]
        sides = 0
        for a in picks.tolist():
            for ok, span, past in ((try_up[a], up[a], 1), (try_down[a], down[a], -1)):
                if not ok:
                    continue
                end = int(cost[a]) + past * int(span)
                sides += 1
                eng.update_costs([a], [int(end)])                  # the end of the range: nothing prices in, no pivot
                assert eng.cost_ranges([a])[2]["big_m"] == bigm
                assert eng.price_once(e.RULE_DANTZIG, 0, m) is None, (a, past)
                eng.solve()
                assert eng.stats()["pivots"] == pivots and eng.stats()["status"] == "optimal", (a, past)
                eng.update_costs([a], [int(end) + past])           # one unit past it: violation 1
                assert eng.cost_ranges([a])[2]["big_m"] == bigm
                hit = eng.price_once(e.RULE_DANTZIG, 0, m)
                assert hit is not None and hit[2] == 1, (a, past, hit)
                eng.update_costs([a], [int(cost[a])])              # back
                assert eng.cost_ranges([a])[2]["big_m"] == bigm
        assert sides >= 32
        d2, u2, r2 = eng.cost_ranges()                              # every cost restored: the same ranges
        assert np.array_equal(d2, down) and np.array_equal(u2, up) and r2["eligible"] == 0


# ------------------------------------------------------------------ d. every engine path
PATHS = {
    "small": (dict(), 0, (200, 1500)),                                             # k_solve_small (LDS)
    "mid": (dict(fused=False, mid_loop=1), 2, (700, 6000)),                        # k_solve_mid
    "graphs": (dict(fused=False, mid_loop=-1, tree_blocks=-1), 0, (1500, 12000)),   # captured graphs of three kernels per pivot
    "blocked": (dict(tree_blocks=2), 2, (1500, 12000)),
    "gather": (dict(fused=False, mid_loop=-1, resident_rc=False), 0, (700, 6000)),  # no resident reduced costs at all
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
        got = eng.cost_ranges()
        _assert_same(got, _want_resident(eng, inst))
        assert got[2]["eligible"] == 0 and (got[0] >= 0).all() and (got[1] >= 0).all()
        assert eng.certify()["verdict"] == "optimal"


def test_a_handle_solved_by_solve_batch(gpu_engine_module):
    e = gpu_engine_module
    insts = [generators.netgen_style(200, 1500, seed=s) for s in (3, 4)]
    engines = [_engine(e, i, rule=2) for i in insts]
    try:
        e.solve_batch(engines)
        for eng, inst in zip(engines, insts):
            assert eng.result().status == "optimal"
            got = eng.cost_ranges()
            _assert_same(got, _want_resident(eng, inst))
            assert got[2]["eligible"] == 0
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
        got = eng.cost_ranges()
        _assert_same(got, _want_resident(eng, inst))
        assert got[2]["eligible"] == 0


def test_both_ranks_of_a_sharded_pair(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(1500, 12000, seed=8)
    with _engine(e, inst, rule=0, fused=False, mid_loop=-1) as eng:
        eng.solve()
        res = eng.result()
        whole = eng.cost_ranges()
    answers = []
    for rank in (0, 1):
        with _engine(e, inst, rule=0, shard=(rank, 2), fused=False, mid_loop=-1) as eng:
            cold = eng.cost_ranges()                               # the cold start: every arc non-basic at zero, its own slack
            _assert_same(cold, _want_resident(eng, inst))
            assert cold[2]["basic_real"] == 0 and cold[2]["basic_artificial"] == inst.n
            assert eng.set_basis(res.in_tree, (res.flow == inst.cap) & ~res.in_tree & (inst.cap > 0))
            got = eng.cost_ranges()
            _assert_same(got, _want_resident(eng, inst))
            answers.append(got)
    for k in (0, 1):
        assert np.array_equal(answers[0][k], answers[1][k])
    assert {k: answers[0][2][k] for k in FIELDS} == {k: answers[1][2][k] for k in FIELDS}
    assert whole[2]["basic_real"] + whole[2]["basic_artificial"] == inst.n == answers[0][2]["basic_real"] + answers[0][2]["basic_artificial"]


# ------------------------------------------------------------------ read-only
@pytest.mark.parametrize("path", ("small", "mid", "graphs", "blocked", "devex"))
def test_the_call_changes_no_later_pivot(gpu_engine_module, path):
    e = gpu_engine_module
    kw, rule, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=5)
    runs = []
    for ranging in (False, True):
        with _engine(e, inst, rule=rule, **kw) as eng:
            eng.solve(150)
            if ranging:
                mid = eng.cost_ranges()
                _assert_same(mid, _want_resident(eng, inst))       # mid-solve: negative entries, reported as they are
                assert mid[2]["eligible"] > 0 and ((mid[0] < 0) | (mid[1] < 0)).any()
                eng.cost_ranges(np.arange(0, inst.m, 7))
            eng.solve(37)
            if ranging:
                eng.cost_ranges()
            eng.solve()
            res, tree = eng.result(), eng.tree()
        stats = {k: res.stats[k] for k in ("pivots", "degenerate", "bound_flips", "cycle_arcs", "subtree_nodes", "arcs_priced")}
        runs.append((res.status, res.objective, stats, res.flow, res.potential, tree["order"], tree["parent"], tree["state"]))
    a, b = runs
    assert a[:3] == b[:3]
    for x, y in zip(a[3:], b[3:]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_and_leave_the_handle_alone(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(200, 1500, seed=3)
    drop = ("arc_pass_ms", "node_pass_ms")
    with _engine(e, inst, rule=0) as eng:
        eng.solve()
        before = {k: v for k, v in eng.certify().items() if k not in drop}
        good = eng.cost_ranges()
        for bad in ([inst.m], [-1], [0, 5, inst.m + 3]):
            with pytest.raises(e.EngineError) as err:
                eng.cost_ranges(bad)
            assert err.value.code == -1 and "index" in str(err.value)
        lib, h = eng._lib, eng._h
        i64p = ctypes.POINTER(ctypes.c_int64)
        buf, idx = np.zeros(inst.m, np.int64), np.zeros(4, np.int64)
        ptr = lambda a: a.ctypes.data_as(i64p)                                                   # noqa: E731
        assert lib.mcf_cost_ranges(h, -1, None, None, ptr(buf), None) == -1                       # null down, entries to return
        assert lib.mcf_cost_ranges(h, -1, None, ptr(buf), None, None) == -1
        assert lib.mcf_cost_ranges(h, 4, ptr(idx), None, None, None) == -1
        assert lib.mcf_cost_ranges(h, 4, None, ptr(buf), ptr(buf), None) == -1                    # a count without a list
        assert lib.mcf_cost_ranges(h, 0, None, None, None, None) == 0                             # nothing to return: fine
        assert lib.mcf_cost_ranges(None, -1, None, ptr(buf), ptr(buf), None) == -1
        assert {k: v for k, v in eng.certify().items() if k not in drop} == before
        again = eng.cost_ranges()
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    with e.McfEngine(1, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(1, np.int64)) as eng:
        d, u, rep = eng.cost_ranges()                              # n == 1, m == 0: an empty answer
        assert len(d) == len(u) == 0 and rep["eligible"] == rep["basic_real"] == rep["inf_down"] == rep["inf_up"] == 0


# ------------------------------------------------------------------ the Python layer
def test_shim_cost_ranges_on_the_sample_problem(gpu_engine_module):
    case = next(c for c in CASES if c["name"] == "sample_problem")
    problem = nfs.build_problem(case["nodes"], case["arcs"], case["directed"], case["tolerance"])
    solver = nfs.NetworkSimplex(problem, nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True))
    first = solver.solve()
    assert first.status == "optimal" and first.objective == 15.0
    ranges = solver.cost_ranges()
    costs = {(a["tail"], a["head"]): a["cost"] for a in case["arcs"]}
    assert set(ranges) == set(costs) == set(solver.flat.keys)      # the keys update_costs takes
    for key, (lo, hi) in ranges.items():
        assert (lo is None or lo <= costs[key]) and (hi is None or costs[key] <= hi), (key, lo, hi)
    # s -> a -> t costs 3, s -> t costs 4: the direct arc may fall to 3 and rise for ever; caller's units
    assert ranges[("s", "t")] == (3.0, None)
    assert solver.cost_ranges([("s", "t")]) == {("s", "t"): (3.0, None)}
    with pytest.raises(nfs.InvalidProblemError):
        solver.cost_ranges([("t", "s")])
    # an edit inside every finite interval re-solves in 0 iterations
    for key, (lo, hi) in ranges.items():
        for c in (lo, hi):
            if c is None or abs(c) > max(costs.values()):      # (a new maximum would raise big-M: outside what the ranges promise)
                continue
            assert solver.update_costs({key: c}) == 1
            again = solver.solve()
            assert again.status == "optimal" and again.iterations == 0, (key, c)
            solver.update_costs({key: costs[key]})
            assert solver.solve().iterations == 0
    solver.update_costs({("s", "t"): 2.0})                         # below the interval: the basis changes
    assert solver.solve().iterations > 0


def test_shim_cost_ranges_on_an_soa_problem(gpu_engine_module):
    from network_flow_solver_amd.data import SoAProblem

    inst = generators.netgen_style(700, 6000, seed=17)
    soa = SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply)
    solver = nfs.NetworkSimplex(soa, nfs.SolverOptions(pricing_strategy="candidate_list", explicit_pricing_strategy=True))
    assert solver.solve().status == "optimal"
    lowest, highest = solver.cost_ranges()
    down, up, _ = solver.engine.cost_ranges()
    assert lowest.dtype == highest.dtype == np.int64
    assert np.array_equal(lowest, np.where(down == ry.INF, -ry.INF, inst.cost - np.where(down == ry.INF, 0, down)))
    assert np.array_equal(highest, np.where(up == ry.INF, ry.INF, inst.cost + np.where(up == ry.INF, 0, up)))
    assert (lowest <= inst.cost).all() and (inst.cost <= highest).all()
    idx = np.array([5, 5, 17, 0])
    lo2, hi2 = solver.cost_ranges(idx)
    assert np.array_equal(lo2, lowest[idx]) and np.array_equal(hi2, highest[idx])
    # (indices, costs), as update_costs takes them: three arcs moved to a finite end of their own range, one at a time
    finite = np.flatnonzero((highest > inst.cost) & (highest <= np.abs(inst.cost).max()))[:3]    # (no new maximum: big-M stays)
    assert len(finite) == 3
    for a in finite.tolist():
        assert solver.update_costs(([a], [int(highest[a])])) == 1
        assert solver.solve().iterations == 0
        solver.update_costs(([a], [int(inst.cost[a])]))
        assert solver.solve().iterations == 0
