"""mcf_certify_ray / mcf_certify_cut on the device, against Python-int yardsticks computed from downloaded arrays
(``farkas_yardsticks``: a parent-pointer walk, a queue search, plain sums) and the certificates of ``verdict_instances``.
Nothing here has a tolerance: both calls are exact integer arithmetic.  Every instance has its verdict by construction
(``tests/test_verdicts_cpu.py`` vets them), so none is ever skipped."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import farkas_yardsticks as fy
import verdict_instances as vi
from network_flow_solver_amd import generators

pytestmark = pytest.mark.gpu

RULE_IDS = {0: "dantzig", 1: "devex_block", 2: "candidate_list"}
MCF_INF = 1 << 60
GRAPH_BLOCKED = dict(fused=False, mid_loop=-1, tree_blocks=3)      # captured graphs over the blocked preorder list
GRAPH_DENSE = dict(fused=False, mid_loop=-1, tree_blocks=-1)       # ... over the dense preorder array
FORCINGS = {"graph_blocked": GRAPH_BLOCKED, "graph_dense": GRAPH_DENSE}
# the engine paths of the read-only test: options, nodes / arcs of the netgen-style instance
PATHS = {"small": (dict(), (200, 1500)), "mid": (dict(fused=False, mid_loop=1), (700, 6000)),
         "grid_dense": (GRAPH_DENSE, (1500, 12000)), "grid_blocked": (GRAPH_BLOCKED, (1500, 12000))}
TIMING = ("device_ms",)


@functools.lru_cache(maxsize=None)
def _instances(size):
    return vi.gpu_instances(size)


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _plain(d, drop=()):
    """A result dict without its timing and its arrays, for ==."""
    return {k: v for k, v in d.items() if k not in TIMING + ("arcs", "S") + tuple(drop)}


def _ray_yardstick(inst, res, tree, arc, backward):
    art = fy.artificial_flows(inst, res.flow)
    return fy.walk_ray(inst, tree["parent"], tree["pred_arc"], arc, backward, res.flow, tree["pi"], art, vi.big_m(inst))


def _check_ray(eng, inst):
    """After a solve that ended unbounded: the ray proves the verdict and equals the walked cycle.  Returns it."""
    res, tree = eng.result(), eng.tree()
    assert res.status == "unbounded"
    arc, rc = res.stats["unbounded_arc"], res.stats["unbounded_rc"]
    ray = eng.certify_ray()
    assert ray["proven"] and ray["arc"] == arc and ray["cost"] == ray["reduced_cost"] == rc < 0
    assert ray["theta"] == MCF_INF and ray["theta_arc"] == -1
    cycle = vi.cycle_of(inst, tree["parent"], tree["pred_arc"], arc)
    assert ray["arcs"].tolist() == [a for a, _ in cycle]
    assert ray["length"] == len(cycle) == vi.unbounded_certificate(inst, tree, arc, rc)
    want = _ray_yardstick(inst, res, tree, arc, False)
    assert _plain(ray) == _plain(want), (ray, want)
    again = eng.certify_ray()
    assert _plain(again) == _plain(ray) and np.array_equal(again["arcs"], ray["arcs"])           # bit-identical when repeated
    named = eng.certify_ray(arc)                                                               # the same arc by its index
    assert _plain(named) == _plain(ray) and np.array_equal(named["arcs"], ray["arcs"])
    bare = eng.certify_ray(want_arcs=False)
    assert "arcs" not in bare and _plain(bare) == _plain(ray)
    return ray


def _check_cut(eng, inst):
    """After a solve that ended infeasible: the computed cut proves it and equals the host search.  Returns it."""
    res = eng.result()
    assert res.status == "infeasible"
    cut = eng.certify_cut()
    art = fy.artificial_flows(inst, res.flow)
    S, levels = fy.residual_search(inst, res.flow, art)
    assert np.array_equal(cut["S"], S)
    want = fy.cut_sums(inst, S, res.flow, art)
    want["rounds"] = levels
    assert _plain(cut) == want, (cut, want)
    assert cut["proven"] and cut["deficit_in_S"] == cut["leaving_unsaturated"] == cut["entering_with_flow"] == 0
    # stats.artificial_flow adds up the artificial arcs of both senses, which carry the same amount: twice what leaves S
    assert cut["excess"] == cut["artificial_out"] > 0 and 2 * cut["excess"] == res.stats["artificial_flow"]
    again = eng.certify_cut()
    assert _plain(again) == _plain(cut) and np.array_equal(again["S"], cut["S"])
    # the set it found, handed back as the caller's: the same instance-side figures, nothing from the flow
    back = eng.certify_cut(cut["S"])
    assert _plain(back) == fy.cut_sums(inst, S) and back["proven"]
    assert all(back[k] == cut[k] for k in ("leaving_arcs", "capacity", "supply", "excess", "nodes_in_S"))
    return cut


# ------------------------------------------------------------------ 1. unbounded instances
@pytest.mark.parametrize("rule", (0, 1, 2), ids=RULE_IDS.values())
@pytest.mark.parametrize("size", ["small", "medium"])
def test_every_unbounded_instance_yields_its_ray(gpu_engine_module, size, rule):
    seen = 0
    for name, (inst, want, _) in _instances(size).items():
        if want != "unbounded":
            continue
        with _engine(gpu_engine_module, inst, rule) as eng:
            eng.solve()
            ray = _check_ray(eng, inst)
        if name == "deep_unbounded":
            assert ray["length"] == inst.n
        seen += 1
    assert seen == (4 if size == "small" else 2)


@pytest.mark.parametrize("case", [("small", "unbounded_5"), ("medium", "unbounded_600")], ids=lambda c: c[1])
def test_the_ray_is_the_same_on_every_engine_path(gpu_engine_module, case):
    """The pivot sequence does not depend on the engine path, so the verdict's tree and its ray do not either."""
    inst = _instances(case[0])[case[1]][0]
    rays = {}
    for path, kw in {"default": dict(), **FORCINGS}.items():
        with _engine(gpu_engine_module, inst, 2, **kw) as eng:
            eng.solve()
            stats = eng.stats()
            rays[path] = _check_ray(eng, inst)
        if path != "default":
            assert stats["pricing_mode"] in (0, 1) and (stats["tree_blocks"] == 3) == (path == "graph_blocked")
    for path in FORCINGS:
        assert _plain(rays[path]) == _plain(rays["default"]) and np.array_equal(rays[path]["arcs"], rays["default"]["arcs"]), path


@pytest.mark.parametrize("path", ["default", "graph_blocked"])
def test_a_ray_of_600_arcs(gpu_engine_module, path):
    """The chain family at 600 nodes: the verdict's cycle is the whole chain, longer than the cycle scan's path buffers."""
    inst = vi.deep_unbounded(600)
    with _engine(gpu_engine_module, inst, 0, **({} if path == "default" else GRAPH_BLOCKED)) as eng:
        eng.solve()
        ray = _check_ray(eng, inst)
        short = eng._lib.mcf_certify_ray                                                  # a buffer of 7: the head of the cycle
        idx = np.full(9, -7, np.int64)
        out = gpu_engine_module.McfRay()
        assert short(eng._h, -1, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 7, ctypes.byref(out)) == 0
    assert ray["length"] == 600 and ray["arcs"].tolist() == [599] + list(range(599))
    assert out.length == 600 and idx.tolist() == [599, 0, 1, 2, 3, 4, 5, -7, -7]


def test_rays_of_non_basic_arcs_of_an_optimal_handle(gpu_engine_module):
    """Forty seeded non-basic arcs of the optimal medium instance, both push directions, on the blocked list: every field
    equals the walk; none is proven."""
    inst = _instances("medium")["uncap_0"][0]
    with _engine(gpu_engine_module, inst, 2, **GRAPH_BLOCKED) as eng:
        eng.solve()
        res, tree = eng.result(), eng.tree()
        assert res.status == "optimal"
        rng = np.random.default_rng(40)
        lower, upper = np.flatnonzero(tree["state"] > 0), np.flatnonzero(tree["state"] < 0)
        assert len(upper) >= 10                                     # arcs at capacity: pushed backward
        arcs = np.concatenate((rng.choice(lower, 30, replace=False), rng.choice(upper, 10, replace=False)))
        bounded = 0
        for arc in arcs.tolist():
            backward = bool(tree["state"][arc] < 0)
            ray = eng.certify_ray(arc)
            want = _ray_yardstick(inst, res, tree, arc, backward)
            assert _plain(ray) == _plain(want) and ray["arcs"].tolist() == want["arcs"], arc
            assert not ray["proven"] and ray["cost"] == ray["reduced_cost"]
            bounded += ray["theta"] < MCF_INF
        assert bounded > 0


# ------------------------------------------------------------------ 2. infeasible instances
@pytest.mark.parametrize("rule", (0, 1, 2), ids=RULE_IDS.values())
@pytest.mark.parametrize("size", ["small", "medium"])
def test_every_infeasible_instance_yields_its_cut(gpu_engine_module, size, rule):
    seen = 0
    for name, (inst, want, _) in _instances(size).items():
        if want != "infeasible":
            continue
        with _engine(gpu_engine_module, inst, rule) as eng:
            eng.solve()
            cut = _check_cut(eng, inst)
        assert 0 < cut["nodes_in_S"] < inst.n
        seen += 1
    assert seen == (3 if size == "small" else 2)


@pytest.mark.parametrize("path", list(FORCINGS))
def test_the_cut_on_the_forced_engine_paths(gpu_engine_module, path):
    inst = _instances("medium")["cut"][0]
    with _engine(gpu_engine_module, inst, 2, **FORCINGS[path]) as eng:
        eng.solve()
        forced = _check_cut(eng, inst)
    with _engine(gpu_engine_module, inst, 2) as eng:
        eng.solve()
        default = _check_cut(eng, inst)
    assert _plain(forced) == _plain(default) and np.array_equal(forced["S"], default["S"])


def test_handles_without_resident_reduced_costs_and_sharded_handles(gpu_engine_module):
    """The gather path keeps no adjacency (the call builds its own on first use); a shard keeps only its own: every arc is
    still looked at, because the state is replicated."""
    inst = _instances("medium")["starved"][0]
    with _engine(gpu_engine_module, inst, 2) as eng:
        eng.solve()
        want = _check_cut(eng, inst)
    with _engine(gpu_engine_module, inst, 0, fused=False, mid_loop=-1, resident_rc=False) as eng:
        eng.solve()
        assert eng.stats()["pricing_mode"] == 0
        _check_cut(eng, inst)
    with _engine(gpu_engine_module, inst, 2, shard=(1, 3), fused=False, mid_loop=-1) as eng:   # the cold start of a shard
        flow0 = np.zeros(inst.m, np.int64)
        art0 = fy.artificial_flows(inst, flow0)
        S0, levels = fy.residual_search(inst, flow0, art0)
        cold = fy.cut_sums(inst, S0, flow0, art0)
        cold["rounds"] = levels
        cut = eng.certify_cut()
        assert _plain(cut) == cold and np.array_equal(cut["S"], S0)
        assert _plain(eng.certify_cut(want["S"])) == fy.cut_sums(inst, want["S"])
        tree = eng.tree()
        for arc in (0, inst.m // 2, inst.m - 1):                   # every real arc is non-basic: its cycle passes the root
            ray = eng.certify_ray(arc)
            walked = fy.walk_ray(inst, tree["parent"], tree["pred_arc"], arc, False, flow0, tree["pi"], art0, vi.big_m(inst))
            assert _plain(ray) == _plain(walked) and ray["arcs"].tolist() == walked["arcs"]
            assert ray["artificial_count"] == (2 if inst.tail[arc] != inst.head[arc] else 0) and not ray["proven"]
    unb = _instances("medium")["unbounded_5"][0]
    with _engine(gpu_engine_module, unb, 0, fused=False, mid_loop=-1, resident_rc=False) as eng:
        eng.solve()
        _check_ray(eng, unb)


# ------------------------------------------------------------------ 3. search depth
def test_the_search_goes_as_deep_as_the_residual_graph(gpu_engine_module):
    """A chain of 300 nodes, cut between 199 and 200: S = {0 .. 199}, one round per node -- 200 rounds, more than six batches
    of the 32 rounds queued between two looks at the level word."""
    inst = fy.chain_cut_instance(300, 199, 1000, 400)
    for kw in (dict(), GRAPH_DENSE):
        with _engine(gpu_engine_module, inst, 0, **kw) as eng:
            eng.solve()
            cut = _check_cut(eng, inst)
        assert cut["nodes_in_S"] == 200 and cut["proven"] and cut["rounds"] == 200 >= 32 + 1
        assert cut["S"][:200].all() and not cut["S"][200:].any()
        assert (cut["leaving_arcs"], cut["capacity"], cut["supply"], cut["excess"]) == (1, 400, 1000, 600)


# ------------------------------------------------------------------ 4. the caller's cut, no solve
@pytest.mark.parametrize("size", ["small", "medium"])
def test_callers_cut_on_a_fresh_handle(gpu_engine_module, size):
    inst = _instances(size)["cut"][0]
    inside = np.zeros(inst.n, bool)
    inside[vi.cut_set(inst)] = True
    leaving, capacity, supply = vi.cut_of(inst)
    with _engine(gpu_engine_module, inst, 0) as eng:
        cut = eng.certify_cut(inside)
        other = eng.certify_cut(~inside)
        empty = eng.certify_cut()                                   # computed on the cold start: every supply node is a seed
        assert eng.stats()["pivots"] == 0 and eng.stats()["status"] == "running"
    assert cut["proven"] and np.array_equal(cut["S"], inside)
    assert (cut["leaving_arcs"], cut["capacity"], cut["supply"], cut["excess"]) == (len(leaving), capacity, supply, supply - capacity)
    assert _plain(cut) == fy.cut_sums(inst, inside) and _plain(other) == fy.cut_sums(inst, ~inside) and not other["proven"]
    flow0 = np.zeros(inst.m, np.int64)
    art0 = fy.artificial_flows(inst, flow0)
    S0, levels = fy.residual_search(inst, flow0, art0)
    want = fy.cut_sums(inst, S0, flow0, art0)
    want["rounds"] = levels
    assert _plain(empty) == want and np.array_equal(empty["S"], S0) and empty["seeds"] == int((inst.supply > 0).sum())
    # an uncapacitated leaving arc spoils the cut even where the finite capacities alone fall short
    cap = inst.cap.copy()
    cap[int(leaving[np.flatnonzero(inst.cap[leaving] == 0)[0]])] = -1
    opened = generators.ArcSoA(inst.n, inst.tail, inst.head, inst.cost, cap, inst.supply, "opened")
    with _engine(gpu_engine_module, opened, 0) as eng:
        cut = eng.certify_cut(inside, want_set=False)
    assert cut["leaving_uncapacitated"] == 1 and not cut["proven"] and cut["excess"] == supply - capacity > 0 and "S" not in cut


def test_an_optimal_handle_has_no_seeds(gpu_engine_module):
    inst = _instances("small")["uncap_0"][0]
    with _engine(gpu_engine_module, inst, 0) as eng:
        eng.solve()
        cut = eng.certify_cut()
    assert not cut["S"].any() and not cut["proven"] and not any(_plain(cut).values())


# ------------------------------------------------------------------ 5. read-only
@pytest.mark.parametrize("rule", (0, 2), ids=["dantzig", "candidate_list"])
@pytest.mark.parametrize("path", list(PATHS))
def test_neither_call_changes_a_later_pivot(gpu_engine_module, path, rule):
    kw, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=5)
    runs = []
    for witness in (False, True):
        with _engine(gpu_engine_module, inst, rule, **kw) as eng:
            if witness:
                eng.certify_cut()
            for _ in range(4):                                     # a budgeted solve, both calls between the slices
                eng.solve(45)
                if witness:
                    tree = eng.tree()
                    eng.certify_cut()
                    eng.certify_ray(int(np.flatnonzero(tree["state"] != 0)[0]))
                    eng.certify_cut(np.arange(inst.n) % 2 == 0)
            eng.solve()
            res, tree = eng.result(), eng.tree()
        stats = {k: res.stats[k] for k in ("pivots", "degenerate", "bound_flips", "cycle_arcs", "subtree_nodes", "arcs_priced")}
        runs.append((res.status, res.objective, stats, res.flow, res.potential, tree["order"], tree["parent"], tree["state"]))
    a, b = runs
    assert a[0] == "optimal" and a[:3] == b[:3]
    for x, y in zip(a[3:], b[3:]):
        assert np.array_equal(x, y)


def test_mid_solve_states_are_reported_as_they_stand(gpu_engine_module):
    """After 30 and 90 pivots of the infeasible medium instance on the blocked list: the computed set equals the host search
    over the downloaded flows, deficits and open arcs included; the ray of a non-basic arc equals the walk."""
    inst = _instances("medium")["cut"][0]
    with _engine(gpu_engine_module, inst, 2, **GRAPH_BLOCKED) as eng:
        for k in (30, 60):
            eng.solve(k)
            res, tree = eng.result(), eng.tree()
            cut = eng.certify_cut()
            art = fy.artificial_flows(inst, res.flow)
            S, levels = fy.residual_search(inst, res.flow, art)
            want = fy.cut_sums(inst, S, res.flow, art)
            want["rounds"] = levels
            assert np.array_equal(cut["S"], S) and _plain(cut) == want
            arc = int(np.flatnonzero(tree["state"] != 0)[k])
            ray = eng.certify_ray(arc)
            want = _ray_yardstick(inst, res, tree, arc, bool(tree["state"][arc] < 0))
            assert _plain(ray) == _plain(want) and ray["arcs"].tolist() == want["arcs"]


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_handle_as_it_was(gpu_engine_module):
    e = gpu_engine_module
    inst = _instances("small")["uncap_0"][0]
    with _engine(e, inst, 0) as eng:
        eng.solve()
        before, tree = eng.result(), eng.tree()
        cert = eng.certify()
        basic = int(np.flatnonzero(tree["state"] == 0)[0])
        for arc, code in ((-1, -6), (basic, -1), (inst.m, -1), (-2, -1)):       # MCF_E_STATE; MCF_E_BAD_ARG three times
            with pytest.raises(e.EngineError) as err:
                eng.certify_ray(arc)
            assert err.value.code == code, arc
        idx = np.zeros(4, np.int64)
        i64p = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        ray = e.McfRay()
        nonbasic = int(np.flatnonzero(tree["state"] != 0)[0])
        assert eng._lib.mcf_certify_ray(eng._h, nonbasic, i64p, 4, None) == -1             # null out
        assert eng._lib.mcf_certify_ray(eng._h, nonbasic, None, 4, ctypes.byref(ray)) == -1   # a capacity without a buffer
        assert eng._lib.mcf_certify_ray(eng._h, nonbasic, i64p, -1, ctypes.byref(ray)) == -1
        assert eng._lib.mcf_certify_cut(eng._h, None, None, None) == -1
        after, tree2 = eng.result(), eng.tree()
        assert after.status == before.status == "optimal" and after.stats["pivots"] == before.stats["pivots"]
        assert np.array_equal(after.flow, before.flow) and np.array_equal(after.potential, before.potential)
        assert all(np.array_equal(tree[k], tree2[k]) for k in tree)
        again = eng.certify()
        assert {k: v for k, v in again.items() if not k.endswith("_ms")} == {k: v for k, v in cert.items() if not k.endswith("_ms")}
        eng.solve()
        assert eng.result().stats["pivots"] == before.stats["pivots"]
    with _engine(e, _instances("small")["starved"][0], 0) as eng:                          # infeasible is not unbounded either
        eng.solve()
        with pytest.raises(e.EngineError) as err:
            eng.certify_ray()
        assert err.value.code == -6


# ------------------------------------------------------------------ 7. mcf_solve_batch
def test_handles_solved_in_one_batch_yield_their_witnesses(gpu_engine_module):
    e = gpu_engine_module
    cases = _instances("small")
    names = ("unbounded_2", "starved", "unbounded_5", "cut", "uncap_0", "deep_unbounded", "isolated")
    engines = [_engine(e, cases[name][0], 2) for name in names]
    try:
        e.solve_batch(engines)
        for name, eng in zip(names, engines):
            inst, want, _ = cases[name]
            assert eng.result().status == want
            if want == "unbounded":
                _check_ray(eng, inst)
            elif want == "infeasible":
                _check_cut(eng, inst)
            else:
                assert not eng.certify_cut()["proven"]
    finally:
        for eng in engines:
            eng.close()


# ------------------------------------------------------------------ 8. the Python layer
def test_unbounded_ray_after_the_raised_error(gpu_engine_module):
    import network_flow_solver_amd as nfs

    nodes = [{"id": "s", "supply": 2.5}, {"id": "a", "supply": 0.0}, {"id": "b", "supply": 0.0}, {"id": "c", "supply": 0.0},
             {"id": "t", "supply": -2.5}]
    arcs = [{"tail": "s", "head": "a", "capacity": 4.0, "cost": 1.0}, {"tail": "a", "head": "t", "capacity": None, "cost": 1.0},
            {"tail": "a", "head": "b", "capacity": None, "cost": 0.5}, {"tail": "b", "head": "c", "capacity": None, "cost": -1.25},
            {"tail": "c", "head": "a", "capacity": None, "cost": 0.5}]
    problem = nfs.build_problem(nodes, arcs, directed=True, tolerance=1e-6)
    solver = nfs.NetworkSimplex(problem)
    with pytest.raises(nfs.UnboundedProblemError) as err:
        solver.solve()
    ray = solver.unbounded_ray()
    assert isinstance(ray, nfs.UnboundedRay) and ray.proven and ray.length == 3
    assert ray.arcs[0] == err.value.entering_arc and sorted(ray.arcs) == [("a", "b"), ("b", "c"), ("c", "a")]
    assert all(ray.arcs[i][1] == ray.arcs[(i + 1) % 3][0] for i in range(3))                  # push order: head meets tail
    assert ray.cost == ray.reduced_cost == err.value.reduced_cost == -0.25
    assert ray.raw["cost"] == -25 and ray.raw["theta"] == MCF_INF
    # the same through an SoAProblem: indices instead of keys
    soa = nfs.SoAProblem(3, np.array([0, 1, 2, 0]), np.array([1, 2, 0, 2]), np.array([1, 1, -3, 5]), np.array([-1, -1, -1, 7]),
                         np.array([1, 0, -1]))
    solver = nfs.NetworkSimplex(soa)
    with pytest.raises(nfs.UnboundedProblemError):
        solver.solve()
    ray = solver.unbounded_ray()
    assert ray.proven and sorted(ray.arcs) == [0, 1, 2] and ray.cost == -1.0


def test_infeasibility_cut_with_lower_bounds_in_the_callers_units(gpu_engine_module):
    import network_flow_solver_amd as nfs

    # s supplies 10.5; {s, a} can send out at most 3.5 + 2.25; the arc t -> a has to carry at least 1.5 INTO the set
    nodes = [{"id": "s", "supply": 10.5}, {"id": "a", "supply": 0.0}, {"id": "b", "supply": 0.0}, {"id": "t", "supply": -10.5}]
    arcs = [{"tail": "s", "head": "a", "capacity": None, "cost": 1.0}, {"tail": "a", "head": "b", "capacity": 3.5, "cost": 1.0, "lower": 1.0},
            {"tail": "s", "head": "t", "capacity": 2.25, "cost": 4.0}, {"tail": "b", "head": "t", "capacity": None, "cost": 1.0},
            {"tail": "t", "head": "a", "capacity": 5.0, "cost": 0.5, "lower": 1.5}]
    problem = nfs.build_problem(nodes, arcs, directed=True, tolerance=1e-6)
    solver = nfs.NetworkSimplex(problem)
    assert solver.solve().status == "infeasible"
    cut = solver.infeasibility_cut()
    assert isinstance(cut, nfs.InfeasibleCut) and cut.proven
    assert cut.nodes == ["a", "s"] and sorted(cut.leaving_arcs) == [("a", "b"), ("s", "t")]
    assert (cut.capacity, cut.supply, cut.entering_lower, cut.excess) == (5.75, 10.5, 1.5, 6.25)
    assert cut.excess == cut.supply + cut.entering_lower - cut.capacity
    assert cut.raw["excess"] == cut.raw["artificial_out"] == 625 and cut.raw["leaving_uncapacitated"] == 0
    # the caller's own set, on a solver that never solved
    fresh = nfs.NetworkSimplex(problem)
    named = fresh.infeasibility_cut(["s", "a"])
    assert (named.nodes, named.capacity, named.supply, named.excess, named.proven) == (cut.nodes, 5.75, 10.5, 6.25, True)
    loose = fresh.infeasibility_cut(["s"])                                   # s -> a is uncapacitated: proves nothing
    assert not loose.proven and loose.raw["leaving_uncapacitated"] == 1 and loose.leaving_arcs == [("s", "a"), ("s", "t")]
    with pytest.raises(nfs.InvalidProblemError):
        fresh.infeasibility_cut(["nobody"])
    # SoAProblem: indices
    soa = nfs.SoAProblem(3, np.array([0, 1]), np.array([1, 2]), np.array([1, 1]), np.array([-1, 4]), np.array([9, 0, -9]),
                         lower=np.array([0, 1]))
    solver = nfs.NetworkSimplex(soa)
    assert solver.solve().status == "infeasible"
    cut = solver.infeasibility_cut()
    assert cut.proven and cut.nodes == [0, 1] and cut.leaving_arcs == [1] and (cut.capacity, cut.supply, cut.excess) == (4.0, 9.0, 5.0)
