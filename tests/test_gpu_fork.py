"""mcf_fork / mcf_restore on the device: a fork is a complete copy of a resident handle -- every introspection call answers
for it what it answers for the source, bit for bit, and it goes on pivoting exactly as the source would, in every state
(mid-solve included), on every engine path, tree layout, rule and key_mode -- and ``solve_scenarios`` on top of it.

Every comparison is exact.  Measured times (``*_ms``, ``*_seconds``) are the only fields left out."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import oracle
from network_flow_solver_amd import (InvalidProblemError, NetworkSimplex, SolverOptions, UnboundedProblemError, build_problem, generators,
                                     solve_min_cost_flow, solve_scenarios)
from network_flow_solver_amd import engine as eng_mod
from network_flow_solver_amd.data import SoAProblem
from session_model import PIN

pytestmark = pytest.mark.gpu

DANTZIG, DEVEX, CANDIDATE = 0, 1, 2
ORACLE_RULE = {DANTZIG: "dantzig", DEVEX: "devex", CANDIDATE: "candidate_list"}
COUNTERS = ("pivots", "degenerate", "bound_flips", "arcs_priced", "cycle_arcs", "subtree_nodes", "nodes_moved", "cycle_scans")
GRID = dict(fused=False, mid_loop=-1)


@functools.lru_cache(maxsize=None)
def netgen(n, m, seed=1):
    return generators.netgen_style(n, m, seed=seed)


@functools.lru_cache(maxsize=None)
def oracle_iterations(n, m, seed, rule):
    return int(oracle.solve_soa(netgen(n, m, seed), ORACLE_RULE[rule])["iterations"])


def first_leg(n, m, seed, rule, at_least=0):
    """About a third of the oracle's pivot count, made a prime: no multiple of 64 (the batch), nor of the
    minor-iteration period, nor of anything else a launch shape could divide."""
    k = max(oracle_iterations(n, m, seed, rule) // 3, at_least, 3)
    while any(k % p == 0 for p in range(2, int(k ** 0.5) + 1)):
        k += 1
    return k


def make(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _exact(d):
    return {k: v for k, v in d.items() if not (k.endswith("_ms") or k.endswith("_seconds") or isinstance(v, float))}


def introspect(eng):
    """Everything the contract lists, measured times left out."""
    r = eng.result()
    rc, resident = eng.reduced_costs()
    keys, present = eng.pricing_keys()
    down, up, rep = eng.cost_ranges()
    return {"status": r.status, "objective": r.objective, "flow": r.flow, "potential": r.potential, "in_tree": r.in_tree,
            "stats": _exact(r.stats), "tree": eng.tree(), "rc": rc, "resident": resident, "keys": keys, "present": present,
            "weights": eng.weights(), "certificate": _exact(eng.certify()), "ranges": (down, up), "ranges_report": _exact(rep)}


# counts of host calls and launches: equal on two handles only when both were driven through the same calls
CALL_COUNTS = ("batches", "price_launches", "pivot_launches", "apply_launches", "loop_launches")


def assert_same(a, b, what="", same_calls=True):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if k == "stats" and not same_calls:
            x, y = ({f: v for f, v in d.items() if f not in CALL_COUNTS} for d in (x, y))
        if isinstance(x, dict):
            assert x.keys() == y.keys(), (what, k)
            for kk in x:
                if isinstance(x[kk], np.ndarray):
                    assert np.array_equal(x[kk], y[kk]), (what, k, kk)
                else:
                    assert x[kk] == y[kk], (what, k, kk, x[kk], y[kk])
        elif isinstance(x, tuple):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), (what, k)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)
        else:
            assert x == y, (what, k, x, y)


def twin_continuation(e, inst, rule, kw, k, before_fork=None, check_leg_one=None):
    """The core test.  A and a control B (never forked) make the first leg of k pivots and stop mid-solve; A is forked three
    times and every fork answers as A; a second leg on A, B and fork 0 shows that the fork did not disturb A (A == B) and
    that fork 0 goes on as A; A is destroyed, fork 1 and B run to the end alike; an edit of fork 2 leaves fork 0 alone."""
    a, b = make(e, inst, rule, **kw), make(e, inst, rule, **kw)
    forks = []
    try:
        if before_fork is not None:
            inst = before_fork(a, b, inst)
        a.solve(max_pivots=k); b.solve(max_pivots=k)
        ia = introspect(a)
        assert ia["status"] == "iteration_limit", "the first leg must end mid-solve, otherwise the test shows nothing"
        if check_leg_one is not None:
            check_leg_one(ia)
        rep = {}
        forks = a.fork(3, report=rep)
        assert rep["count"] == 3 and rep["segments"] > 0 and rep["bytes_per_fork"] > 0
        for i, f in enumerate(forks):
            assert_same(ia, introspect(f), f"fork {i} after the fork")
        assert_same(ia, introspect(a), "the source after the fork")
        # leg two on the source, the control and fork 0
        for h in (a, b, forks[0]):
            h.solve(max_pivots=k)
        ia2 = introspect(a)
        assert_same(ia2, introspect(b), "source against the control after leg two: the fork disturbed the source")
        i02 = introspect(forks[0])
        assert_same(ia2, i02, "fork 0 against the source after leg two")
        # the source goes away; fork 1 and the control run to the end
        a.close()
        forks[1].solve(); b.solve()
        i1, ib = introspect(forks[1]), introspect(b)
        assert_same(ib, i1, "fork 1 against the control at the end", same_calls=False)   # (fork 1 sat out leg two)
        assert i1["status"] == "optimal" and all(i1["stats"][c] == ib["stats"][c] for c in COUNTERS)
        assert i1["certificate"]["verdict"] == "optimal" and i1["certificate"]["proves_status"]
        assert i1["objective"] == int(round(oracle.solve_soa(inst, "dantzig")["objective"]))
        # an edit of fork 2 leaves fork 0 alone
        arcs = np.arange(0, inst.m, 7)
        forks[2].update_costs(arcs, forks[2].cost[arcs] + 3)
        assert_same(i02, introspect(forks[0]), "fork 0 after an edit of fork 2")
        assert np.array_equal(forks[0].cost, np.asarray(inst.cost)) and forks[2].cost[0] == inst.cost[0] + 3
    finally:
        for h in [a, b] + forks:
            h.close()


def _priority(m):
    return np.random.default_rng(9).integers(0, 4, m).astype(np.int8)


TWINS = {
    # path: (n, m, rule, options)
    "lds_dantzig": (64, 512, DANTZIG, {}),
    "lds_devex": (64, 512, DEVEX, {}),
    "lds_candidate": (64, 512, CANDIDATE, {}),
    "mid_devex": (512, 4096, DEVEX, dict(mid_loop=1)),
    "mid_candidate": (512, 4096, CANDIDATE, dict(mid_loop=1)),
    "grid_graph": (512, 4096, DANTZIG, dict(GRID)),
    "grid_no_graph": (512, 4096, DANTZIG, dict(GRID, use_graph=False)),
    "grid_no_rcache": (512, 4096, DANTZIG, dict(GRID, resident_rc=False)),
    "grid_key_codes": (512, 4096, DANTZIG, dict(GRID, compressed_keys=1)),
    "grid_dirty_marks": (512, 4096, DANTZIG, dict(GRID, full_sweeps=-1)),
    "grid_candidate_cache": (512, 4096, CANDIDATE, dict(GRID)),
    "grid_devex_tuner": (512, 4096, DEVEX, dict(GRID, devex_tuner=1)),
    "blocked_list": (512, 4096, DANTZIG, dict(GRID, tree_blocks=3)),
    "blocked_list_no_pool": (512, 4096, DANTZIG, dict(GRID, tree_blocks=3, tree_pool=-1)),
    "blocked_list_run": (512, 4096, CANDIDATE, dict(GRID, tree_blocks=3, pivot_run=2)),
    "key_mode_2": (512, 4096, DANTZIG, dict(GRID, key_mode=2)),
}


@pytest.mark.parametrize("path", list(TWINS))
def test_twin_continuation(gpu_engine_module, path):
    n, m, rule, kw = TWINS[path]
    kw = dict(kw, **PIN)
    if kw.get("key_mode") == 2:
        kw["arc_priority"] = _priority(m)
    inst = netgen(n, m)

    def check(ia):
        mode = ia["stats"]["pricing_mode"]
        assert mode == (2 if path.startswith("lds") else 3 if path.startswith("mid") else mode)
        if path == "grid_key_codes":
            assert ia["present"]
        if path == "grid_no_rcache":
            assert not ia["resident"]
        if path.startswith("blocked"):
            assert ia["stats"]["tree_blocks"] > 0
    twin_continuation(gpu_engine_module, inst, rule, kw, first_leg(n, m, 1, rule), check_leg_one=check)


def test_twin_continuation_after_the_reduced_costs_were_dropped(gpu_engine_module):
    n, m = 3000, 24000
    kw = dict(GRID, tree_blocks=3, rc_drop=1, **PIN)

    def check(ia):
        assert ia["stats"]["rc_dropped_at"] > 0 and not ia["resident"]
    # (the handle looks at its subtree sizes every 4 096 pivots: the first leg has to go past the first look)
    twin_continuation(gpu_engine_module, netgen(n, m), CANDIDATE, kw, first_leg(n, m, 1, CANDIDATE, at_least=5000), check_leg_one=check)


# ------------------------------------------------------------------ after the edits that reshape a handle

def _extra_arcs(inst, k, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, inst.n, k)
    h = (t + 1 + rng.integers(0, inst.n - 1, k)) % inst.n
    return t.astype(np.int32), h.astype(np.int32), rng.integers(1, 10001, k).astype(np.int64), rng.integers(1, 1001, k).astype(np.int64)


@pytest.mark.parametrize("path", ["grid", "lds"])
def test_fork_after_add_arcs_across_a_padding_boundary(gpu_engine_module, path):
    n, m, kw = (512, 4090, dict(GRID, **PIN)) if path == "grid" else (64, 1000, dict(PIN))
    inst = netgen(n, m)
    extra = _extra_arcs(inst, 60, 4)          # m crosses a multiple of 1 024: every arc array is reallocated
    assert (m + 1023) // 1024 < (m + 60 + 1023) // 1024
    grown = generators.ArcSoA(inst.n, np.concatenate([inst.tail, extra[0]]), np.concatenate([inst.head, extra[1]]),
                              np.concatenate([inst.cost, extra[2]]), np.concatenate([inst.cap, extra[3]]), inst.supply, "grown")

    def grow(a, b, _inst):
        for h in (a, b):
            h.solve(max_pivots=41)
            h.add_arcs(*extra)
        return grown
    twin_continuation(gpu_engine_module, inst, DANTZIG, kw, first_leg(n, m, 1, DANTZIG), before_fork=grow)


def test_fork_after_an_update_rhs_that_rewrote_the_host_image(gpu_engine_module):
    e = gpu_engine_module
    inst = netgen(512, 4096)
    kw = dict(GRID, **PIN)
    with make(e, inst, DANTZIG, **kw) as a, make(e, inst, DANTZIG, **kw) as b:
        cap = None
        for h in (a, b):
            h.solve()
            r, tree = h.result(), h.tree()
            arc = int(np.nonzero((tree["state"] == 0) & (r.flow > 1))[0][0])
            rep = h.update_rhs(arcs=[arc], caps=[int(r.flow[arc]) // 2])
            assert rep["path"] == 1, rep
            cap = h.cap
        ia = introspect(a)
        forks = a.fork(2)
        try:
            for f in forks:
                assert_same(ia, introspect(f), "after the fork")
            a.close()
            forks[0].solve(); b.solve()
            i0, ib = introspect(forks[0]), introspect(b)
            assert_same(ib, i0, "fork against the control at the end")
            edited = generators.ArcSoA(inst.n, inst.tail, inst.head, inst.cost, cap, inst.supply, "edited")
            assert i0["status"] == "optimal" and i0["objective"] == int(round(oracle.solve_soa(edited, "dantzig")["objective"]))
            forks[1].reset(); forks[1].solve()       # the fork's own host image is whole: a cold start from it reaches the optimum
            assert forks[1].result().objective == i0["objective"]
        finally:
            for f in forks:
                f.close()


# ------------------------------------------------------------------ copy geometry on the device

def _fork_and_finish(e, inst, rule, kw, count, budget):
    with make(e, inst, rule, **kw) as a, make(e, inst, rule, **kw) as b:
        a.solve(max_pivots=budget); b.solve(max_pivots=budget)
        ia = introspect(a)
        rep = {}
        forks = a.fork(count, report=rep)
        try:
            assert len(forks) == count and rep["count"] == count
            for i, f in enumerate(forks):
                assert_same(ia, introspect(f), f"fork {i} of {count}")
            forks[-1].solve(); b.solve()
            assert_same(introspect(b), introspect(forks[-1]), "last fork against the control at the end")
            assert forks[-1].certify()["verdict"] == "optimal"
        finally:
            for f in forks:
                f.close()
        return rep


@pytest.mark.parametrize("n", [64, 65, 66, 67])
def test_node_arrays_that_are_no_multiple_of_16_bytes(gpu_engine_module, n):
    rep = _fork_and_finish(gpu_engine_module, netgen(n, 8 * n), DEVEX, dict(GRID, **PIN), 2, 37)
    assert rep["segments"] >= 20


@pytest.mark.parametrize("count", [1, 2, 70])
def test_fork_counts_on_a_tiny_instance(gpu_engine_module, count):
    _fork_and_finish(gpu_engine_module, netgen(12, 40), CANDIDATE, dict(PIN), count, 5)


def test_fork_of_a_larger_grid_handle(gpu_engine_module):
    rep = _fork_and_finish(gpu_engine_module, netgen(5000, 40000), CANDIDATE, dict(GRID, **PIN), 3, 1009)
    assert rep["bytes_per_fork"] > 40000 * 30


# ------------------------------------------------------------------ mcf_restore

def test_restore_brings_edited_forks_back(gpu_engine_module):
    e = gpu_engine_module
    inst = netgen(512, 4096)
    kw = dict(GRID, **PIN)
    k = first_leg(512, 4096, 1, CANDIDATE)
    with make(e, inst, CANDIDATE, **kw) as a, make(e, inst, CANDIDATE, **kw) as b:
        a.solve(max_pivots=k); b.solve(max_pivots=k)
        ia = introspect(a)
        forks = a.fork(2)
        try:
            arcs = np.arange(0, inst.m, 5)
            forks[0].update_costs(arcs, inst.cost[arcs] * 2); forks[0].solve()
            forks[1].solve(max_pivots=100)
            forks[1].update_rhs(arcs=[3, 4], caps=[1, 2]); forks[1].solve()
            assert introspect(forks[0])["objective"] != introspect(forks[1])["objective"]
            rep = e.restore(forks, a)
            assert rep["count"] == 2 and rep["bytes_per_fork"] > 0
            for f in forks:
                assert_same(ia, introspect(f), "after the restore")
                assert np.array_equal(f.cost, inst.cost) and np.array_equal(f.cap, inst.cap)
            assert_same(ia, introspect(a), "the source after the restore")
            forks[0].solve(); forks[1].solve(max_pivots=k); forks[1].solve(); b.solve()
            ib = introspect(b)
            assert_same(ib, introspect(forks[0]), "restored fork 0 against the control")
            i1 = introspect(forks[1])
            assert all(i1["stats"][c] == ib["stats"][c] for c in COUNTERS) and np.array_equal(i1["flow"], ib["flow"])
            assert np.array_equal(i1["tree"]["order"], ib["tree"]["order"])
        finally:
            for f in forks:
                f.close()


def test_restore_refuses_another_shape_and_bad_lists(gpu_engine_module):
    e = gpu_engine_module
    inst = netgen(512, 4096)
    kw = dict(GRID, **PIN)
    other_m = netgen(512, 4000)
    with make(e, inst, DANTZIG, **kw) as a:
        a.solve(max_pivots=101)
        ia = introspect(a)
        others = {"m": make(e, other_m, DANTZIG, **kw), "rule": make(e, inst, CANDIDATE, **kw),
                  "tree layout": make(e, inst, DANTZIG, tree_blocks=3, **kw)}
        fork = a.fork(1)[0]
        try:
            for what, o in others.items():
                o.solve(max_pivots=53)
                before = introspect(o)
                with pytest.raises(e.EngineError) as err:
                    e.restore([fork, o], a)
                assert err.value.code == -6 and what in str(err.value), (what, str(err.value))
                assert_same(before, introspect(o), f"the refused handle ({what})")
                assert_same(ia, introspect(fork), "the handle listed beside the refused one")
            for bad in ([a], [fork, fork]):
                with pytest.raises(e.EngineError) as err:
                    e.restore(bad, a)
                assert err.value.code == -1
            assert_same(ia, introspect(a), "the source")
        finally:
            fork.close()
            for o in others.values():
                o.close()


# ------------------------------------------------------------------ errors

def test_errors(gpu_engine_module):
    e = gpu_engine_module
    lib = e.load_library()
    inst = netgen(64, 512)
    out = (ctypes.c_void_p * 2)()
    with make(e, inst, DANTZIG) as a:
        a.solve()
        ia = introspect(a)
        assert lib.mcf_fork(None, 1, out, None) == -1
        assert lib.mcf_fork(a._h, 1, None, None) == -1
        assert lib.mcf_fork(a._h, -1, out, None) == -1
        assert lib.mcf_fork(a._h, 0, out, None) == 0 and out[0] is None
        assert a.fork(0) == []
        assert lib.mcf_restore(None, 1, a._h, None) == -1
        assert lib.mcf_restore(out, 1, a._h, None) == -1          # a null entry
        assert lib.mcf_restore(out, -1, a._h, None) == -1
        assert lib.mcf_restore(out, 0, a._h, None) == 0
        assert_same(ia, introspect(a), "the source after the refused calls")
    with make(e, inst, DANTZIG, shard=(0, 2), fused=False) as s:
        with pytest.raises(e.EngineError) as err:
            s.fork(1)
        assert err.value.code == -6 and "shard_count" in str(err.value)


# ------------------------------------------------------------------ scenarios

def _find_cycle(n, tail, head):
    """Arc indices of one directed cycle (depth-first search; path holds (arc into the node, node) below the root)."""
    out = [[] for _ in range(n)]
    for a, (t, h) in enumerate(zip(tail, head)):
        out[int(t)].append((a, int(h)))
    color, path = [0] * n, []

    def visit(u):
        color[u] = 1
        for a, v in out[u]:
            if color[v] == 1:                      # v is on the path: the arcs from v down to u, and a
                cyc = [a]
                for pa, pu in reversed(path):
                    if pu == v:
                        break
                    cyc.append(pa)
                return cyc
            if color[v] == 0:
                path.append((a, v))
                r = visit(v)
                if r is not None:
                    return r
                path.pop()
        color[u] = 2
        return None
    for s in range(n):
        if color[s] == 0:
            r = visit(s)
            if r is not None:
                return r
    raise AssertionError("no directed cycle")


def _cycle_arcs(n, tail, head):
    cyc = _find_cycle(n, tail, head)
    # the arcs found close a walk back to the node where the search met a grey node: check it is a cycle
    nodes_out = sorted(int(tail[a]) for a in cyc)
    nodes_in = sorted(int(head[a]) for a in cyc)
    assert nodes_out == nodes_in and len(set(nodes_out)) == len(cyc)
    return np.asarray(sorted(cyc))


def _scenario_arrays(inst, base_solver, count):
    """``count`` scenarios as (cost, cap, supply) arrays plus the edits in index form: mixed cost, supply and capacity
    edits, one empty, one inside the cost ranges (no pivot), one infeasible and one unbounded by construction."""
    rng = np.random.default_rng(17)
    down, up, _ = base_solver.engine.cost_ranges()
    src = int(np.argmax(inst.supply))
    cyc = _cycle_arcs(inst.n, inst.tail, inst.head)
    quiet = int(np.nonzero((up > 1) & (up < eng_mod.RANGE_INF))[0][0])
    out = []
    for k in range(count):
        cost, cap, supply = inst.cost.copy(), inst.cap.copy(), inst.supply.copy()
        sc = {}
        if k == 0:
            pass
        elif k == 1:                                   # inside the range: the basis stays optimal
            cost[quiet] += 1
            sc["costs"] = (np.array([quiet]), np.array([cost[quiet]]))
        elif k == 2:                                   # nothing can leave the largest source
            arcs = np.nonzero(inst.tail == src)[0]
            cap[arcs] = 0
            sc["capacities"] = (arcs, np.zeros(arcs.size, np.int64))
        elif k == 3:                                   # a negative cycle without capacities
            cost[cyc] = -7; cap[cyc] = -1
            sc["costs"] = (cyc, cost[cyc]); sc["capacities"] = (cyc, cap[cyc])
        else:
            if k % 3 != 2:
                arcs = rng.choice(inst.m, 6, replace=False)
                cost[arcs] = rng.integers(1, 20001, 6)
                sc["costs"] = (arcs, cost[arcs])
            if k % 3 != 0:
                u, w = rng.choice(inst.n, 2, replace=False)
                d = int(rng.integers(1, 40))
                supply[u] += d; supply[w] -= d
                sc["supplies"] = (np.array([u, w]), np.array([supply[u], supply[w]]))
            if k % 2:
                arcs = rng.choice(inst.m, 4, replace=False)
                cap[arcs] = rng.integers(0, 600, 4)
                sc["capacities"] = (arcs, cap[arcs])
        out.append((sc, cost, cap, supply))
    return out


def _cold(problem):
    try:
        r = solve_min_cost_flow(problem)
        return r.status, r.objective
    except UnboundedProblemError:
        return "unbounded", None


def _got(r):
    return ("unbounded", None) if isinstance(r, UnboundedProblemError) else (r.status, r.objective)


def test_scenarios_on_an_soa_problem(gpu_engine_module):
    inst = netgen(64, 512, 3)
    problem = SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply)
    solver = NetworkSimplex(problem)
    try:
        base = solver.solve()
        assert base.status == "optimal"
        cert_before = _exact(solver.engine.certify())
        cases = _scenario_arrays(inst, solver, 40)
        results = solve_scenarios(solver, [c[0] for c in cases], return_exceptions=True)
        assert len(results) == 40
        seen = set()
        for k, ((sc, cost, cap, supply), r) in enumerate(zip(cases, results)):
            edited = SoAProblem(inst.n, inst.tail, inst.head, cost, cap, supply)
            got = _got(r)
            assert got == _cold(edited), (k, sc.keys())
            ref = oracle.solve_soa(generators.ArcSoA(inst.n, inst.tail, inst.head, cost, cap, supply, f"s{k}"), "dantzig")
            assert got[0] == ref["status"], k
            if got[0] == "optimal":
                assert got[1] == float(int(round(ref["objective"]))), k
            seen.add(got[0])
        assert seen == {"optimal", "infeasible", "unbounded"}
        assert results[0].iterations == 0 and results[0].objective == base.objective       # the empty scenario
        assert results[1].iterations == 0 and results[1].status == "optimal"               # inside the ranges: no pivot
        assert any(r.iterations > 0 for r in results if not isinstance(r, Exception))
        with pytest.raises(UnboundedProblemError):
            solve_scenarios(solver, [cases[3][0]])
        with pytest.raises(InvalidProblemError):
            solve_scenarios(solver, [cases[4][0], {"arcs": ()}])
        assert _exact(solver.engine.certify()) == cert_before
        again = solver.solve()
        assert again.status == "optimal" and again.iterations == 0 and again.objective == base.objective
    finally:
        solver.engine.close()


def test_scenarios_on_an_object_model_problem(gpu_engine_module):
    inst = netgen(12, 40, 2)
    keys, keep = {}, []
    for a, (t, h) in enumerate(zip(inst.tail.tolist(), inst.head.tolist())):
        if (t, h) not in keys:
            keys[(t, h)] = a
            keep.append(a)
    keep = np.asarray(keep)
    name = [f"v{i:02d}" for i in range(inst.n)]
    key_of = [(name[int(inst.tail[a])], name[int(inst.head[a])]) for a in keep]

    def problem_of(cost, cap, supply):
        nodes = [{"id": name[i], "supply": float(supply[i])} for i in range(inst.n)]
        arcs = [{"tail": key_of[j][0], "head": key_of[j][1], "cost": float(cost[j]), "capacity": None if cap[j] < 0 else float(cap[j])}
                for j in range(len(keep))]
        return build_problem(nodes, arcs, directed=True, tolerance=1e-6)
    cost0, cap0, supply0 = inst.cost[keep].astype(np.int64), inst.cap[keep].astype(np.int64), inst.supply.astype(np.int64)
    sub = generators.ArcSoA(inst.n, inst.tail[keep], inst.head[keep], cost0, cap0, supply0, "object")
    solver = NetworkSimplex(problem_of(cost0, cap0, supply0), options=SolverOptions(pricing_strategy="dantzig"))
    try:
        base = solver.solve()
        assert base.status == "optimal"
        # the engine's arc order is the solver's (sorted by key): ranges are asked by key
        cases = _scenario_arrays(sub, _ByKey(solver, key_of), 40)
        scenarios = []
        for sc, _, _, _ in cases:
            named = {}
            if "costs" in sc:
                named["costs"] = {key_of[int(a)]: float(c) for a, c in zip(*sc["costs"])}
            if "supplies" in sc:
                named["supplies"] = {name[int(v)]: float(s) for v, s in zip(*sc["supplies"])}
            if "capacities" in sc:
                named["capacities"] = {key_of[int(a)]: (None if c < 0 else float(c)) for a, c in zip(*sc["capacities"])}
            scenarios.append(named)
        results = solve_scenarios(solver, scenarios, return_exceptions=True)
        seen = set()
        for k, ((sc, cost, cap, supply), r) in enumerate(zip(cases, results)):
            got = _got(r)
            assert got == _cold(problem_of(cost, cap, supply)), (k, sc.keys())
            seen.add(got[0])
        assert seen == {"optimal", "infeasible", "unbounded"}
        assert results[0].iterations == 0 and results[0].objective == base.objective
        assert results[1].iterations == 0 and results[1].status == "optimal"
        again = solver.solve()
        assert again.status == "optimal" and again.iterations == 0 and again.objective == base.objective
    finally:
        solver.engine.close()


class _ByKey:
    """cost_ranges of an object-model solver in the order of a key list, behind the two attributes _scenario_arrays reads."""

    def __init__(self, solver, key_of):
        self.engine = self
        flat = solver.flat
        index = {k: i for i, k in enumerate(flat.keys)}
        self._perm = np.asarray([index[k] for k in key_of])
        self._solver = solver

    def cost_ranges(self):
        down, up, rep = self._solver.engine.cost_ranges()
        return down[self._perm], up[self._perm], rep
