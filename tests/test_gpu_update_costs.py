"""Re-optimising after arc cost changes on the resident handle (``mcf_update_costs``, ``-m gpu``).

Everything goes through the C ABI (``engine.McfEngine`` is the ctypes binding).  The device state right after the call is
checked against numpy -- potentials along the tree, reduced costs, key codes -- and the re-solve against a fresh handle
that was created with the new costs and solved cold.  Every comparison is exact."""

import time

import numpy as np
import pytest

import network_flow_solver_amd as nfs
import random_instances
import wide_range_instances as wri
from conftest import check_optimality, check_tree_invariants, optimum_is_unique
from network_flow_solver_amd import generators
from network_flow_solver_amd.data import SoAProblem
from network_flow_solver_amd.generators import ArcSoA

pytestmark = pytest.mark.gpu

RULE_IDS = {0: "dantzig", 1: "devex_block", 2: "candidate_list"}
# engine path: options, rules, stats()["pricing_mode"], nodes / arcs of the netgen-style instance
PATHS = {
    "small": (dict(), (0, 1, 2), 2, (200, 1500)),                                                  # k_solve_small (LDS)
    "mid": (dict(fused=False, mid_loop=1), (0, 1, 2), 3, (700, 6000)),                             # k_solve_mid
    "grid_dense": (dict(fused=False, mid_loop=-1, tree_blocks=-1), (0, 1, 2), 1, (1500, 12000)),   # three kernels per pivot
    "grid_blocked_4": (dict(tree_blocks=4), (0, 1, 2), 1, (1500, 12000)),                          # blocked preorder list
    "grid_blocked_7": (dict(tree_blocks=7), (0, 1, 2), 1, (1500, 12000)),
    "key_codes": (dict(fused=False, mid_loop=-1, compressed_keys=1), (0, 2), 1, (1500, 12000)),    # k_price_v
    "gather": (dict(fused=False, mid_loop=-1, resident_rc=False), (0, 2), 0, (700, 6000)),         # k_price
}
PATH_CASES = [(p, r) for p, (_, rules, _, _) in PATHS.items() for r in rules]
PATH_IDS = [f"{p}-{RULE_IDS[r]}" for p, r in PATH_CASES]
TREE_KEYS = ("parent", "pred_arc", "size", "pos", "order", "depth", "psize", "state")


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _with_costs(inst, cost):
    return ArcSoA(inst.n, inst.tail, inst.head, np.asarray(cost, np.int64), inst.cap, inst.supply, inst.name + "_recosted")


def _perturb(inst, cost, seed, share=0.05, span=0.10):
    """`share` of the arcs, each cost moved by up to +-`span` of itself (at least +-1): (indices, new costs)."""
    rng = np.random.default_rng([77, seed, inst.m])
    k = max(1, int(inst.m * share))
    idx = rng.choice(inst.m, k, replace=False).astype(np.int64)
    width = np.maximum(1, (np.abs(cost[idx]) * span).astype(np.int64))
    return idx, cost[idx] + rng.integers(-width, width + 1)


def _fresh(e, inst, rule, kw):
    with _engine(e, inst, rule, **kw) as eng:
        eng.solve()
        return eng.result()


def _tree_potentials(inst, cost, tree, big_m):
    """Potentials the tree implies under `cost`, from parent / pred_arc alone (numpy; root potential as given)."""
    n = inst.n
    pi = np.zeros(n + 1, dtype=np.int64)
    pi[n] = tree["pi"][n]
    for v in tree["order"][1:].tolist():           # preorder: a parent comes before its children
        p, a = int(tree["parent"][v]), int(tree["pred_arc"][v])
        if a >= inst.m:                            # artificial arc of node v: the direction is not part of the introspection
            d = int(tree["pi"][v] - tree["pi"][p])
            assert abs(d) == big_m, (v, d, big_m)
            pi[v] = pi[p] + d
        else:
            c = int(cost[a])
            pi[v] = pi[p] - c if inst.tail[a] == v else pi[p] + c
            assert {int(inst.tail[a]), int(inst.head[a])} == {v, p}
    return pi


def _check_state(eng, inst, cost, big_m, before, resident_before, half=1 << 28):
    """The handle right after mcf_update_costs: flows / states / tree untouched, potentials follow the new costs along
    the tree, reduced costs and key codes exact."""
    res, tree = eng.result(), eng.tree()
    assert np.array_equal(res.flow, before["res"].flow) and np.array_equal(res.in_tree, before["res"].in_tree)
    for k in TREE_KEYS:
        assert np.array_equal(tree[k], before["tree"][k]), k
    assert tree["pi"][inst.n] == before["tree"]["pi"][inst.n]
    check_tree_invariants(inst.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
    want_pi = _tree_potentials(inst, cost, tree, big_m)
    assert np.array_equal(tree["pi"], want_pi)
    rc, resident = eng.reduced_costs()
    assert resident == resident_before
    want_rc = cost + tree["pi"][inst.tail] - tree["pi"][inst.head]
    assert np.array_equal(rc, want_rc)
    assert not rc[tree["state"] == 0].any()
    keys, present = eng.pricing_keys()
    if present:
        viol = (-tree["state"].astype(np.int64) * want_rc).tolist()
        assert keys.tolist() == [wri.vkey_int(v, big_m, half) for v in viol]
    return res, tree


def _snapshot(eng):
    return {"res": eng.result(), "tree": eng.tree()}


def _same_optimum(inst_new, got, want):
    assert got.status == want.status == "optimal"
    assert got.objective == want.objective
    rc = check_optimality(inst_new, got.flow, got.potential)
    if optimum_is_unique(inst_new, got.flow, got.in_tree, rc):
        assert np.array_equal(got.flow, want.flow)


# ------------------------------------------------------------------ every path: state after the call, re-solve, chain
@pytest.mark.parametrize("path,rule", PATH_CASES, ids=PATH_IDS)
def test_state_after_the_call_and_resolve_on_every_path(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, mode, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=11)
    big_m = wri.big_m_of(inst.n, int(np.abs(inst.cost).max()))
    for start in ("solved", "mid_solve"):
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve(-1 if start == "solved" else 150)
            before = _snapshot(eng)
            assert before["res"].stats["pricing_mode"] == mode
            assert before["res"].status == ("optimal" if start == "solved" else "iteration_limit")
            if path.startswith("grid_blocked"):
                assert before["res"].stats["tree_blocks"] == int(path[-1])
            resident = eng.reduced_costs()[1]
            cost = inst.cost.copy()
            pivots = before["res"].stats["pivots"]
            for step in range(5 if start == "solved" else 1):      # a chain of successive updates on one handle
                idx, new = _perturb(inst, cost, step)
                new = np.clip(new, 1, int(inst.cost.max()))          # (big-M stays as created; its growth has a test of its own)
                eng.update_costs(idx, new)
                cost[idx] = new
                _check_state(eng, inst, cost, big_m, before, resident)
                eng.solve()
                got = eng.result()
                assert got.stats["pivots"] >= pivots                 # cumulative
                pivots = got.stats["pivots"]
                recosted = _with_costs(inst, cost)
                _same_optimum(recosted, got, _fresh(e, recosted, rule, kw))
                before = _snapshot(eng)
                assert eng.reduced_costs()[1] == resident


def test_level_coded_keys_and_wide_costs(gpu_engine_module):
    """Key codes in their level-coded form (big-M >= 2^29) and with a narrow half width, on the wide-range family."""
    e = gpu_engine_module
    inst = wri.make(0, *wri.SIZES["medium"])
    big_m = wri.big_m_of(inst.n, int(np.abs(inst.cost).max()))
    assert big_m >= 1 << 29
    for half_log2 in (0, 12):
        kw = dict(fused=False, mid_loop=-1, compressed_keys=1, vkey_half_log2=half_log2)
        for budget in (300, -1):
            with _engine(e, inst, 0, **kw) as eng:
                eng.solve(budget)
                before = _snapshot(eng)
                cost = inst.cost.copy()
                idx, new = _perturb(inst, cost, 5, share=0.2, span=0.5)
                new = np.clip(new, -wri.cmax_for(inst.n), wri.cmax_for(inst.n))
                eng.update_costs(idx, new)
                cost[idx] = new
                assert eng.pricing_keys()[1]
                _check_state(eng, inst, cost, big_m, before, True, half=1 << (half_log2 or 28))
                eng.solve()
                got = eng.result()
            recosted = _with_costs(inst, cost)
            want = _fresh(e, recosted, 0, kw)
            assert (got.status, got.objective) == (want.status, want.objective) and got.status == "optimal"
            assert wri.exact_certificate(recosted, got.flow, got.potential) == got.objective


# ------------------------------------------------------------------ provable zero-pivot cases
@pytest.mark.parametrize("rule", (0, 1, 2), ids=list(RULE_IDS.values()))
@pytest.mark.parametrize("path", ("small", "grid_dense", "grid_blocked_4"))
def test_changes_that_keep_the_basis_optimal_cost_no_pivot(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=12)
    with _engine(e, inst, rule, **kw) as eng:
        eng.solve()
        r0 = eng.result()
        assert r0.status == "optimal"
        eng.update_costs([], [])                                          # count = 0
        eng.solve()
        assert eng.result().stats["pivots"] == r0.stats["pivots"]
        eng.update_costs(np.arange(inst.m), inst.cost)                    # the identical costs
        eng.solve()
        r1 = eng.result()
        assert r1.stats["pivots"] == r0.stats["pivots"] and r1.objective == r0.objective and r1.status == "optimal"
        # dearer where nothing flows, cheaper where the arc is full: every reduced cost keeps its sign
        state = eng.tree()["state"]
        cost = inst.cost.copy()
        rng = np.random.default_rng(3)
        lower = np.nonzero(state == 1)[0]
        upper = np.nonzero(state == -1)[0]
        lower = rng.choice(lower, max(1, lower.size // 3), replace=False)
        cost[lower] = np.minimum(cost[lower] + rng.integers(1, 500, lower.size), inst.cost.max())   # (big-M as created)
        if upper.size:
            cost[upper] -= rng.integers(1, 500, upper.size)
        idx = np.concatenate((lower, upper))
        eng.update_costs(idx, cost[idx])
        eng.solve()
        r2 = eng.result()
        assert r2.stats["pivots"] == r0.stats["pivots"] and r2.status == "optimal"
        assert np.array_equal(r2.flow, r0.flow) and np.array_equal(r2.potential, r0.potential)
    recosted = _with_costs(inst, cost)
    assert r2.objective == _fresh(e, recosted, rule, kw).objective
    check_optimality(recosted, r2.flow, r2.potential)


# ------------------------------------------------------------------ basic arcs: potentials move below them, nowhere else
@pytest.mark.parametrize("path", ("small", "mid", "grid_dense", "grid_blocked_4"))
def test_basic_arc_changes_shift_exactly_the_subtrees_below(gpu_engine_module, path):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=13)
    with _engine(e, inst, 2, **kw) as eng:
        eng.solve()
        tree = eng.tree()
        basic = np.nonzero(tree["state"] == 0)[0]
        rng = np.random.default_rng(4)
        picked = rng.choice(basic, min(12, basic.size), replace=False)
        delta = rng.integers(-300, 301, picked.size)
        delta[delta == 0] = 7
        eng.update_costs(picked, inst.cost[picked] + delta)
        after = eng.tree()
    pos, size = tree["pos"], tree["size"]
    want = np.zeros(inst.n + 1, dtype=np.int64)
    for a, d in zip(picked.tolist(), delta.tolist()):
        t, h = int(inst.tail[a]), int(inst.head[a])
        x = t if tree["pred_arc"][t] == a and tree["parent"][t] == h else h   # the end point the arc is the tree arc of
        assert tree["pred_arc"][x] == a
        below = (pos >= pos[x]) & (pos < pos[x] + size[x])                    # x's subtree: a preorder interval
        want[below] += -d if x == t else d
    assert np.array_equal(after["pi"] - tree["pi"], want)
    assert (want != 0).any() and (want == 0).any()


# ------------------------------------------------------------------ big-M
@pytest.mark.parametrize("path,rule", [("small", 0), ("mid", 1), ("grid_dense", 2), ("grid_blocked_4", 2), ("key_codes", 0)])
def test_a_cost_above_the_create_time_maximum_raises_big_m(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=14)
    old_big_m = wri.big_m_of(inst.n, int(np.abs(inst.cost).max()))
    huge = 1 << 30 if path != "key_codes" else 3_000_000     # key_codes: from the plain code range (big-M < 2^29) into the level-coded one
    new_big_m = wri.big_m_of(inst.n, huge)
    assert old_big_m < new_big_m < wri.BIG_M_LIMIT
    for budget in (40, -1):                                  # 40 pivots: most nodes still hang on their artificial arc
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve(budget)
            before = _snapshot(eng)
            resident = eng.reduced_costs()[1]
            cost = inst.cost.copy()
            idx = np.array([5, inst.m // 2, 5], dtype=np.int64)
            new = np.array([17, -huge, huge], dtype=np.int64)   # arc 5 is named twice: the last entry wins
            eng.update_costs(idx, new)
            cost[idx] = new
            assert cost[5] == huge
            _check_state(eng, inst, cost, new_big_m, before, resident)
            eng.solve()
            got = eng.result()
            # big-M never shrinks: back to small costs, the artificial arcs keep the larger one
            eng.update_costs(idx, inst.cost[idx])
            t = eng.tree()
            art = t["pred_arc"] >= inst.m
            assert (np.abs(t["pi"] - t["pi"][np.maximum(t["parent"], 0)])[art] == new_big_m).all()
        recosted = _with_costs(inst, cost)
        _same_optimum(recosted, got, _fresh(e, recosted, rule, kw))


def test_inadmissible_costs_are_refused_and_leave_the_handle_alone(gpu_engine_module):
    e = gpu_engine_module
    inst = wri.make(0, 16384, 65536)                         # n large enough for big-M to bind below INT32_MAX
    kw = dict(fused=False, mid_loop=-1)
    assert wri.cmax_for(inst.n) < wri.INT32_MAX
    want = _fresh(e, inst, 0, kw)
    with _engine(e, inst, 0, **kw) as eng:
        eng.solve(200)
        before = _snapshot(eng)
        rc_before = eng.reduced_costs()[0]
        too_big = (wri.BIG_M_LIMIT + inst.n + 1) // (inst.n + 2)        # (too_big + 1)(n + 2) >= 2^44
        assert too_big <= wri.INT32_MAX and wri.big_m_of(inst.n, too_big) >= wri.BIG_M_LIMIT
        for idx, new in (([3], [too_big]), ([3], [-(1 << 31)]), ([0, 3], [1, 1 << 31])):
            with pytest.raises(e.EngineError) as err:
                eng.update_costs(idx, new)
            assert err.value.code == -5                                   # MCF_E_RANGE
        for idx, new in (([-1], [1]), ([inst.m], [1]), ([0, inst.m], [1, 1])):
            with pytest.raises(e.EngineError) as err:
                eng.update_costs(idx, new)
            assert err.value.code == -1                                   # MCF_E_BAD_ARG
        lib = eng._lib
        assert lib.mcf_update_costs(None, 0, None, None) == -1
        assert lib.mcf_update_costs(eng._h, -1, None, None) == -1
        assert lib.mcf_update_costs(eng._h, 2, None, None) == -1
        after = _snapshot(eng)
        assert np.array_equal(after["res"].flow, before["res"].flow) and after["res"].status == before["res"].status
        for k in TREE_KEYS + ("pi",):
            assert np.array_equal(after["tree"][k], before["tree"][k]), k
        assert np.array_equal(eng.reduced_costs()[0], rc_before)
        eng.solve()
        got = eng.result()
    assert (got.status, got.objective, got.stats["pivots"]) == (want.status, want.objective, want.stats["pivots"])
    assert np.array_equal(got.flow, want.flow)


def test_sharded_handles_refuse(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(700, 6000, seed=15)
    with _engine(e, inst, 0, shard=(0, 2)) as eng:
        with pytest.raises(e.EngineError) as err:
            eng.update_costs([0], [1])
        assert err.value.code == -6                                       # MCF_E_STATE


# ------------------------------------------------------------------ host image
@pytest.mark.parametrize("path", ("small", "grid_dense", "grid_blocked_4"))
def test_reset_and_set_basis_see_the_new_costs(gpu_engine_module, path):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=16)
    with _engine(e, inst, 2, **kw) as eng:
        eng.solve()
        old = eng.result()
        cost = inst.cost.copy()
        idx, new = _perturb(inst, cost, 9, share=0.1, span=0.3)
        new[0] = 2_000_000                                                # ... and a larger big-M
        eng.update_costs(idx, new)
        cost[idx] = new
        recosted = _with_costs(inst, cost)
        want = _fresh(e, recosted, 2, kw)
        eng.reset()
        eng.solve()
        cold = eng.result()
        assert (cold.status, cold.objective, cold.stats["pivots"]) == (want.status, want.objective, want.stats["pivots"])
        assert np.array_equal(cold.flow, want.flow) and np.array_equal(cold.potential, want.potential)
        at_upper = ~old.in_tree & (inst.cap > 0) & (old.flow == inst.cap)
        assert eng.set_basis(old.in_tree.astype(np.int8), at_upper.astype(np.int8)), eng.last_error()
        eng.solve()
        warm = eng.result()
        _same_optimum(recosted, warm, want)


# ------------------------------------------------------------------ scale: the auto-selected blocked layout
def test_a_quarter_million_nodes_on_the_auto_selected_blocked_list(gpu_engine_module, capsys):
    """262 144 nodes / 2 M arcs (above the 200 000-node threshold of the blocked preorder list), candidate list: solve,
    perturb 1 % of the costs by up to +-10 %, re-solve, certify.  Prints its own wall time: 17.5 s on an MI355X (cold solve
    762 558 pivots, 17.1 s with the generator; update call 5.0 ms for 20 971 arcs; re-solve 6 838 pivots in 0.23 s) -- the
    existing million-node test takes 104 s."""
    e = gpu_engine_module
    t0 = time.time()
    inst = generators.netgen_style(1 << 18, 1 << 21, seed=1)
    with _engine(e, inst, 2) as eng:
        eng.solve()
        first = eng.result()
        assert first.status == "optimal" and first.stats["tree_blocks"] > 0
        t1 = time.time()
        cost = inst.cost.copy()
        idx, new = _perturb(inst, cost, 1, share=0.01, span=0.10)
        before_pi = eng.tree()["pi"]
        tu = time.time()
        eng.update_costs(idx, new)
        tu = time.time() - tu
        cost[idx] = new
        tree = eng.tree()
        rc, _ = eng.reduced_costs()
        assert np.array_equal(rc, cost + tree["pi"][inst.tail] - tree["pi"][inst.head]) and not rc[tree["state"] == 0].any()
        assert (tree["pi"] != before_pi).any()
        t2 = time.time()
        eng.solve()
        got = eng.result()
        t3 = time.time()
    assert got.status == "optimal"
    recosted = _with_costs(inst, cost)
    check_optimality(recosted, got.flow, got.potential)
    assert got.objective == int(np.dot(got.flow, cost))      # (< 2^45: exact in int64)
    extra = got.stats["pivots"] - first.stats["pivots"]
    assert 0 < extra < first.stats["pivots"]
    with capsys.disabled():
        print(f"\n  [update_costs 262144 / 2097152] cold solve {first.stats['pivots']} pivots {t1 - t0:.1f} s (with generation), "
              f"update {tu * 1e3:.2f} ms for {idx.size} arcs, re-solve {extra} pivots {t3 - t2:.2f} s, test {time.time() - t0:.1f} s", flush=True)


# ------------------------------------------------------------------ the shim
def _object_problem(options):
    """A seeded object-model instance: directed, with parallel arcs, quarter-unit costs (cost scale 100), optimal."""
    from network_flow_solver_amd.simplex import flatten_problem

    for seed in range(400):
        nodes, arcs, directed = random_instances.make(seed)
        if not directed or len(arcs) < 8 or len({(a["tail"], a["head"]) for a in arcs}) == len(arcs):
            continue
        problem = nfs.build_problem(nodes, arcs, True, 1e-6)
        if flatten_problem(problem).cost_scale != 100:
            continue
        solver = nfs.NetworkSimplex(problem, options)
        first = solver.solve()
        if first.status == "optimal" and first.iterations > 0:
            return nodes, arcs, problem, solver, first
    raise AssertionError("no suitable instance among the seeds")


def test_shim_update_costs_on_an_object_problem(gpu_engine_module):
    import copy

    options = nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True)
    nodes, arcs, problem, solver, first = _object_problem(options)
    untouched = copy.deepcopy(problem)
    keys = sorted({(a["tail"], a["head"]) for a in arcs})
    changes = {keys[0]: 0.5, keys[len(keys) // 2]: 9.25, keys[-1]: -1.0}
    assert solver.update_costs(changes) == len(changes)
    assert problem == untouched and solver.problem is not problem
    second = solver.solve()
    # the same problem built from scratch: last arc of every changed key takes the cost
    new_arcs = [dict(a) for a in arcs]
    for key, c in changes.items():
        last = max(i for i, a in enumerate(new_arcs) if (a["tail"], a["head"]) == key)
        new_arcs[last]["cost"] = c
    fresh_problem = nfs.build_problem(nodes, new_arcs, True, 1e-6)
    assert sorted((a.tail, a.head, a.cost) for a in solver.problem.arcs) == sorted((a.tail, a.head, a.cost) for a in fresh_problem.arcs)
    want = nfs.NetworkSimplex(fresh_problem, nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True)).solve()
    assert second.status == want.status
    assert second.objective == pytest.approx(want.objective, abs=1e-9)   # caller units, whatever the internal scale
    assert second.iterations == solver.stats["pivots"] - first.iterations  # this call's pivots, not the cumulative count
    if second.status == "optimal":
        # duals in caller units: complementary slackness against the caller's costs
        for a in fresh_problem.arcs:
            f = second.flows.get((a.tail, a.head), 0.0)
            if len([b for b in fresh_problem.arcs if (b.tail, b.head) == (a.tail, a.head)]) > 1:
                continue
            rc = a.cost + second.duals[a.tail] - second.duals[a.head]
            if a.lower + 1e-9 < f and (a.capacity is None or f < a.capacity - 1e-9):
                assert abs(rc) < 1e-9
    with pytest.raises(nfs.InvalidProblemError):
        solver.update_costs({keys[0]: 0.123456})                          # off this solver's cost scale: nothing changes
    again = solver.solve()
    assert again.iterations == 0 and again.objective == second.objective


def test_shim_update_costs_on_an_soa_problem(gpu_engine_module):
    inst = generators.netgen_style(700, 6000, seed=17)
    lower = np.zeros(inst.m, np.int64)
    lower[::7] = 1
    soa = SoAProblem(inst.n, inst.tail, inst.head, inst.cost, np.maximum(inst.cap, 2), inst.supply, lower=lower)
    cost0 = soa.cost.copy()
    solver = nfs.NetworkSimplex(soa, nfs.SolverOptions(pricing_strategy="candidate_list", explicit_pricing_strategy=True))
    first = solver.solve()
    assert first.status == "optimal"
    idx, new = _perturb(inst, inst.cost, 21, share=0.05, span=0.2)
    assert solver.update_costs((np.concatenate((idx[:3], idx)), np.concatenate((new[:3] + 5, new)))) == idx.size
    assert np.array_equal(soa.cost, cost0) and solver.problem is not soa
    cost = inst.cost.copy()
    cost[idx] = new
    assert np.array_equal(solver.problem.cost, cost)
    second = solver.solve()
    want = nfs.NetworkSimplex(SoAProblem(inst.n, inst.tail, inst.head, cost, np.maximum(inst.cap, 2), inst.supply, lower=lower),
                              nfs.SolverOptions(pricing_strategy="candidate_list", explicit_pricing_strategy=True)).solve()
    assert (second.status, second.objective) == (want.status, want.objective)
    assert 0 < second.iterations < first.iterations and second.iterations == solver.stats["pivots"] - first.iterations
    flow = np.asarray(second.flows.array, dtype=np.int64)
    assert second.objective == float(np.dot(flow, cost))                 # lower-bound shift included, new costs
    duals = second.duals.array.astype(np.int64)
    rc = cost + duals[inst.tail] - duals[inst.head]
    interior = (flow > lower) & (flow < np.maximum(inst.cap, 2))
    assert not rc[interior].any()
