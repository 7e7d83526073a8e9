"""mcf_certify / mcf_bottlenecks on the device, against numpy and Python-int yardsticks computed from downloaded arrays.

What is compared: every count, every worst value and its index (ties: lowest index), the 128-bit objectives, the
verdict.  Yardsticks: ``planted_trees.np_cert`` (numpy on int64 where the values fit, Python ints for the sums),
``wide_range_instances.exact_certificate`` and ``conftest.check_optimality``.  Nothing here has a tolerance: the call is
exact integer arithmetic.
"""

from __future__ import annotations

import time

import numpy as np
import pytest

import verdict_instances as vi
import wide_range_instances as wri
from conftest import check_optimality, check_tree_invariants
from network_flow_solver_amd import generators
from planted_trees import first_worst as _first_worst, np_cert as _np_cert   # (shared with test_gpu_passes_geometry.py)

pytestmark = pytest.mark.gpu

RULE_IDS = {0: "dantzig", 1: "devex_block", 2: "candidate_list"}
MCF_INF = 1 << 60
# engine path: options, rules, stats()["pricing_mode"], nodes / arcs of the netgen-style instance
PATHS = {
    "small": (dict(), (0, 1, 2), 2, (200, 1500)),                                                  # k_solve_small (LDS)
    "mid": (dict(fused=False, mid_loop=1), (0, 1, 2), 3, (700, 6000)),                             # k_solve_mid
    "grid_dense": (dict(fused=False, mid_loop=-1, tree_blocks=-1), (0, 1, 2), 1, (1500, 12000)),   # three kernels per pivot
    "grid_blocked_2": (dict(tree_blocks=2), (0, 1, 2), 1, (1500, 12000)),                          # blocked list, tiny blocks
    "grid_blocked_7": (dict(tree_blocks=7), (0, 1, 2), 1, (1500, 12000)),
    "key_codes": (dict(fused=False, mid_loop=-1, compressed_keys=1), (0, 2), 1, (1500, 12000)),    # k_price_v
    "incremental": (dict(fused=False, mid_loop=-1, full_sweeps=-1), (0, 2), 1, (1500, 12000)),     # clean workgroups keep candidates
    "gather": (dict(fused=False, mid_loop=-1, resident_rc=False), (0, 2), 0, (700, 6000)),         # k_price
    # reduced costs given up mid-solve: the handle looks once 4 096 pivots have passed, so the instance has to need more than
    # that (the CPU emulation makes 6 591 .. 8 742 pivots on seeds 3 .. 5 at this size under either rule, 3 167 .. 3 386 at 1 500 nodes)
    "rc_drop": (dict(tree_blocks=4, rc_drop=1), (1, 2), None, (3000, 24000)),
}
PATH_CASES = [(p, r) for p, (_, rules, _, _) in PATHS.items() for r in rules]
PATH_IDS = [f"{p}-{RULE_IDS[r]}" for p, r in PATH_CASES]
ZERO_COUNTS = ("negative_flow_count", "over_capacity_count", "imbalance_count", "dual_lower_count", "dual_upper_count")
BASIS_COUNTS = ("basic_count_mismatch", "tree_rc_count", "state_flow_count", "tree_shape_count", "strong_count")


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _assert_matches(cert, want):
    got = {k: cert[k] for k in want}
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def _assert_proven_optimal(cert, inst, res):
    assert cert["verdict"] == "optimal" and cert["proves_status"] and cert["status"] == "optimal", cert
    assert all(cert[k] == 0 for k in ZERO_COUNTS + BASIS_COUNTS), cert
    assert cert["gap"] == 0 and cert["artificial_flow"] == 0 and cert["bigm_term"] == 0
    assert cert["primal"] == cert["dual"] == res.objective == wri.exact_objective(inst, res.flow)
    assert cert["basic_arcs"] == inst.n and cert["rc_mismatch_count"] == 0 and cert["key_mismatch_count"] == 0
    assert cert["checks"] == 63


# ------------------------------------------------------------------ 1. solved handles prove themselves
@pytest.mark.parametrize("path,rule", PATH_CASES, ids=PATH_IDS)
def test_solved_handles_prove_themselves(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, mode, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=3)
    with _engine(e, inst, rule, **kw) as eng:
        eng.solve()
        res = eng.result()
        cert = eng.certify()
        again = eng.certify()
        stats = eng.stats()
    assert res.status == "optimal"
    if mode is not None:
        assert stats["pricing_mode"] == mode
    else:
        assert stats["rc_dropped_at"] > 0 and cert["rc_compared"] == 0      # the handle gave its reduced costs up
    _assert_proven_optimal(cert, inst, res)
    check_optimality(inst, res.flow, res.potential)
    _assert_matches(cert, _np_cert(inst, inst.cost, res.flow, res.potential))
    if mode in (1, 3):
        assert cert["rc_compared"] == inst.m
    if path == "key_codes":
        assert cert["key_compared"] == inst.m
    drop = ("arc_pass_ms", "node_pass_ms")
    assert {k: v for k, v in cert.items() if k not in drop} == {k: v for k, v in again.items() if k not in drop}   # deterministic


@pytest.mark.parametrize("size,kw", [("small", dict()), ("medium", dict(fused=False, mid_loop=-1)), ("medium", dict(tree_blocks=3))],
                         ids=["small", "grid_dense", "grid_blocked"])
@pytest.mark.parametrize("rule", (0, 1, 2), ids=RULE_IDS.values())
def test_wide_range_objectives_beyond_64_bits(gpu_engine_module, size, kw, rule):
    """The wide-range family: negative objectives, and with nonneg=True positive ones beyond 2^63; the chain and edge instances."""
    e = gpu_engine_module
    n, m = wri.SIZES[size]
    cases = [wri.make(1, n, m), wri.make(2, n, m, nonneg=True), wri.make(3, n, m, tie_rich=True), wri.chain_instance()]
    if size == "medium" and rule == 0:
        cases.append(wri.edge_instance())
    for inst in cases:
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve()
            res = eng.result()
            cert = eng.certify()
        assert res.status == "optimal", inst.name
        _assert_proven_optimal(cert, inst, res)
        assert cert["primal"] == wri.exact_certificate(inst, res.flow, res.potential), inst.name
    big = wri.make(2, n, m, nonneg=True)
    with _engine(e, big, rule, **kw) as eng:
        eng.solve()
        assert eng.certify()["primal"] > 1 << 63


@pytest.mark.parametrize("variant", vi.INFEASIBLE_VARIANTS)
@pytest.mark.parametrize("kw", [dict(), dict(fused=False, mid_loop=-1), dict(tree_blocks=3)], ids=["small", "grid_dense", "grid_blocked"])
def test_infeasible_instances_are_proven_infeasible(gpu_engine_module, variant, kw):
    e = gpu_engine_module
    inst = vi.infeasible(5, variant=variant)
    for rule in (0, 1, 2):
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve()
            res = eng.result()
            cert = eng.certify()
        assert res.status == "infeasible"
        assert cert["status"] == "infeasible" and cert["verdict"] == "infeasible" and cert["proves_status"], cert
        assert cert["artificial_flow"] == res.stats["artificial_flow"] > 0
        assert cert["bigm_term"] == cert["big_m"] * cert["artificial_flow"] and cert["big_m"] == vi.big_m(inst)
        assert cert["gap"] == 0 and cert["primal"] == res.objective
        assert all(cert[k] == 0 for k in ZERO_COUNTS + BASIS_COUNTS), cert
        # the caller's flow alone says nothing about artificial arcs: the imbalance is reported as it stands
        alone = eng_free_certify(e, inst, rule, kw, res.flow, res.potential)
        _assert_matches(alone, _np_cert(inst, inst.cost, res.flow, res.potential))
        assert alone["imbalance_count"] > 0 and alone["verdict"] == "not_proven" and alone["artificial_flow"] == 0


def eng_free_certify(e, inst, rule, kw, flow, potential, checks=0):
    """Caller's arrays certified on a FRESH handle (cold start: its own state plays no part)."""
    with _engine(e, inst, rule, **kw) as eng:
        return eng.certify(flow, potential, checks)


# ------------------------------------------------------------------ 2. mid-solve states are reported exactly
@pytest.mark.parametrize("path,rule", PATH_CASES, ids=PATH_IDS)
def test_mid_solve_states_are_reported_exactly(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=4)
    with _engine(e, inst, rule, **kw) as eng:
        for k in (0, 15, 60):
            if k:
                eng.solve(k)
            cert = eng.certify()
            res = eng.result()
            tree = eng.tree()
            rc, _ = eng.reduced_costs()
            priced = eng.price_once(0)
            assert res.status == "iteration_limit" and cert["verdict"] == "not_proven" and not cert["proves_status"]
            assert cert["status"] == ("running" if k == 0 else "iteration_limit")
            pi = tree["pi"][: inst.n] - tree["pi"][inst.n]
            want = _np_cert(inst, inst.cost, res.flow, pi)
            del want["imbalance_count"], want["imbalance_worst"], want["imbalance_worst_node"], want["gap"]
            _assert_matches(cert, want)                                      # (rc of get_reduced_costs == cost + pi[t] - pi[h])
            assert np.array_equal(rc, inst.cost + pi[inst.tail] - pi[inst.head])
            assert cert["imbalance_count"] == 0                              # artificial arcs included: conserved at every pivot
            assert all(cert[c] == 0 for c in BASIS_COUNTS), cert
            assert cert["rc_mismatch_count"] == 0 and cert["key_mismatch_count"] == 0
            assert cert["artificial_flow"] == res.stats["artificial_flow"]
            assert cert["gap"] == cert["primal"] + cert["bigm_term"] - cert["dual"]
            check_tree_invariants(inst.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
            # the plain Dantzig key: the entering arc is the worse of the two classes' worst arcs, ties to the lowest index.
            # (a violation of the upper class on a BASIC arc cannot be entered and does not occur: tree arcs have rc == 0)
            st = tree["state"]
            viol = -st.astype(np.int64) * rc
            assert priced is not None and cert["dual_lower_count"] + cert["dual_upper_count"] > 0
            arc, direction, key = priced
            assert key == int(viol.max()) and arc == int(np.flatnonzero(viol == key)[0])
            fwd = (cert["dual_lower_worst"], -cert["dual_lower_arc"]) if cert["dual_lower_count"] else (0, 0)
            bwd = (cert["dual_upper_worst"], -cert["dual_upper_arc"]) if cert["dual_upper_count"] else (0, 0)
            if inst.cap.min() > 0:     # (an arc of capacity 0 at rc > 0 ... cannot violate either class; at rc < 0 it is eligible but not "lower")
                assert (key, -arc) == max(fwd, bwd), (priced, cert)


# ------------------------------------------------------------------ 3. planted violations in caller's arrays
def _optimal(e, inst, rule=0, **kw):
    with _engine(e, inst, rule, **kw) as eng:
        eng.solve()
        res = eng.result()
    assert res.status == "optimal"
    return res


@pytest.mark.parametrize("kw", [dict(), dict(fused=False, mid_loop=-1), dict(tree_blocks=3)], ids=["small", "grid_dense", "grid_blocked"])
def test_planted_violations_trip_exactly_their_own_group(gpu_engine_module, kw):
    e = gpu_engine_module
    n, m = wri.SIZES["small"] if not kw else wri.SIZES["medium"]
    inst = wri.make(7, n, m, qmax=1 << 56)                      # flows near 2^56..2^59 (the ring arcs carry up to 8 qmax)
    assert int(np.abs(inst.cost).max()) in (wri.INT32_MAX, wri.cmax_for(n))
    res = _optimal(e, inst, **kw)
    with _engine(e, inst, 0, **kw) as eng:                      # a cold handle: only the instance counts
        clean = eng.certify(res.flow, res.potential)
        assert clean["verdict"] == "optimal" and clean["checks"] == 15 and clean["status"] == "running" and not clean["proves_status"]
        _assert_matches(clean, _np_cert(inst, inst.cost, res.flow, res.potential))
        capped = np.flatnonzero((inst.cap > 0) & (inst.cap < MCF_INF))

        # one arc over its capacity by (2^59 - cap): bounds, and the two nodes' balances
        a = int(capped[3])
        f = res.flow.copy()
        f[a] = (1 << 59) + 12345
        c = eng.certify(f, res.potential)
        want = _np_cert(inst, inst.cost, f, res.potential)
        _assert_matches(c, want)
        assert c["over_capacity_count"] == 1 and c["negative_flow_count"] == 0 and c["bounds_worst_arc"] == a
        assert c["bounds_worst"] == (1 << 59) + 12345 - int(inst.cap[a]) and c["imbalance_count"] == 2 and c["verdict"] == "not_proven"

        # one negative flow
        b = int(np.flatnonzero(res.flow == 0)[5])
        f = res.flow.copy()
        f[b] = -7
        c = eng.certify(f, res.potential)
        _assert_matches(c, _np_cert(inst, inst.cost, f, res.potential))
        assert c["negative_flow_count"] == 1 and c["over_capacity_count"] == 0 and (c["bounds_worst"], c["bounds_worst_arc"]) == (7, b)
        assert c["imbalance_count"] == 2 and c["imbalance_worst"] == 7 and c["imbalance_worst_node"] == min(inst.tail[b], inst.head[b])

        # one unit moved along a two-arc path u -> v -> w that is no cycle: u and w out of balance, bounds untouched
        room = (res.flow + 1 <= np.where(inst.cap < 0, MCF_INF, inst.cap))
        first = next(i for i in np.flatnonzero(room) if any(room[j] and inst.tail[j] == inst.head[i] and inst.head[j] != inst.tail[i]
                                                              for j in np.flatnonzero(inst.tail == inst.head[i])))
        second = next(j for j in np.flatnonzero(inst.tail == inst.head[first]) if room[j] and inst.head[j] != inst.tail[first])
        f = res.flow.copy()
        f[first] += 1
        f[second] += 1
        c = eng.certify(f, res.potential)
        _assert_matches(c, _np_cert(inst, inst.cost, f, res.potential))
        assert c["negative_flow_count"] == c["over_capacity_count"] == 0 and c["imbalance_count"] == 2 and c["imbalance_worst"] == 1
        assert c["imbalance_worst_node"] == min(inst.tail[first], inst.head[second])

        # one potential shifted: only the arcs at that node can change class; primal groups stay clean
        node = int(inst.tail[a])
        for shift in (1, -(1 << 40), wri.INT32_MAX):
            p = res.potential.copy()
            p[node] += shift
            c = eng.certify(res.flow, p)
            want = _np_cert(inst, inst.cost, res.flow, p)
            _assert_matches(c, want)
            assert c["negative_flow_count"] == c["over_capacity_count"] == c["imbalance_count"] == 0
            assert c["dual_lower_count"] + c["dual_upper_count"] > 0 and c["verdict"] == "not_proven"
            at_node = (inst.tail == node) | (inst.head == node)
            assert at_node[c["dual_lower_arc"]] if c["dual_lower_count"] else True
            assert at_node[c["dual_upper_arc"]] if c["dual_upper_count"] else True
            assert c["primal"] == clean["primal"]

        # costs of +INT32_MAX and -INT32_MAX planted on two arcs of a copy of the instance (a carries flow, b none): the same
        # flows and potentials certified against it -- the primal groups stay clean, the objective moves by flow[a] * the change
        cost2 = inst.cost.copy()
        cost2[a], cost2[b] = wri.INT32_MAX, -wri.INT32_MAX
        inst2 = generators.ArcSoA(inst.n, inst.tail, inst.head, cost2, inst.cap, inst.supply, "planted_costs")
        with _engine(e, inst2, 0, **kw) as eng2:
            c = eng2.certify(res.flow, res.potential)
        _assert_matches(c, _np_cert(inst2, cost2, res.flow, res.potential))
        assert c["negative_flow_count"] == c["over_capacity_count"] == c["imbalance_count"] == 0
        assert c["primal"] == clean["primal"] + int(res.flow[a]) * (wri.INT32_MAX - int(inst.cost[a]))
        rc_b = -wri.INT32_MAX + int(res.potential[inst.tail[b]]) - int(res.potential[inst.head[b]])
        if rc_b < 0 and inst.cap[b] != 0:            # b is empty and can take flow: a lower-class violation of exactly |rc|
            assert c["dual_lower_count"] >= 1 and c["dual_lower_worst"] >= -rc_b

        # a single group on request; unknown bits refused; potentials outside 2^61 refused
        only = eng.certify(f, res.potential, checks=e.CERT_BOUNDS)
        assert only["checks"] == 1 and only["imbalance_count"] == 0 and only["verdict"] == "not_proven"
        with pytest.raises(e.EngineError) as err:
            eng.certify(checks=64)
        assert err.value.code == -1
        p = res.potential.copy()
        p[0] = (1 << 61) + 1
        with pytest.raises(e.EngineError) as err:
            eng.certify(res.flow, p)
        assert err.value.code == -5
        # the cold handle itself was never touched
        cold = eng.certify()
        assert cold["status"] == "running" and all(cold[k] == 0 for k in BASIS_COUNTS) and cold["primal"] == 0


# ------------------------------------------------------------------ 4. read-only
@pytest.mark.parametrize("path,rule", PATH_CASES, ids=PATH_IDS)
def test_the_call_changes_no_later_pivot(gpu_engine_module, path, rule):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=5)
    runs = []
    for certify in (False, True):
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve(150)
            if certify:
                eng.certify()
                eng.bottlenecks(1, 2)
                eng.certify(np.zeros(inst.m, np.int64), np.zeros(inst.n, np.int64))
            eng.solve(37)
            if certify:
                eng.certify()
            eng.solve()
            res, tree = eng.result(), eng.tree()
        if path == "rc_drop":
            assert res.stats["rc_dropped_at"] > 0
        stats = {k: res.stats[k] for k in ("pivots", "degenerate", "bound_flips", "cycle_arcs", "subtree_nodes", "arcs_priced")}
        runs.append((res.status, res.objective, stats, res.flow, res.potential, tree["order"], tree["parent"], tree["state"]))
    a, b = runs
    assert a[:3] == b[:3]
    for x, y in zip(a[3:], b[3:]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 5. after update_costs, set_basis and reset
@pytest.mark.parametrize("path", ["small", "mid", "grid_dense", "grid_blocked_2", "key_codes"])
def test_after_update_costs_set_basis_and_reset(gpu_engine_module, path):
    e = gpu_engine_module
    kw, _, _, (n, m) = PATHS[path]
    inst = generators.netgen_style(n, m, seed=6)
    with _engine(e, inst, 2, **kw) as eng:
        eng.solve()
        res = eng.result()
        rng = np.random.default_rng(9)
        idx = rng.choice(inst.m, inst.m // 20, replace=False)
        cost = inst.cost.copy()
        cost[idx] = np.maximum(1, cost[idx] // 3)
        eng.update_costs(idx, cost[idx])
        c = eng.certify()
        tree = eng.tree()
        pi = tree["pi"][: inst.n] - tree["pi"][inst.n]
        _assert_matches(c, {k: v for k, v in _np_cert(inst, cost, res.flow, pi).items() if not k.startswith("imbalance")})
        assert c["status"] == "running" and c["verdict"] == "not_proven" and c["dual_lower_count"] + c["dual_upper_count"] > 0
        assert all(c[k] == 0 for k in BASIS_COUNTS) and c["rc_mismatch_count"] == 0 and c["key_mismatch_count"] == 0 and c["imbalance_count"] == 0
        eng.solve()
        again = eng.result()
        c = eng.certify()
        assert c["verdict"] == "optimal" and c["proves_status"] and c["primal"] == again.objective == int(np.dot(again.flow, cost))
        # reset: the cold start again, under the new costs
        eng.reset()
        c = eng.certify()
        # (every node hangs on the root by an artificial arc that carries |supply|: supplies flow in, demands flow out)
        assert c["status"] == "running" and c["primal"] == 0
        assert c["artificial_flow"] == int(np.abs(inst.supply).sum()) == eng.result().stats["artificial_flow"]
        assert all(c[k] == 0 for k in BASIS_COUNTS) and c["imbalance_count"] == 0 and c["basic_arcs"] == inst.n
        # the optimal basis installed: its flows are back before a single pivot is made (the potentials of a component that
        # hangs on a degenerate artificial arc may differ, so the dual half is not asserted here)
        assert eng.set_basis(again.in_tree, (again.flow == inst.cap) & ~again.in_tree & (inst.cap > 0))
        c = eng.certify()
        assert c["status"] == "running" and not c["proves_status"] and c["primal"] == again.objective
        assert all(c[k] == 0 for k in BASIS_COUNTS + ZERO_COUNTS[:3]) and c["rc_mismatch_count"] == 0
        # a basis that is not optimal: consistent at once, dual violations until re-solved
        eng.set_basis(res.in_tree, (res.flow == inst.cap) & ~res.in_tree & (inst.cap > 0))
        c = eng.certify()
        assert all(c[k] == 0 for k in BASIS_COUNTS) and c["imbalance_count"] == 0
        eng.solve()
        assert eng.certify()["verdict"] == "optimal"


def test_a_sharded_handle_checks_every_arc_and_its_own_reduced_costs(gpu_engine_module):
    e = gpu_engine_module
    inst = generators.netgen_style(1500, 12000, seed=8)
    res = _optimal(e, inst, 0, fused=False, mid_loop=-1)
    for rule in (0, 2):
        with _engine(e, inst, rule, shard=(1, 3), fused=False, mid_loop=-1) as eng:
            cold = eng.certify()
            assert all(cold[k] == 0 for k in BASIS_COUNTS) and cold["imbalance_count"] == 0 and cold["rc_mismatch_count"] == 0
            assert 0 < cold["rc_compared"] < inst.m
            want = _np_cert(inst, inst.cost, np.zeros(inst.m, np.int64), eng.tree()["pi"][: inst.n] - eng.tree()["pi"][inst.n])
            _assert_matches(cold, {k: v for k, v in want.items() if k.startswith("dual_") or k == "primal"})
            assert eng.set_basis(res.in_tree, (res.flow == inst.cap) & ~res.in_tree & (inst.cap > 0))
            warm = eng.certify()
            assert warm["primal"] == res.objective and warm["rc_mismatch_count"] == 0 and 0 < warm["rc_compared"] < inst.m
            assert all(warm[k] == 0 for k in BASIS_COUNTS + ZERO_COUNTS[:3])
            _assert_matches(eng.certify(res.flow, res.potential), _np_cert(inst, inst.cost, res.flow, res.potential))


# ------------------------------------------------------------------ 6. bottlenecks
def _np_bottlenecks(inst, flow, num, den):
    capped = (inst.cap >= 0) & (inst.cap < MCF_INF)
    return np.array([i for i, (f, c, k) in enumerate(zip(flow.tolist(), inst.cap.tolist(), capped.tolist()))
                     if k and f > 0 and f * den >= c * num], dtype=np.int64)


@pytest.mark.parametrize("kw", [dict(), dict(fused=False, mid_loop=-1)], ids=["small", "grid_dense"])
def test_bottlenecks_equal_exact_integers(gpu_engine_module, kw):
    e = gpu_engine_module
    base = vi.uncapacitated(3, *(vi.SIZES["small"] if not kw else vi.SIZES["medium"]))
    assert (base.cap == vi.EDGE_CAP).any()                       # an arc with cap = 2^60 - 1
    for inst in (base, generators.netgen_style(1500, 12000, seed=2)):
        with _engine(e, inst, 0, **kw) as eng:
            eng.solve()
            res = eng.result()
            for num, den in ((1, 1), (19, 20), (1, 2), (0, 1), (1, (1 << 62)), ((1 << 62), (1 << 62) + 1), (3, 2)):
                want = _np_bottlenecks(inst, res.flow, num, den)
                idx, count = eng.bottlenecks(num, den)
                assert count == want.size and np.array_equal(idx, want), (inst.name, num, den)
                few, count = eng.bottlenecks(num, den, limit=5)
                assert count == want.size and np.array_equal(few, want[:5])
            assert eng.certify()["saturated_arcs"] == _np_bottlenecks(inst, res.flow, 1, 1).size
            # a caller's flow: an arc of capacity 2^60 - 1 filled to the brim, and one unit short of it
            edge = int(np.flatnonzero(inst.cap == vi.EDGE_CAP)[0]) if (inst.cap == vi.EDGE_CAP).any() else None
            if edge is not None:
                f = res.flow.copy()
                f[edge] = vi.EDGE_CAP
                assert edge in eng.bottlenecks(1, 1, flow=f)[0]
                f[edge] = vi.EDGE_CAP - 1
                assert edge not in eng.bottlenecks(1, 1, flow=f)[0]
                assert edge in eng.bottlenecks((1 << 60) - 2, (1 << 60) - 1, flow=f)[0]
            with pytest.raises(e.EngineError):
                eng.bottlenecks(1, 0)


def test_bottlenecks_scan_more_than_1024_chunks(gpu_engine_module):
    """The scan of the chunk counts is one workgroup of 1 024 threads; from 1 024 * 4 096 + 4 097 arcs on there are more
    than 1 024 chunks of 4 096 indices and a thread scans more than one of them (`per > 1` in scan_chunk_totals)."""
    e = gpu_engine_module
    n, m = 64, 1024 * 4096 + 4097
    i = np.arange(m, dtype=np.int64)
    tail, head = (i % n).astype(np.int32), ((i + 1) % n).astype(np.int32)
    hit = i % 1000 == 7
    flow = np.where(hit, 10, 0).astype(np.int64)
    want = np.flatnonzero(hit)
    with e.McfEngine(n, tail, head, np.ones(m, dtype=np.int64), np.full(m, 10, dtype=np.int64), np.zeros(n, dtype=np.int64)) as eng:
        idx, count = eng.bottlenecks(1, 1, flow=flow, limit=m)
        assert count == want.size and np.array_equal(idx, want)
        few, count = eng.bottlenecks(1, 1, flow=flow, limit=10)
        assert count == want.size and np.array_equal(few, want[:10])


# ------------------------------------------------------------------ 8. scale
def test_a_quarter_million_nodes_certified_on_the_device(gpu_engine_module, capsys):
    """262 144 nodes / 2 M arcs on the auto-selected blocked list (the size of the update-costs scale test): the device
    certificate equals the host certificate from downloaded arrays, and must be the faster of the two end to end.  Both
    wall times, the kernel durations and their ratio are printed, none is asserted beyond "faster"."""
    e = gpu_engine_module
    inst = generators.netgen_style(1 << 18, 1 << 21, seed=1)
    with _engine(e, inst, 2) as eng:
        eng.solve()
        eng.certify()                                            # first call: scratch, supplies
        t0 = time.perf_counter()
        cert = eng.certify()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = eng.result()
        t_down = time.perf_counter() - t0
        check_optimality(inst, res.flow, res.potential)
        objective = int(np.dot(res.flow, inst.cost))             # (< 2^63 here)
        t_host = time.perf_counter() - t0
        idx, count = eng.bottlenecks(19, 20)
        assert res.stats["tree_blocks"] > 0 and res.status == "optimal"
    _assert_proven_optimal(cert, inst, res)
    assert cert["primal"] == objective
    _assert_matches(cert, _np_cert(inst, inst.cost, res.flow, res.potential))
    assert np.array_equal(idx, _np_bottlenecks(inst, res.flow, 19, 20)) and count == idx.size
    with capsys.disabled():
        print(f"\n  [certify 262144 / 2097152] device {t_dev * 1e3:.2f} ms (arc pass {cert['arc_pass_ms'] * 1e3:.1f} us, node pass "
              f"{cert['node_pass_ms'] * 1e3:.1f} us), host {t_host * 1e3:.1f} ms (download {t_down * 1e3:.1f} ms), ratio {t_host / t_dev:.1f}x", flush=True)
    assert t_dev < t_host


# ------------------------------------------------------------------ 7. the Python layer
def _chain_problem():
    import network_flow_solver_amd as nfs

    nodes = [{"id": "s", "supply": 10.0}, {"id": "a", "supply": 0.0}, {"id": "b", "supply": 0.0}, {"id": "t", "supply": -10.0}]
    arcs = [{"tail": "s", "head": "a", "capacity": 6.0, "cost": 1.0}, {"tail": "s", "head": "b", "capacity": 10.0, "cost": 2.5},
            {"tail": "a", "head": "t", "capacity": 8.0, "cost": 1.0}, {"tail": "b", "head": "t", "capacity": None, "cost": 1.0},
            {"tail": "a", "head": "b", "capacity": 4.0, "cost": 0.25, "lower": 0.0}]
    return nfs, nfs.build_problem(nodes, arcs, directed=True, tolerance=1e-6)


def test_validate_flow_and_bottlenecks_through_the_python_layer(gpu_engine_module):
    nfs, problem = _chain_problem()
    solver = nfs.NetworkSimplex(problem)
    result = solver.solve()
    assert result.status == "optimal"
    cert = solver.certify()
    assert cert.verdict == "optimal" and cert.proves_status and cert.gap == 0 and cert.basis_inconsistencies == 0
    assert cert.primal_objective == round(result.objective * cert.flow_scale * cert.cost_scale)
    assert cert.worst_bound_arc is None and cert.worst_dual_arc is None and cert.worst_imbalance_node is None
    good = nfs.validate_flow(problem, result)
    assert good.is_valid and good.errors == [] and good.capacity_violations == [] and good.lower_bound_violations == []
    assert good.flow_balance == {"s": 0.0, "a": 0.0, "b": 0.0, "t": 0.0}
    # s -> a is the only arc at its capacity (6 of 6); a -> t carries 6 of 8
    top = nfs.compute_bottleneck_arcs(problem, result)
    assert [(b.tail, b.head, b.flow, b.capacity, b.utilization, b.slack) for b in top] == [("s", "a", 6.0, 6.0, 1.0, 0.0)]
    wide = nfs.compute_bottleneck_arcs(problem, result, threshold=0.4)
    assert [(b.tail, b.head) for b in wide] == [("s", "a"), ("a", "t"), ("s", "b")] and wide[1].utilization == 0.75 and wide[2].utilization == 0.4
    # a deliberately broken result: one arc over its capacity, one below its lower bound, conservation broken at three nodes
    broken = nfs.FlowResult(objective=0.0, flows={("s", "a"): 7.5, ("a", "t"): 6.0, ("s", "b"): 4.0, ("b", "t"): 4.0, ("a", "b"): -1.0},
                            status="optimal", iterations=0, duals={})
    bad = nfs.validate_flow(problem, broken)
    assert not bad.is_valid and bad.capacity_violations == [("s", "a")] and bad.lower_bound_violations == [("a", "b")]
    assert bad.flow_balance == {"s": -1.5, "a": 2.5, "b": -1.0, "t": 0.0}
    assert len(bad.errors) == 2 + 3 and bad.errors[0] == "Arc (s, a): flow 7.500000 exceeds capacity 6.000000"


# ------------------------------------------------------------------ 7b. the reference's own answers, recorded
def _utils_cases():
    import json
    from pathlib import Path

    return json.loads((Path(__file__).parent / "golden" / "utils_cases.json").read_text())


def _as_soa(nfs, case):
    """The case as an SoAProblem (its node ids are "1" .. "n" in node order, its data integers)."""
    ids = [nd["id"] for nd in case["nodes"]]
    assert ids == [str(i + 1) for i in range(len(ids))]
    col = lambda k: [a[k] for a in case["arcs"]]                                         # noqa: E731
    ints = lambda xs: np.array([int(x) for x in xs], np.int64)                           # noqa: E731
    assert all(float(x) == int(x) for k in ("cost", "lower") for x in col(k))
    return nfs.SoAProblem(len(ids), ints(col("tail")) - 1, ints(col("head")) - 1, ints(col("cost")),
                          ints([-1 if c is None else c for c in col("capacity")]), ints([nd["supply"] for nd in case["nodes"]]),
                          lower=ints(col("lower")), tolerance=case["tolerance"])


@pytest.mark.parametrize("case", _utils_cases(), ids=lambda c: c["name"])
def test_utils_return_what_the_reference_recorded(gpu_engine_module, case):
    """tests/golden/utils_cases.json holds what the reference's validate_flow / compute_bottleneck_arcs returned
    (make_utils_golden.py) for its own solved flows and for one broken flow dict per problem: every field is compared.
    Lists, messages, orders and the bottleneck floats are equal; the balances agree to 1e-9 (a clean result reports exact
    zeros where the reference reports its float residuals, and the host's sums run in another order)."""
    import network_flow_solver_amd as nfs

    problems = [nfs.build_problem(case["nodes"], case["arcs"], directed=case["directed"], tolerance=case["tolerance"])]
    if case["name"].startswith("soa_"):
        problems.append(_as_soa(nfs, case))
    for problem in problems:
        for which in ("solved", "broken"):
            rec = case[which]
            result = nfs.FlowResult(objective=0.0, flows={(t, h): f for t, h, f in rec["flows"]}, status="optimal", iterations=0, duals={})
            got, want = nfs.validate_flow(problem, result), rec["validate"]
            assert got.is_valid == want["is_valid"] and got.errors == want["errors"], (which, got.errors, want["errors"])
            assert [list(k) for k in got.capacity_violations] == want["capacity_violations"]
            assert [list(k) for k in got.lower_bound_violations] == want["lower_bound_violations"]
            assert list(got.flow_balance) == list(want["flow_balance"])
            assert all(abs(got.flow_balance[k] - v) <= 1e-9 for k, v in want["flow_balance"].items()), (got.flow_balance, want["flow_balance"])
            for th, arcs in rec["bottlenecks"].items():
                top = nfs.compute_bottleneck_arcs(problem, result, threshold=float(th))
                assert [[b.tail, b.head, b.flow, b.capacity, b.utilization, b.cost, b.slack] for b in top] == arcs, (which, th)
