"""The HIP kernels at the edges of the engine's numeric domain (``-m gpu``).

Instances: ``wide_range_instances`` -- |cost| up to INT32_MAX with negative and zero costs, capacities and supplies up
to 2^56, reduced costs up to ~2^45, objectives beyond 64 bits.  Yardsticks: the CPU emulation of the same headers
(pivot for pivot), numpy int64 / Python-int arithmetic (reduced costs, key codes, arg-max, certificate, objective) and
the oracle's restated block selection (Devex merits, bit for bit).  Every comparison is exact.

Each test prints one line under ``-s`` / in the captured log: engine path, instances compared pivot for pivot, the
objective classes seen (> 2^63, negative) and, where key codes are read, the arcs seen per code class."""

import functools

import numpy as np
import pytest

import oracle
import network_flow_solver_amd as nfs
import wide_range_instances as wri
from conftest import check_tree_invariants
from test_gpu_parity import _check_shard_state, _drive_shards
from wide_range_instances import _vkey_code

pytestmark = pytest.mark.gpu

RULE_IDS = {0: "dantzig", 1: "devex_block", 2: "candidate_list"}
LADDER = (0, 1, 5, 40, 300, 10 ** 9)             # pivot budgets, cumulative: the states 0, 1, 6, 46, 346, final

# every engine path that has kernel code of its own: options, the rules it supports, stats()["pricing_mode"]
PATHS = {
    "fused_lds": (dict(fused=True), (0, 1, 2), 2),                                                    # k_solve_small
    "kernel_per_phase_graph": (dict(fused=False, mid_loop=-1, use_graph=True), (0, 1, 2), 1),         # k_price_rc, k_pivot, k_update, k_rcupd
    "kernel_per_phase_eager": (dict(fused=False, mid_loop=-1, use_graph=False, batch_pivots=7), (0, 1, 2), 1),
    "persistent_loop": (dict(fused=False, mid_loop=1), (0, 1, 2), 3),                                 # k_solve_mid
    "gather_pricing": (dict(fused=False, mid_loop=-1, resident_rc=False), (0, 1, 2), 0),              # k_price
    "key_codes": (dict(fused=False, mid_loop=-1, compressed_keys=1), (0, 2), 1),                      # k_price_v
    "key_codes_half_2_12": (dict(fused=False, mid_loop=-1, compressed_keys=1, vkey_half_log2=12), (0, 2), 1),
    "no_key_codes": (dict(fused=False, mid_loop=-1, compressed_keys=-1), (0, 2), 1),                  # k_price_rc
    "blocked_list": (dict(tree_blocks=3), (0, 1, 2), 1),                                 # k_update_bpl
}
PATH_CASES = [(p, r) for p, (_, rules, _) in PATHS.items() for r in rules]


@functools.lru_cache(maxsize=None)
def _instance(kind):
    return {"small": lambda: wri.make(0), "small_ties": lambda: wri.make(1, tie_rich=True), "small_q56": lambda: wri.make(2, qmax=1 << 56),
            "small_q20": lambda: wri.make(3, qmax=1 << 20), "chain": wri.chain_instance, "chain_c1000": lambda: wri.chain_instance(chain_cost=1000),
            "medium": lambda: wri.make(0, *wri.SIZES["medium"]), "medium_ties": lambda: wri.make(1, *wri.SIZES["medium"], tie_rich=True),
            "medium_q56": lambda: wri.make(2, *wri.SIZES["medium"], qmax=1 << 56),
            "medium_pos": lambda: wri.make(0, *wri.SIZES["medium"], nonneg=True),
            "large": lambda: wri.make(0, *wri.SIZES["large"]), "edge": wri.edge_instance}[kind]()


@functools.lru_cache(maxsize=None)
def _emul(kind, rule, max_pivots=-1):
    i = _instance(kind)
    return oracle.emul_solve(i.n, i.tail, i.head, i.cost, i.cap, i.supply, rule=rule, max_pivots=max_pivots)


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _big_m(inst):
    return wri.big_m_of(inst.n, int(np.abs(inst.cost).max()))


def _same_as_emulation(res, tree, em):
    assert res.stats["pivots"] == em["pivots"] and res.stats["degenerate"] == em["degenerate"]
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"])
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"])


def _certified(inst, res, tree):
    """The result proves itself: exact certificate, the 128-bit objective (two 64-bit halves) == the sum over Python ints."""
    assert res.status == "optimal"
    exact = wri.exact_certificate(inst, res.flow, res.potential)
    assert isinstance(res.objective, int) and res.objective == exact
    check_tree_invariants(inst.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
    return exact


def _classes(objectives):
    return {"above_2^63": sum(o > 1 << 63 for o in objectives), "negative": sum(o < 0 for o in objectives)}


def _log(capsys, text):
    with capsys.disabled():
        print(f"\n  [numeric range] {text}", flush=True)


# ------------------------------------------------------------------ whole solves, every path
@pytest.mark.parametrize("path,rule", PATH_CASES, ids=[f"{p}-{RULE_IDS[r]}" for p, r in PATH_CASES])
def test_every_engine_path_pivots_like_the_emulation(gpu_engine_module, capsys, path, rule):
    """Pivot for pivot with the CPU emulation (pivots, degenerate pivots, flows, potentials, preorder, parents), the exact
    objective out of the two 64-bit halves, the Python-int certificate and the tree invariants -- on the 60-node family
    (uniform, tie-rich, qmax 2^56 and 2^20), the chain instance and, beyond the LDS path, on 1 024 nodes."""
    e = gpu_engine_module
    kw, _, mode = PATHS[path]
    kinds = ["small", "small_ties", "small_q56", "small_q20", "chain"] + ([] if path == "fused_lds" else ["medium", "medium_ties"])
    objectives = []
    for kind in kinds:
        inst, em = _instance(kind), _emul(kind, rule)
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve()
            res, tree = eng.result(), eng.tree()
            if path.startswith("key_codes"):
                assert eng.pricing_keys()[1] and res.stats["sweep_variant"] & 1
            if path == "no_key_codes":
                assert not eng.pricing_keys()[1]
        assert res.stats["pricing_mode"] == mode, (path, kind, res.stats["pricing_mode"])
        if path == "blocked_list":
            assert res.stats["tree_blocks"] == 3
        assert em["status"] == "optimal" and res.objective == em["objective"]
        _same_as_emulation(res, tree, em)
        objectives.append(_certified(inst, res, tree))
    seen = _classes(objectives)
    assert seen["above_2^63"] > 0 and seen["negative"] > 0, seen
    _log(capsys, f"{path} / {RULE_IDS[rule]}: {len(kinds)} instances pivot for pivot, objectives {seen}")


LARGE_CASES = [("persistent_loop", 0), ("persistent_loop", 1), ("persistent_loop", 2), ("kernel_per_phase_graph", 2), ("blocked_list", 1)]


@pytest.mark.parametrize("path,rule", LARGE_CASES, ids=[f"{p}-{RULE_IDS[r]}" for p, r in LARGE_CASES])
def test_mid_loop_size_and_admissibility_edge(gpu_engine_module, capsys, path, rule):
    """4 096 nodes / 32 768 + 4 096 arcs, and n = 8 189 with one arc at INT32_MAX (big-M = 2^44 - 2^31, reduced costs to
    2^45): pivot for pivot with the emulation over the first 3 000 pivots (the emulation needs half a minute for the whole
    Dantzig solve), then to the end, where the result has to prove itself (certificate, exact objective)."""
    e = gpu_engine_module
    kw, _, mode = PATHS[path]
    objectives = []
    for kind in ("large", "edge"):
        inst, em = _instance(kind), _emul(kind, rule, 3000)
        with _engine(e, inst, rule, **kw) as eng:
            eng.solve(max_pivots=3000)
            res, tree = eng.result(), eng.tree()
            assert res.stats["pricing_mode"] == mode and res.status == em["status"] == "iteration_limit"
            assert res.objective == em["objective"] == wri.exact_objective(inst, res.flow)
            _same_as_emulation(res, tree, em)
            eng.solve()
            res, tree = eng.result(), eng.tree()
        objectives.append(_certified(inst, res, tree))
    _log(capsys, f"{path} / {RULE_IDS[rule]}: 2 instances pivot for pivot over 3 000 pivots, certified at the end, objectives {_classes(objectives)}")


# ------------------------------------------------------------------ resident reduced costs and key codes along a solve
@pytest.mark.parametrize("mid_loop", [-1, 1], ids=["kernel_per_phase", "persistent_loop"])
@pytest.mark.parametrize("rule", [0, 1, 2], ids=list(RULE_IDS.values()))
def test_resident_reduced_costs_stay_exact_at_2_45(gpu_engine_module, rule, mid_loop):
    """k_rcupd / k_solve_mid patch the resident reduced costs by +-sigma with sigma up to ~2^45: resident copy ==
    cost + pi[tail] - pi[head] in int64 for every arc at every stage, on 1 024 nodes and at the admissibility edge."""
    for kind in ("medium", "edge"):
        inst = _instance(kind)
        with _engine(gpu_engine_module, inst, rule, fused=False, mid_loop=mid_loop, full_sweeps=-1) as eng:
            largest = 0
            for budget in LADDER[:-1] + ((10 ** 9,) if kind == "medium" else (2000,)):
                if budget:
                    eng.solve(max_pivots=budget)
                rc, resident = eng.reduced_costs()
                assert resident
                pi = eng.tree()["pi"]
                assert rc.dtype == np.int64 and np.array_equal(rc, inst.cost + pi[inst.tail] - pi[inst.head])
                largest = max(largest, int(np.abs(rc).max()))
            assert largest > 1 << (41 if kind == "medium" else 44)      # values a 32-bit lane would have lost


@pytest.mark.parametrize("half_log2", [0, 12], ids=["half_2_28", "half_2_12"])
@pytest.mark.parametrize("rule", [0, 2], ids=["dantzig", "candidate_list"])
def test_key_codes_stay_exact_in_every_code_class(gpu_engine_module, capsys, rule, half_log2):
    """k_price_v reads 4-byte codes: code == mcf_vkey(-state * rc) for every arc at every stage of the budget ladder, and
    all six code classes occur -- ineligible, the three levels, saturated between two levels, saturated above level 2
    (the family gives five of them at big-M ~ 2^41; level 1 comes from the chain instance, whose violation walks down
    from 2 big-M to big-M + 3 C; tests/test_numeric_range_cpu.py checks on the emulation that they do occur)."""
    e = gpu_engine_module
    half = 1 << (half_log2 or 28)
    seen = dict.fromkeys(wri.KEY_CLASSES, 0)
    for kind in ("medium", "chain" if half_log2 == 0 else "chain_c1000"):
        inst, big_m = _instance(kind), _big_m(_instance(kind))
        with _engine(e, inst, rule, fused=False, mid_loop=-1, compressed_keys=1, vkey_half_log2=half_log2,
                     full_sweeps=-1 if rule == 0 else 1) as eng:
            for budget in LADDER:
                if budget:
                    eng.solve(max_pivots=budget)
                keys, present = eng.pricing_keys()
                assert present
                t = eng.tree()
                viol = -(t["state"].astype(np.int64)) * (inst.cost + t["pi"][inst.tail] - t["pi"][inst.head])
                assert np.array_equal(keys, _vkey_code(viol, big_m, half))
                for k, c in wri.key_classes(viol, big_m, half).items():
                    seen[k] += c
            res, tree = eng.result(), eng.tree()
        _same_as_emulation(res, tree, _emul(kind, rule))
        _certified(inst, res, tree)
    assert all(seen.values()), seen
    _log(capsys, f"key codes / {RULE_IDS[rule]} / half 2^{half_log2 or 28}: arcs per code class over the ladder {seen}")


# ------------------------------------------------------------------ kernel level: one pricing pass
def _ranges(m):
    return [(0, m), (37, m - 113), (m // 3, min(m, m // 3 + 1003)), (m - 41, m), (5, 6)]


@pytest.mark.parametrize("path", ["fused_lds", "kernel_per_phase_graph", "gather_pricing", "persistent_loop"])
def test_dantzig_pick_equals_the_int64_argmax(gpu_engine_module, path):
    """mcf_price_once (Dantzig) against numpy's int64 arg-max (first index among equals) over the whole arc range and
    over unaligned sub-ranges, with violations up to 2^45: the arc AND the violation, which no 32-bit lane of a
    reduction can carry."""
    kw = PATHS[path][0]
    for kind in ("small", "small_ties") if path == "fused_lds" else ("medium", "medium_ties", "edge"):
        inst = _instance(kind)
        largest = picks = 0
        with _engine(gpu_engine_module, inst, 0, **kw) as eng:
            for budget in LADDER[:-1] + (1500,):
                if budget:
                    eng.solve(max_pivots=budget)
                t = eng.tree()
                viol = -(t["state"].astype(np.int64)) * (inst.cost + t["pi"][inst.tail] - t["pi"][inst.head])
                for lo, hi in _ranges(inst.m):
                    sub = np.zeros_like(viol)
                    sub[lo:hi] = viol[lo:hi]
                    got = eng.price_once(0, lo, hi)
                    if sub.max() <= 0:
                        assert got is None
                        continue
                    assert got is not None and got[0] == int(np.argmax(sub)) and got[2] == int(sub.max()), (kind, budget, lo, hi, got)
                    assert got[1] == int(t["state"][got[0]])
                    largest = max(largest, got[2])
                    picks += 1
        assert picks >= 10 and largest > 1 << (32 if kind.startswith("small") else 41), (kind, picks, largest)


def _block_reference(inst, tree, weights, lo, hi):
    """oracle.price_block = the restated NetworkSimplex._select_entering_arc_vectorized, in float64, on the engine's
    state.  The residuals are the engine's arc states (eligible forward: state +1, backward: state -1), which is what the
    kernel prices by: a zero-capacity arc sits "at its lower bound" for the engine."""
    state = tree["state"]
    return oracle.price_block(inst.tail, inst.head, inst.cost.astype(np.float64), tree["pi"][: inst.n].astype(np.float64),
                              (state > 0).astype(np.float64), (state < 0).astype(np.float64), (state == 0).astype(np.uint8),
                              weights.astype(np.float64), lo, hi)


@pytest.mark.parametrize("path", ["fused_lds", "kernel_per_phase_graph", "gather_pricing", "persistent_loop"])
def test_devex_merit_bit_pattern_beyond_2_27(gpu_engine_module, path):
    """mcf_price_once (Devex) against the float64 reference selection on IDENTICAL state and weights: arc, direction and
    the merit's BIT PATTERN, at stages of a Devex solve where |rc| > 2^27 -- rc^2 is then not representable, so a float
    intermediate, a contracted multiply-divide or another order of the two operations shows in the last bits."""
    kw = PATHS[path][0]
    for kind in ("small", "small_ties") if path == "fused_lds" else ("medium", "medium_ties"):
        inst = _instance(kind)
        checked = inexact = ties = 0
        with _engine(gpu_engine_module, inst, 1, **kw) as eng:
            for budget in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 600):
                if budget:
                    eng.solve(max_pivots=budget)
                tree, w = eng.tree(), eng.weights()
                assert (w >= 1).all()
                viol = -(tree["state"].astype(np.int64)) * (inst.cost + tree["pi"][inst.tail] - tree["pi"][inst.head])
                merit = np.where(viol > 0, viol.astype(np.float64) * viol.astype(np.float64) / w.astype(np.float64), 0.0)
                for lo, hi in _ranges(inst.m):
                    got, exp = eng.price_once(1, lo, hi), _block_reference(inst, tree, w, lo, hi)
                    if exp is None:
                        assert got is None
                        continue
                    assert got is not None and (got[0], got[1]) == (exp[0], exp[1]), (kind, budget, lo, hi, got, exp)
                    assert np.int64(got[2]) == np.float64(exp[2]).view(np.int64), (kind, budget, lo, hi, got, exp)
                    v = int(viol[exp[0]])
                    assert v > 0 and exp[2] == merit[exp[0]]
                    checked += 1
                    if v > 1 << 27 and int(float(v) * float(v)) != v * v:
                        inexact += 1
                    ties += int((merit[lo:hi] == exp[2]).sum() > 1)
        assert checked >= 20 and inexact >= 10, (kind, checked, inexact)
        if kind.endswith("ties"):
            assert ties > 0, kind


@pytest.mark.parametrize("mode", ["forward_first", "priority", "capacity"])
def test_key_variants_at_violations_near_2_45(gpu_engine_module, mode):
    """KEY_FORWARD_FIRST / KEY_PRIORITY: bit 61 on top of violations near 2^45 (the admissibility edge), against the
    int64 merit; KEY_CAPACITY: float64(cap) * float64(viol) with capacities near 2^58 and violations near 2^42, against
    numpy's float64 product.  First index among equals; the parity hook still reports the plain violation."""
    e = gpu_engine_module
    kind = "medium_q56" if mode == "capacity" else "edge"
    inst = _instance(kind)
    prio = np.random.default_rng(5).integers(0, 4, inst.m).astype(np.int8) if mode == "priority" else None
    key_mode = {"forward_first": e.KEY_FORWARD_FIRST, "priority": e.KEY_PRIORITY, "capacity": e.KEY_CAPACITY}[mode]
    for kw in (dict(fused=False, mid_loop=-1), dict(fused=False, mid_loop=-1, resident_rc=False), dict(fused=False, mid_loop=1)):
        largest = 0
        with _engine(e, inst, 0, key_mode=key_mode, arc_priority=prio, **kw) as eng:
            for budget in LADDER[:-1]:
                if budget:
                    eng.solve(max_pivots=budget)
                t = eng.tree()
                state = t["state"].astype(np.int64)
                viol = -state * (inst.cost + t["pi"][inst.tail] - t["pi"][inst.head])
                elig = viol > 0
                if mode == "capacity":
                    capf = np.where((inst.cap < 0) | (inst.cap >= wri.MCF_INF), np.inf, inst.cap.astype(np.float64))
                    merit = np.where(elig, capf * viol.astype(np.float64), 0.0)
                else:
                    pref = (state > 0) if mode == "forward_first" else ((prio & np.where(state > 0, 1, 2)) != 0)
                    merit = np.where(elig, viol + pref.astype(np.int64) * (1 << 61), 0)
                for lo, hi in _ranges(inst.m)[:3]:
                    got = eng.price_once(0, lo, hi)
                    if merit[lo:hi].max() <= 0:
                        assert got is None
                        continue
                    assert got is not None and got[0] == lo + int(np.argmax(merit[lo:hi])), (mode, kw, budget, lo, hi, got)
                    if mode != "capacity":
                        assert got[2] == int(viol[got[0]])
                    largest = max(largest, int(viol[got[0]]))
        assert largest > 1 << (41 if mode == "capacity" else 44)


# ------------------------------------------------------------------ batches, shards, warm start, the shim
def test_batched_launches_on_mixed_wide_range_instances(gpu_engine_module, capsys):
    """mcf_solve_batch: LDS-loop handles in one launch and persistent-loop handles (with LDS ones mixed in) in another,
    rules and instance kinds mixed -- each ends exactly where the emulation ends."""
    e = gpu_engine_module
    for label, kinds, kw in (("small batch", ["small", "small_ties", "small_q56", "small_q20", "chain"] * 3, {}),
                             ("mid batch", ["medium", "small", "medium_ties", "chain", "medium_q56", "small_ties"], {"mid_loop": 1})):
        rules = [k % 3 for k in range(len(kinds))]
        engines = [_engine(e, _instance(kind), rule, **kw) for kind, rule in zip(kinds, rules)]
        try:
            modes = sorted({eng.stats()["pricing_mode"] for eng in engines})
            assert modes == ([2] if not kw else [2, 3])
            e.solve_batch(engines, max_pivots=29)
            e.solve_batch(engines)
            objectives = []
            for eng, kind, rule in zip(engines, kinds, rules):
                res, tree = eng.result(), eng.tree()
                _same_as_emulation(res, tree, _emul(kind, rule))
                objectives.append(_certified(_instance(kind), res, tree))
        finally:
            for eng in engines:
                eng.close()
        seen = _classes(objectives)
        assert seen["above_2^63"] > 0 and seen["negative"] > 0
        _log(capsys, f"{label}: {len(kinds)} instances pivot for pivot, objectives {seen}")


@pytest.mark.parametrize("rule", [0, 1, 2], ids=list(RULE_IDS.values()))
def test_three_sharded_handles_in_lock_step(gpu_engine_module, capsys, rule):
    """Three sharded handles on one GPU (per-pivot protocol; candidate lists for rule 2), key codes and incremental sweeps
    on where the rule has them: replicas bit-identical, every rank's reduced costs and codes exact, Dantzig / Devex pivot
    for pivot with the (unsharded) emulation, the result certified."""
    e = gpu_engine_module
    objectives = []
    for kind in ("medium", "medium_pos"):
        inst = _instance(kind)
        keyed = rule != 1
        opts = dict(compressed_keys=1, full_sweeps=-1) if rule != 1 else {}
        engs = _drive_shards(e, inst, rule, 3, 10 ** 9, rule == 2, **opts)
        try:
            res, tree = _check_shard_state(e, inst, engs, keyed=keyed)
        finally:
            for eng in engs:
                eng.close()
        objectives.append(_certified(inst, res, tree))
        em = _emul(kind, rule)
        assert res.objective == em["objective"]
        if rule != 2:     # (sharded, a candidate list holds one entry per rank's workgroup: another, equally valid, pivot sequence)
            _same_as_emulation(res, tree, em)
    seen = _classes(objectives)
    assert seen["above_2^63"] > 0 and seen["negative"] > 0
    _log(capsys, f"three shards / {RULE_IDS[rule]}: 2 instances{' pivot for pivot' if rule != 2 else ''}, objectives {seen}")


@pytest.mark.parametrize("path,rule", [("fused_lds", 0), ("kernel_per_phase_graph", 1), ("persistent_loop", 2), ("blocked_list", 1)])
def test_warm_start_from_a_wide_range_optimum(gpu_engine_module, path, rule):
    """mcf_set_basis with flows and potentials of 2^40: the optimal basis comes back with the same flows; its real arcs
    span the nodes, so nothing with room to move is eligible -- what remains is one bound flip of step 0 per
    zero-capacity arc with a negative reduced cost (see the CPU test of the same name), and nothing at all without
    such arcs."""
    kw = PATHS[path][0]
    inst = _instance("small" if path == "fused_lds" else "medium")
    keep = inst.cap != 0
    from network_flow_solver_amd.generators import ArcSoA
    bare = ArcSoA(inst.n, inst.tail[keep], inst.head[keep], inst.cost[keep], inst.cap[keep], inst.supply, inst.name + "_no_zero_caps")
    for case in (inst, bare):
        with _engine(gpu_engine_module, case, rule, **kw) as eng:
            eng.solve()
            cold = eng.result()
            assert cold.status == "optimal" and int(cold.in_tree.sum()) == case.n - 1
            at_upper = (~cold.in_tree & (cold.flow == case.cap) & (case.cap > 0)).astype(np.int8)
            assert eng.set_basis(cold.in_tree.astype(np.int8), at_upper)
            eng.solve()
            warm, tree = eng.result(), eng.tree()
        assert warm.objective == cold.objective and np.array_equal(warm.flow, cold.flow)
        rc = case.cost + cold.potential[case.tail] - cold.potential[case.head]
        flips = int(((case.cap == 0) & (rc < 0)).sum())
        assert warm.stats["pivots"] == warm.stats["degenerate"] == warm.stats["bound_flips"] == flips
        assert (case is inst) == (flips > 0)
        _certified(case, warm, tree)


def test_supply_range_on_the_device_side_of_the_abi(gpu_engine_module):
    """mcf_create refuses [2^60, 2^60, -2^61] with MCF_E_RANGE and a message (on the host: no kernel is launched for
    it), and solves the largest admissible supply to the exact objective on every rule."""
    e = gpu_engine_module
    tail, head = np.array([0, 1], np.int32), np.array([2, 2], np.int32)
    cost, cap = np.array([wri.INT32_MAX, -5], np.int64), np.array([-1, -1], np.int64)
    with pytest.raises(e.EngineError) as err:
        e.McfEngine(3, tail, head, cost, cap, np.array([1 << 60, 1 << 60, -(1 << 61)], np.int64))
    assert err.value.code == -5 and "supplies" in str(err.value) and "2^60" in str(err.value)
    supply = np.array([1 << 59, (1 << 59) - 1, -((1 << 60) - 1)], np.int64)
    for rule in (0, 1, 2):
        for kw in ({}, dict(fused=False, mid_loop=-1), dict(fused=False, mid_loop=1)):
            with e.McfEngine(3, tail, head, cost, cap, supply, rule=rule, **kw) as eng:
                eng.solve()
                res = eng.result()
            assert res.status == "optimal" and res.flow.tolist() == [1 << 59, (1 << 59) - 1]
            assert res.objective == (1 << 59) * wri.INT32_MAX - 5 * ((1 << 59) - 1) > 1 << 89


def test_the_shim_rounds_the_exact_objective_once(gpu_engine_module):
    """solve_min_cost_flow on a SoAProblem of the family: FlowResult.objective is a float there, and it has to be the
    exact 128-bit objective rounded ONCE -- float(exact) -- not a float sum of float products (which is off by
    thousands of units in the last place at 2^75)."""
    for kind in ("small", "small_q56", "chain"):
        inst = _instance(kind)
        exact = _emul(kind, 0)["objective"]
        assert abs(exact) > 1 << 63
        problem = nfs.SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply)
        for strategy in ("dantzig", "devex", "candidate_list"):
            got = nfs.solve_min_cost_flow(problem, nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True))
            assert got.status == "optimal" and isinstance(got.objective, float) and got.objective == float(exact)
            assert wri.exact_objective(inst, got.flows.array) == exact
