"""GPU parity tests (``-m gpu``): the HIP engine, called through the C ABI, against

* the reference-derived golden fixtures (exact status / integer objective / flows),
* the oracle (oracle/ref_simplex.c) on freshly seeded instances,
* the CPU emulation of the same pivot algorithm (pivot-for-pivot: any divergence is a
  parallelisation or memory-ordering bug),
* and, at BASELINE.json sizes, size-independent certificates (conservation, bounds,
  complementary slackness, tree invariants).

Integer / index work throughout, so every comparison is exact (no tolerance)."""

import json
from pathlib import Path

import numpy as np
import pytest

import oracle
import network_flow_solver_amd as nfs
from conftest import (CASE_IDS, CASES, check_optimality, check_tree_invariants, golden_flows, load_synthetic,
                      optimum_is_unique)
from network_flow_solver_amd import generators
from wide_range_instances import _vkey_code

pytestmark = pytest.mark.gpu

RULES = [0, 1, 2]
RULE_IDS = ["dantzig", "devex_block", "candidate_list"]


def _solve(engine, inst, rule, **kw):
    with engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw) as eng:
        eng.solve()
        return eng.result(), eng.tree()


# ------------------------------------------------------------------ golden fixtures, raw C ABI
@pytest.mark.parametrize("entry,inst", load_synthetic(), ids=lambda x: x["name"] if isinstance(x, dict) else "")
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_synthetic_goldens_exact(gpu_engine_module, entry, inst, rule):
    exp = next(iter(entry["expected"].values()))
    res, tree = _solve(gpu_engine_module, inst, rule)
    assert res.status == "optimal"
    assert res.objective == int(round(exp["objective"]))
    check_tree_invariants(inst.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
    rc = check_optimality(inst, res.flow, res.potential)
    if optimum_is_unique(inst, res.flow, res.in_tree, rc):
        got = {(int(inst.tail[i]), int(inst.head[i])): float(res.flow[i]) for i in range(inst.m) if res.flow[i]}
        assert got == golden_flows(exp)
    # differential against the CPU emulation of the same algorithm
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)
    assert res.stats["pivots"] == em["pivots"] and res.stats["degenerate"] == em["degenerate"]
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"])
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"])


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_fused_lds_path_equals_three_kernel_path(gpu_engine_module, rule):
    """Small instances run as ONE persistent LDS-resident workgroup; the same instance forced
    through the three-kernel path (graph and eager) must give the identical pivot sequence."""
    for idx in (0, 3, 6):
        _, inst = load_synthetic()[idx]
        runs = [_solve(gpu_engine_module, inst, rule, fused=True),
                _solve(gpu_engine_module, inst, rule, fused=False, mid_loop=-1, use_graph=True),
                _solve(gpu_engine_module, inst, rule, fused=False, mid_loop=-1, use_graph=False, batch_pivots=7),
                _solve(gpu_engine_module, inst, rule, fused=False, mid_loop=1),              # persistent loop, global state
                _solve(gpu_engine_module, inst, rule, fused=False, mid_loop=1, use_graph=False)]
        assert [r.stats["pricing_mode"] for r, _ in runs] == [2, 1, 1, 3, 3]
        (r0, t0) = runs[0]
        assert r0.stats["batches"] <= 2                      # one launch for the whole solve (+ re-arm)
        for r, t in runs[1:]:
            assert r.stats["pivots"] == r0.stats["pivots"] and r.objective == r0.objective
            assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential)
            assert np.array_equal(t["order"], t0["order"]) and np.array_equal(t["parent"], t0["parent"])
            assert r.stats["arcs_priced"] == r0.stats["arcs_priced"] and r.stats["degenerate"] == r0.stats["degenerate"]


@pytest.mark.parametrize("mid_loop", [-1, 1], ids=["kernel_per_phase", "persistent_loop"])
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_resident_reduced_costs_stay_exact(gpu_engine_module, rule, mid_loop):
    """Large instances price from RESIDENT reduced costs that k_rcupd patches after every basis
    swap.  Invariant: the resident copy equals cost + pi[tail] - pi[head] for every arc, at every
    stage of the solve; and the pivot sequence equals the gather-priced one."""
    _, inst = load_synthetic()[7]                                  # 1 024 nodes / 8 192 arcs: past the LDS path
    e = gpu_engine_module
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, mid_loop=mid_loop,
                     full_sweeps=-1) as eng:                       # incremental sweeps across budgets / resumes as well
        for budget in (0, 1, 5, 40, 300, 10 ** 9):
            if budget:
                eng.solve(max_pivots=budget)
            rc, resident = eng.reduced_costs()
            assert resident
            pi = eng.tree()["pi"]
            assert np.array_equal(rc, inst.cost + pi[inst.tail] - pi[inst.head])
        res, tree = eng.result(), eng.tree()
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule,
                     resident_rc=False) as eng:
        eng.solve()
        assert not eng.reduced_costs()[1]
        ref, rtree = eng.result(), eng.tree()
    assert res.status == ref.status == "optimal" and res.stats["pivots"] == ref.stats["pivots"]
    assert np.array_equal(res.flow, ref.flow) and np.array_equal(res.potential, ref.potential)
    assert np.array_equal(tree["order"], rtree["order"]) and res.stats["arcs_priced"] == ref.stats["arcs_priced"]


@pytest.mark.parametrize("rule", [0, 2], ids=["dantzig", "candidate_list"])
@pytest.mark.parametrize("variant", ["plain", "levels", "levels_narrow", "narrow"])
def test_compressed_pricing_keys(gpu_engine_module, rule, variant):
    """The Dantzig / candidate-list grid sweep reads 4-byte key codes (k_price_v) instead of reduced cost + state.
    Invariant at several stages of a solve: code == mcf_vkey(-state * rc) for every arc; and the pivot sequence equals
    the one of the uncompressed sweep (and of the CPU emulation) -- also when big-M forces the level coding (costs up
    to 2 * 10^6 on 1 024 nodes: big-M ~ 2 * 10^9) and when a narrow level width pushes most arcs into the
    exact-compare path (MCF_VKEY_SAT)."""
    e = gpu_engine_module
    _, inst = load_synthetic()[7]                                  # 1 024 nodes / 8 192 arcs
    cost = inst.cost if variant in ("plain", "narrow") else inst.cost * 200
    half_log2 = {"plain": 0, "levels": 0, "levels_narrow": 12, "narrow": 10}[variant]
    bigm = (int(np.abs(cost).max()) + 1) * (inst.n + 2)
    assert (bigm >= 1 << 29) == (variant.startswith("levels"))
    kw = dict(rule=rule, fused=False, mid_loop=-1, full_sweeps=-1 if rule == 0 else 1)
    sat_seen = 0
    with e.McfEngine(inst.n, inst.tail, inst.head, cost, inst.cap, inst.supply, vkey_half_log2=half_log2, compressed_keys=1, **kw) as eng:
        for budget in (0, 1, 5, 40, 300, 10 ** 9):
            if budget:
                eng.solve(max_pivots=budget)
            keys, present = eng.pricing_keys()
            assert present
            t = eng.tree()
            rc = cost + t["pi"][inst.tail] - t["pi"][inst.head]
            want = _vkey_code(-(t["state"].astype(np.int64)) * rc, bigm, 1 << (half_log2 or 28))
            assert np.array_equal(keys, want)
            sat_seen += int((keys == 0x7fffffff).sum())
        res, tree = eng.result(), eng.tree()
    with e.McfEngine(inst.n, inst.tail, inst.head, cost, inst.cap, inst.supply, compressed_keys=-1, **kw) as eng:
        assert not eng.pricing_keys()[1]
        eng.solve()
        ref, rtree = eng.result(), eng.tree()
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, cost, inst.cap, inst.supply, rule=rule)
    assert res.status == ref.status == "optimal" and res.stats["pivots"] == ref.stats["pivots"]
    assert np.array_equal(res.flow, ref.flow) and np.array_equal(res.potential, ref.potential)
    assert np.array_equal(tree["order"], rtree["order"])
    if rule == 0:
        assert res.stats["pivots"] == em["pivots"] and np.array_equal(res.flow, em["flow"])
    if variant in ("levels_narrow", "narrow"):
        assert sat_seen > 0                                         # the exact-compare path really ran


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("idx", [3, 6, 7], ids=["netgen256", "goto256", "netgen1024"])
def test_cycle_scan_equals_cycle_climb(gpu_engine_module, idx, rule):
    """The workgroup-wide scan over preorder positions (mcf_pivot_scan: ancestors found with the
    position-space subtree sizes, ratio test by team-wide atomics) against the one-lane parent-pointer
    climb: scan only, climb 3 then scan, climb only -- identical pivot sequence and tree, and identical
    to the CPU emulation."""
    _, inst = load_synthetic()[idx]
    # (the LDS-resident loop always climbs: kernel-per-phase path here, the persistent loop has its own test)
    runs = {cs: _solve(gpu_engine_module, inst, rule, cycle_scan=cs, climb_depth=-1, fused=False, mid_loop=-1) for cs in (-1, 1, 4)}
    r0, t0 = runs[-1]
    assert r0.stats["cycle_scans"] == 0 and (t0["psize"] == -1).all()      # sizes are not even kept
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, climb_budget=0)
    assert runs[1][0].stats["cycle_scans"] == em["scans"] > 0
    for cs in (1, 4):
        r, t = runs[cs]
        assert r.stats["cycle_scans"] > 0
        assert r.status == "optimal" and r.stats["pivots"] == r0.stats["pivots"] == em["pivots"]
        assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential)
        for key in ("order", "parent", "size", "pos", "depth"):
            assert np.array_equal(t[key], t0[key]), key
        assert np.array_equal(t["psize"], em["psize"])
        check_tree_invariants(inst.n, t["parent"], t["size"], t["pos"], t["order"], t["depth"], t["psize"])


def test_cycle_scan_on_a_deep_tree(gpu_engine_module):
    """goto-style grids grow spanning trees hundreds of arcs deep: the case the scan exists for.  Several
    chunk rounds per scan; the result must equal the climb's bit for bit."""
    inst = generators.goto_style(48, 48, seed=5)
    a, ta = _solve(gpu_engine_module, inst, 0, cycle_scan=-1)
    b, tb = _solve(gpu_engine_module, inst, 0, cycle_scan=1)
    c, tc = _solve(gpu_engine_module, inst, 0)                            # auto
    assert a.status == b.status == c.status == "optimal"
    assert a.stats["pivots"] == b.stats["pivots"] == c.stats["pivots"]
    assert b.stats["cycle_scans"] > 0 and b.stats["scan_rounds"] >= b.stats["cycle_scans"]
    for r, t in ((b, tb), (c, tc)):
        assert np.array_equal(r.flow, a.flow) and np.array_equal(r.potential, a.potential)
        assert np.array_equal(t["order"], ta["order"]) and np.array_equal(t["depth"], ta["depth"])
        check_tree_invariants(inst.n, t["parent"], t["size"], t["pos"], t["order"], t["depth"], t["psize"])


@pytest.mark.parametrize("rule", [0, 1], ids=["dantzig", "devex_block"])
@pytest.mark.parametrize("name,extra", [("netgen_8_12a", {}), ("gridgen_8_14a", {}), ("goto_8_14a", {"full_sweeps": -1}),
                                        ("netgen_8_14a", {"compressed_keys": 1, "full_sweeps": 1})],
                         ids=["netgen_8_12a", "gridgen_8_14a", "goto_8_14a_incremental", "netgen_8_14a_key_codes"])
def test_overlapped_graph_equals_sequential_graph(gpu_engine_module, name, extra, rule):
    """Captured graphs in which the pricing of pivot t+1 runs on a second stream beside the tree permutation of pivot t
    (it waits for the reduced-cost patch only): same pivots, flows, tree, reduced costs as the one-stream graph, also
    across budgets that end in the middle of a graph."""
    inst = generators.named_instance(name)
    e = gpu_engine_module
    kw = dict(rule=rule, fused=False, mid_loop=-1, **extra)
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, overlap_update=1, **kw) as eng:
        for budget in (1, 17, 1000):
            eng.solve(max_pivots=budget)
        assert eng.stats()["pivots"] == 1018 and eng.stats()["status"] == "iteration_limit"
        eng.solve()
        a, ta = eng.result(), eng.tree()
        rc, resident = eng.reduced_costs()
        assert resident and np.array_equal(rc, inst.cost + ta["pi"][inst.tail] - ta["pi"][inst.head])
    b, tb = _solve(e, inst, overlap_update=-1, **kw)
    assert a.status == b.status == "optimal" and a.objective == b.objective
    assert a.stats["pivots"] == b.stats["pivots"] and a.stats["degenerate"] == b.stats["degenerate"]
    assert a.stats["arcs_priced"] == b.stats["arcs_priced"]
    assert np.array_equal(a.flow, b.flow) and np.array_equal(a.potential, b.potential)
    for key in ("order", "parent", "size", "pos", "depth", "psize"):
        assert np.array_equal(ta[key], tb[key]), key


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("name", ["netgen_8_12a", "goto_8_12a"])
def test_persistent_loop_equals_kernel_per_phase_path(gpu_engine_module, name, rule):
    """k_solve_mid (one persistent workgroup does pricing of a block / re-pricing of the list, pivot, tree update
    and reduced-cost update with the state in global memory) against the k_price_rc -> k_pivot -> k_update
    launches: same pivots, same flows, same tree, resident reduced costs still exact; budgets and resumes land
    on the same pivot counts."""
    inst = generators.named_instance(name)
    e = gpu_engine_module
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, mid_loop=1) as eng:
        for budget in (1, 17, 1000):
            eng.solve(max_pivots=budget)
        assert eng.stats()["pivots"] == 1018 and eng.stats()["status"] == "iteration_limit"
        eng.solve()
        a, ta = eng.result(), eng.tree()
        rc, resident = eng.reduced_costs()
        assert resident and np.array_equal(rc, inst.cost + ta["pi"][inst.tail] - ta["pi"][inst.head])
    b, tb = _solve(e, inst, rule, mid_loop=-1)
    assert a.stats["pricing_mode"] == 3 and b.stats["pricing_mode"] == 1
    assert a.status == b.status == "optimal" and a.objective == b.objective
    assert a.stats["pivots"] == b.stats["pivots"] and a.stats["degenerate"] == b.stats["degenerate"]
    assert a.stats["arcs_priced"] == b.stats["arcs_priced"]
    assert np.array_equal(a.flow, b.flow) and np.array_equal(a.potential, b.potential)
    for key in ("order", "parent", "size", "pos", "depth", "psize"):
        assert np.array_equal(ta[key], tb[key]), key
    check_optimality(inst, a.flow, a.potential)


@pytest.mark.parametrize("rule", [0, 2], ids=["dantzig", "candidate_list"])
@pytest.mark.parametrize("name", ["netgen_8_12a", "gridgen_8_14a"])
def test_incremental_sweeps_select_the_same_arcs(gpu_engine_module, name, rule):
    """A pricing workgroup whose arcs have not changed since it last swept them keeps its candidate (the resident
    reduced costs make "changed" exact: the arcs k_update patches + the entering / leaving arc).  The entering arc
    is still the arg-max over ALL arcs: same pivot sequence as with full sweeps, a fraction of the arcs read."""
    inst = generators.named_instance(name)
    full, tf = _solve(gpu_engine_module, inst, rule, full_sweeps=1, mid_loop=-1)
    inc, ti = _solve(gpu_engine_module, inst, rule, full_sweeps=-1, mid_loop=-1)
    assert full.status == inc.status == "optimal" and full.objective == inc.objective
    assert full.stats["pivots"] == inc.stats["pivots"] and full.stats["arcs_priced"] == inc.stats["arcs_priced"]
    assert np.array_equal(full.flow, inc.flow) and np.array_equal(full.potential, inc.potential)
    assert np.array_equal(tf["order"], ti["order"]) and np.array_equal(tf["parent"], ti["parent"])
    assert full.stats["arcs_swept"] >= full.stats["arcs_priced"] * 0.95       # (block slices overlap by < one group of 4)
    assert inc.stats["arcs_swept"] <= full.stats["arcs_swept"]
    if rule == 0 and name == "gridgen_8_14a":                     # 64 pricing workgroups, small re-hung subtrees
        assert inc.stats["arcs_swept"] < 0.7 * full.stats["arcs_swept"]


def test_cycle_scan_above_65535_nodes(gpu_engine_module):
    """70 000 nodes (several scan rounds per pivot): scan vs climb after 6 000 pivots, and both against the CPU
    emulation."""
    inst = generators.netgen_style(70000, 280000, seed=3)
    e = gpu_engine_module
    out = {}
    for cs in (-1, 0):
        with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, cycle_scan=cs) as eng:
            eng.solve(max_pivots=6000)
            out[cs] = (eng.result(), eng.tree())
    (a, ta), (b, tb) = out[-1], out[0]
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, max_pivots=6000, climb_budget=0)
    assert a.stats["pivots"] == b.stats["pivots"] == em["pivots"] == 6000 and b.stats["cycle_scans"] > 0
    assert np.array_equal(a.flow, b.flow) and np.array_equal(b.flow, em["flow"]) and np.array_equal(b.potential, em["potential"])
    for key in ("order", "parent", "size", "depth"):
        assert np.array_equal(ta[key], tb[key]) and np.array_equal(tb[key], em[key]), key
    assert np.array_equal(tb["psize"], em["psize"]) and tb["psize"][0] == inst.n + 1
    check_tree_invariants(inst.n, tb["parent"], tb["size"], tb["pos"], tb["order"], tb["depth"], tb["psize"])


@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("full_sweeps", [1, -1], ids=["full_sweeps", "incremental_sweeps"])
def test_sharded_kernels_on_one_gpu(gpu_engine_module, rule, full_sweeps):
    """The arc-sharded multi-GPU kernels on real hardware without RCCL: three handles on this GPU, each pricing its
    third of every bucket (options.shard_rank / shard_count); per pivot mcf_enqueue_price on each, the three 16-byte
    candidates put side by side (what the all-gather does), mcf_enqueue_pivot on each.  The replicas must stay
    bit-identical, and -- Dantzig / Devex -- pivot exactly like the unsharded engine."""
    import ctypes

    e = gpu_engine_module
    inst = generators.named_instance("netgen_8_10a")
    G = 3
    engs = [e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, shard=(r, G), device=0,
                        full_sweeps=full_sweeps) for r in range(G)]
    # plain HIP for the candidate buffers (the runtime libmcf_hip.so already loaded; torch's own copy of it cannot be
    # initialised in the same process afterwards)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    buf = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(buf), 32 * G) == 0 and hip.hipMemset(buf, 0, 32 * G) == 0
    local = [buf.value + 16 * r for r in range(G)]          # one 16-byte candidate per rank ...
    gathered = buf.value + 16 * G                            # ... and the gathered list
    try:
        for eng in engs:
            eng.set_max_pivots(10 ** 9)
        done = False
        for _batch in range(4000):
            for _ in range(32):
                for r, eng in enumerate(engs):
                    eng.enqueue_price(0, local[r])
                assert hip.hipMemcpyAsync(gathered, buf.value, 16 * G, 3, None) == 0   # device to device, null stream
                for eng in engs:
                    eng.enqueue_pivot(0, gathered, G)
            assert hip.hipDeviceSynchronize() == 0
            polls = [eng.poll() for eng in engs]
            assert len(set(polls)) == 1                      # same status, same pivot count on every replica
            if polls[0][0] is not None:
                done = True
                break
        assert done
        results = [(eng.result(), eng.tree()) for eng in engs]
    finally:
        for eng in engs:
            eng.close()
        hip.hipFree(buf)
    r0, t0 = results[0]
    assert r0.status == "optimal"
    for r, t in results[1:]:
        assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential)
        assert np.array_equal(t["order"], t0["order"]) and np.array_equal(t["parent"], t0["parent"])
    single, ts = _solve(e, inst, rule, fused=False, mid_loop=-1)
    assert single.objective == r0.objective
    check_optimality(inst, r0.flow, r0.potential)
    if rule != 2:   # candidate list: sharded, the list holds one entry per rank instead of one per pricing workgroup
        assert single.stats["pivots"] == r0.stats["pivots"]
        assert np.array_equal(single.flow, r0.flow) and np.array_equal(ts["order"], t0["order"])


@pytest.mark.parametrize("full_sweeps", [1, -1], ids=["full_sweeps", "incremental_sweeps"])
def test_sharded_candidate_lists_on_one_gpu(gpu_engine_module, full_sweeps):
    """The amortised multi-GPU protocol on real hardware without RCCL: three handles on this GPU; per round
    mcf_enqueue_price_list on each (its shard's per-workgroup candidates), the three lists put side by side (what the
    ONE all-gather per round does), then mcf_enqueue_pivots: minor_cap + 1 pivots that re-price the gathered list.
    Replicas stay bit-identical; every rank's resident reduced costs stay exact on ITS shard (the rank's patch walks only
    its own adjacency); the result is the certified optimum; collectives per pivot ~ 1 / (minor_cap + 1)."""
    import ctypes

    e = gpu_engine_module
    inst = generators.named_instance("netgen_8_10a")
    G = 3
    engs = [e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2, shard=(r, G), device=0,
                        full_sweeps=full_sweeps) for r in range(G)]
    infos = [eng.shard_info() for eng in engs]
    assert len(set(infos)) == 1
    K, minor_cap = infos[0]
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    buf = ctypes.c_void_p()
    nbytes = 16 * K * G
    assert hip.hipMalloc(ctypes.byref(buf), 2 * nbytes) == 0 and hip.hipMemset(buf, 0xff, 2 * nbytes) == 0
    local = [buf.value + 16 * K * r for r in range(G)]
    gathered = buf.value + nbytes
    rounds = 0
    try:
        for eng in engs:
            eng.set_max_pivots(10 ** 9)
        done = False
        for _batch in range(4000):
            for _ in range(4):
                for r, eng in enumerate(engs):
                    eng.enqueue_price_list(0, local[r])
                assert hip.hipMemcpyAsync(gathered, buf.value, nbytes, 3, None) == 0
                for eng in engs:
                    eng.enqueue_pivots(0, gathered, K * G, minor_cap + 1)
                rounds += 1
            assert hip.hipDeviceSynchronize() == 0
            polls = [eng.poll() for eng in engs]
            assert len(set(polls)) == 1
            if _batch == 3:                                   # mid-solve: each rank's own shard of reduced costs is exact
                pi = engs[0].tree()["pi"]
                truth = inst.cost + pi[inst.tail] - pi[inst.head]
                for eng in engs:
                    rc, resident = eng.reduced_costs()
                    assert resident and np.array_equal(rc, truth)
            if polls[0][0] is not None:
                done = True
                break
        assert done
        results = [(eng.result(), eng.tree()) for eng in engs]
    finally:
        for eng in engs:
            eng.close()
        hip.hipFree(buf)
    r0, t0 = results[0]
    assert r0.status == "optimal"
    for r, t in results[1:]:
        assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential)
        assert np.array_equal(t["order"], t0["order"]) and np.array_equal(t["parent"], t0["parent"])
    single, _ = _solve(e, inst, 2, fused=False, mid_loop=-1)
    assert single.objective == r0.objective
    check_optimality(inst, r0.flow, r0.potential)
    assert r0.stats["pivots"] >= 2 * rounds                  # several pivots per collective, not one


def _chain_instance(n, skip=7):
    """A path 0 -> 1 -> ... -> n-1 with capacity 10, shortcut arcs every `skip` nodes and one expensive direct
    arc; 15 units from 0 to n-1.  The optimal tree is essentially the path: cycles thousands of arcs long (the
    reference's long-chain graphs, tests/test_large_directed.py:14-128, scaled up)."""
    tail = list(range(n - 1)) + list(range(0, n - skip, skip)) + [0]
    head = list(range(1, n)) + list(range(skip, n, skip))[: len(range(0, n - skip, skip))] + [n - 1]
    m1, m2 = n - 1, len(range(0, n - skip, skip))
    cost = [1] * m1 + [skip + 2] * m2 + [3 * n]
    cap = [10] * m1 + [4] * m2 + [100]
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = 15, -15
    return generators.ArcSoA(n=n, tail=np.array(tail, np.int32), head=np.array(head, np.int32), cost=np.array(cost, np.int64),
                             cap=np.array(cap, np.int64), supply=supply, name=f"chain_{n}")


@pytest.mark.parametrize("mid_loop", [-1, 1], ids=["kernel_per_phase", "persistent_loop"])
def test_cycle_scan_with_cycles_longer_than_the_lds_buffers(gpu_engine_module, mid_loop):
    """12 000-node chain: cycles of ~6 000 arcs overflow the LDS hit list (4 096 entries) and the LDS path
    buffers (512), so the spill list and the global path scratch are exercised; several scan rounds per pivot.
    Pivot for pivot against the CPU emulation."""
    inst = _chain_instance(12000)
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, climb_budget=0)
    assert em["status"] == "optimal" and em["cycle_arcs"] / em["pivots"] > 4096
    res, tree = _solve(gpu_engine_module, inst, 0, mid_loop=mid_loop, climb_depth=-1)
    assert res.status == "optimal" and res.objective == em["objective"]
    assert res.stats["pivots"] == em["pivots"] and res.stats["cycle_arcs"] == em["cycle_arcs"]
    assert res.stats["cycle_scans"] == em["scans"]
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"])
    for key in ("order", "parent", "size", "depth", "psize"):
        assert np.array_equal(tree[key], em[key]), key
    check_optimality(inst, res.flow, res.potential)


# ------------------------------------------------------------------ golden fixtures, through the reference-shaped API
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("strategy", ["dantzig", "devex", "adaptive", "candidate_list"])
def test_small_cases_through_the_shim(gpu_engine_module, case, strategy):
    exp = case["expected"]["dantzig" if strategy == "dantzig" else "devex"]
    problem = nfs.build_problem(case["nodes"], case["arcs"], case["directed"], case["tolerance"])
    opts = nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True)
    if exp["status"] == "unbounded":
        with pytest.raises(nfs.UnboundedProblemError, match="Unbounded problem detected") as ei:
            nfs.solve_min_cost_flow(problem, opts)
        assert ei.value.entering_arc in {("A", "B"), ("B", "A")} and ei.value.reduced_cost < 0
        return
    res = nfs.solve_min_cost_flow(problem, opts, max_iterations=case.get("max_iterations"))
    assert res.status == exp["status"]
    assert res.objective == pytest.approx(exp["objective"], abs=1e-9)
    if exp["status"] == "infeasible":
        assert res.flows == {} and res.duals == {} and res.objective == 0.0
        return
    ref = oracle.solve_dicts(case["nodes"], case["arcs"], case["directed"], case["tolerance"], "dantzig")
    if ref.min_nonbasic_abs_rc > 1e-6:        # unique optimum: flows must be the reference's
        assert res.flows == golden_flows(exp)
    else:                                      # alternative optima: feasible + same cost is the bar
        bal = {str(nd["id"]): float(nd.get("supply", 0.0)) for nd in case["nodes"]}
        for (t, h), f in res.flows.items():
            bal[t] -= f
            bal[h] += f
        assert all(abs(v) <= 1e-9 for v in bal.values())
    assert set(res.duals) == {str(nd["id"]) for nd in case["nodes"]}
    assert res.basis is not None and all(k in {(a["tail"], a["head"]) for a in case["arcs"]} for k in res.basis.tree_arcs)


# ------------------------------------------------------------------ randomised API-level parity
@pytest.mark.parametrize("seed", list(range(0, 160, 2)))
def test_random_problems_through_the_shim(gpu_engine_module, seed):
    """Negative costs, zero / unlimited capacities, lower bounds, parallel arcs, undirected edges,
    fractional data, infeasible demands -- through solve_min_cost_flow on the GPU, against an
    independent exact solve (networkx) and the oracle wherever the reference is self-consistent
    (see tests/test_random_cpu.py for the two reference defects this input family exposes)."""
    from random_instances import make
    from test_random_cpu import networkx_truth

    nodes, arcs, directed = make(seed)
    problem = nfs.build_problem(nodes, arcs, directed, 1e-6)
    truth_status, truth_obj = networkx_truth(problem)
    for strategy in ("dantzig", "devex"):
        opts = nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True)
        if truth_status == "unbounded":
            with pytest.raises(nfs.UnboundedProblemError):
                nfs.solve_min_cost_flow(problem, opts)
            continue
        res = nfs.solve_min_cost_flow(problem, opts)
        assert res.status == truth_status
        if truth_status == "infeasible":
            assert res.flows == {} and res.objective == 0.0
            continue
        assert res.objective == pytest.approx(truth_obj, abs=1e-7)
        # feasibility of the reported flows in the caller's terms (bounds + conservation)
        bal = {nd["id"]: nd["supply"] for nd in nodes}
        by_key = {}
        for a in arcs:
            by_key.setdefault((a["tail"], a["head"]), []).append(a)
        for (t, h), f in res.flows.items():
            lo = sum((-x["capacity"] if not directed else x["lower"]) for x in by_key[(t, h)])
            hi = sum((float("inf") if x["capacity"] is None else x["capacity"]) for x in by_key[(t, h)])
            assert lo - 1e-9 <= f <= hi + 1e-9
            bal[t] -= f
            bal[h] += f
        assert all(abs(v) <= 1e-9 for v in bal.values())
    ref = oracle.solve_dicts(nodes, arcs, directed, 1e-6, "dantzig")
    refx = oracle.solve_dicts(nodes, arcs, directed, 1e-6, "devex")
    if ref.status == refx.status == "optimal":
        assert ref.objective == pytest.approx(truth_obj, abs=1e-7)


def test_solver_adapter_on_gpu(gpu_engine_module):
    from network_flow_solver_amd.adapter import Mi355xAdapter

    assert Mi355xAdapter.is_available()
    for name, want in (("sample_problem", 15.0), ("textbook_transport", 85.0), ("infeasible_capacity_starved", None)):
        case = next(c for c in CASES if c["name"] == name)
        res = Mi355xAdapter.solve(nfs.build_problem(case["nodes"], case["arcs"], case["directed"], case["tolerance"]))
        if want is None:
            assert res.status == "infeasible" and res.objective is None
        else:
            assert res.status == "optimal" and res.objective == pytest.approx(want) and res.iterations > 0
    case = next(c for c in CASES if c["name"] == "unbounded_cycle")
    res = Mi355xAdapter.solve(nfs.build_problem(case["nodes"], case["arcs"], True, 1e-9))
    assert res.status == "unbounded"


# ------------------------------------------------------------------ fresh seeds vs the oracle
@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("family", ["netgen", "gridgen", "goto"])
def test_fresh_instances_match_oracle(gpu_engine_module, family, seed):
    inst = {"netgen": lambda: generators.netgen_style(200, 1600, seed),
            "gridgen": lambda: generators.gridgen_style(12, 12, seed),
            "goto": lambda: generators.goto_style(12, 12, seed)}[family]()
    ref = oracle.solve_soa(inst, "dantzig")
    for rule in RULES:
        res, _ = _solve(gpu_engine_module, inst, rule)
        assert res.status == ref["status"] == "optimal"
        assert res.objective == int(round(ref["objective"]))
        rc = check_optimality(inst, res.flow, res.potential)
        if optimum_is_unique(inst, res.flow, res.in_tree, rc):
            assert np.array_equal(res.flow, np.round(ref["flow"]).astype(np.int64))


# ------------------------------------------------------------------ kernel-level parity: one pricing pass
def test_pricing_kernel_matches_reference_rule(gpu_engine_module):
    """mcf_price_once (Dantzig) vs the restated DantzigPricing.select_entering_arc on the same
    state, at several points of a solve (start basis, mid-solve, optimum)."""
    _, inst = load_synthetic()[3]
    cap = inst.cap.astype(np.float64)
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0) as eng:
        for budget in (0, 1, 7, 50, 200, 100000):
            if budget:
                eng.solve(max_pivots=budget)
            r = eng.result()
            t = eng.tree()
            got = eng.price_once(0)
            flow = r.flow.astype(np.float64)
            pick = oracle.price_dantzig(inst.tail, inst.head, inst.cost.astype(np.float64),
                                        t["pi"][: inst.n].astype(np.float64), cap - flow, flow,
                                        (t["state"] == 0).astype(np.uint8))
            if pick is None:
                assert got is None and r.status == "optimal"
            else:
                assert got is not None and (got[0], got[1]) == pick
                rc = inst.cost[got[0]] + t["pi"][inst.tail[got[0]]] - t["pi"][inst.head[got[0]]]
                assert got[2] == abs(int(rc))
            # sub-range pricing (block / shard boundaries, unaligned on purpose)
            lo, hi = 37, inst.m - 113
            sub = eng.price_once(0, lo, hi)
            viol = -(t["state"].astype(np.int64)) * (inst.cost + t["pi"][inst.tail] - t["pi"][inst.head])
            viol[:lo] = 0
            viol[hi:] = 0
            if viol.max() <= 0:
                assert sub is None
            else:
                assert sub[0] == int(np.argmax(viol)) and sub[2] == int(viol.max())


def _tie_rich_instance(seed: int, n: int = 48, m: int = 420):
    """Few distinct costs and unit-ish capacities: equal |rc| on many arcs (merit ties, in both directions)."""
    rng = np.random.default_rng(seed)
    tail = rng.integers(0, n, m).astype(np.int32)
    head = ((tail + 1 + rng.integers(0, n - 1, m)) % n).astype(np.int32)
    cost = rng.integers(1, 4, m).astype(np.int64)
    cap = rng.integers(1, 3, m).astype(np.int64)
    ring = np.arange(n, dtype=np.int32)                           # feasibility skeleton: a cheap uncapacitated ring
    tail = np.concatenate((tail, ring)); head = np.concatenate((head, (ring + 1) % n))
    cost = np.concatenate((cost, np.full(n, 3, np.int64))); cap = np.concatenate((cap, np.full(n, -1, np.int64)))
    supply = np.zeros(n, np.int64)
    src = rng.choice(n, 6, replace=False)
    supply[src[:3]] = [4, 3, 2]; supply[src[3:]] = [-2, -3, -4]
    return generators.ArcSoA(n, tail, head, cost, cap, supply, f"tie_rich_{seed}")


def _devex_block_reference(inst, res, tree, weights, lo, hi):
    """The restated NetworkSimplex._select_entering_arc_vectorized (simplex.py:528-617) on the engine's state."""
    cap = inst.cap.astype(np.float64)
    cap[inst.cap < 0] = np.inf
    flow = res.flow.astype(np.float64)
    return oracle.price_block(inst.tail, inst.head, inst.cost.astype(np.float64), tree["pi"][: inst.n].astype(np.float64),
                              cap - flow, flow, (tree["state"] == 0).astype(np.uint8), weights.astype(np.float64), lo, hi)


@pytest.mark.parametrize("which", ["netgen256", "netgen1024", "tie_rich_3", "tie_rich_5", "tie_rich_8"])
def test_devex_kernel_matches_reference_block_selection(gpu_engine_module, which):
    """Kernel-level Devex parity: mcf_price_once(rule = Devex, start, end) against the oracle's restatement of the
    reference's vectorised block selection on IDENTICAL state and weights, at several stages of a Devex solve:
    arc, direction and the merit's bit pattern.  The tie-rich instances make equal merits common, so the
    reference's tie rules are exercised: first maximum per direction (lowest index) and forward only when
    strictly greater (a backward arc wins a forward/backward tie even with a higher index)."""
    inst = {"netgen256": lambda: load_synthetic()[3][1], "netgen1024": lambda: load_synthetic()[7][1]}.get(
        which, lambda: _tie_rich_instance(int(which.rsplit("_", 1)[1])))()
    m = inst.m
    ranges = [(0, m), (0, m // 3), (m // 3, m - 7), (17, 17 + max(8, m // 16)), (m - 40, m)]
    same_dir_ties = cross_dir_ties = checked = 0
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=1) as eng:
        for budget in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 10 ** 9):
            if budget:
                eng.solve(max_pivots=budget)
            res, tree, w = eng.result(), eng.tree(), eng.weights()
            assert (w >= 1).all()
            rc = inst.cost + tree["pi"][inst.tail] - tree["pi"][inst.head]
            viol = (-(tree["state"].astype(np.int64)) * rc).astype(np.float64)
            viol[inst.cap == 0] = 0                                 # (no residual either way: never eligible in the reference)
            merit = np.where(viol > 0, viol * viol / w.astype(np.float64), 0.0)
            for lo, hi in ranges:
                got = eng.price_once(1, lo, hi)
                exp = _devex_block_reference(inst, res, tree, w, lo, hi)
                if exp is None:
                    assert got is None
                    continue
                assert got is not None, (budget, lo, hi, exp)
                got_merit = np.frombuffer(np.int64(got[2]).tobytes(), dtype=np.float64)[0]
                assert (got[0], got[1]) == (exp[0], exp[1]), (budget, lo, hi, got, exp)
                assert got_merit == exp[2] and np.int64(got[2]) == np.float64(exp[2]).view(np.int64)   # bit pattern
                checked += 1
                top = np.nonzero(merit[lo:hi] == exp[2])[0] + lo    # every arc of the range that attains the maximum
                if len(top) > 1:
                    dirs = set(int(tree["state"][i]) for i in top)
                    if len(dirs) == 2:
                        cross_dir_ties += 1
                        assert exp[1] == -1                          # the backward arc wins ...
                        assert exp[0] == min(i for i in top if tree["state"][i] < 0)   # ... the lowest-index one
                    else:
                        same_dir_ties += 1
                        assert exp[0] == top.min()
            if res.status == "optimal":
                break
    assert checked >= 10
    if which.startswith("tie_rich"):
        assert same_dir_ties > 0                                    # the tie rules were really exercised


def test_devex_forward_backward_tie_prefers_the_backward_arc(gpu_engine_module):
    """A forward and a backward candidate with the same merit: the reference's vectorised selection takes the
    backward one (forward wins only when strictly greater, simplex.py:596) although its index is higher; the
    Dantzig loop takes the first index (simplex_pricing.py:126).  The state is installed with mcf_set_basis:
    tree 3 -> 2 -> 1 -> 0 (zero-cost-1 arcs pointing at the root), arc 3 = (3, 0) at its lower bound with
    rc = -2, arc 4 = (0, 3) at its upper bound with rc = +2."""
    e = gpu_engine_module
    tail = np.array([1, 2, 3, 3, 0], np.int32)
    head = np.array([0, 1, 2, 0, 3], np.int32)
    cost = np.array([1, 1, 1, 1, -1], np.int64)
    cap = np.array([-1, -1, -1, 5, 2], np.int64)
    supply = np.zeros(4, np.int64)
    inst = generators.ArcSoA(4, tail, head, cost, cap, supply, "fwd_bwd_tie")
    for kw in ({}, {"fused": False}, {"fused": False, "mid_loop": -1}, {"fused": False, "resident_rc": False}):
        with e.McfEngine(4, tail, head, cost, cap, supply, rule=1, **kw) as eng:
            assert eng.set_basis([1, 1, 1, 0, 0], [0, 0, 0, 0, 1])
            res, tree, w = eng.result(), eng.tree(), eng.weights()
            assert res.flow.tolist() == [2, 2, 2, 0, 2] and (w == 1).all()
            rc = cost + tree["pi"][tail] - tree["pi"][head]
            assert rc.tolist() == [0, 0, 0, -2, 2] and tree["state"].tolist() == [0, 0, 0, 1, -1]
            exp = _devex_block_reference(inst, res, tree, w, 0, 5)
            assert exp == (4, -1, 4.0)
            got = eng.price_once(1)
            assert (got[0], got[1]) == (4, -1) and np.int64(got[2]) == np.float64(4.0).view(np.int64)
            assert eng.price_once(1, 0, 4)[:2] == (3, 1)              # without the backward arc in range
            assert eng.price_once(0)[:2] == (3, 1)                     # Dantzig: first index among equal violations
            eng.solve()
            assert eng.result().status == "optimal" and eng.result().objective == 0


def test_devex_pivot_counts_close_to_the_reference(gpu_engine_module):
    """configs[2]'s rule must not be less efficient than the reference's own Devex: on the Devex goldens (pivot
    counts produced by running the reference) the engine takes at most 1.2x as many pivots for the same optimum.
    (Round 1 took 2.4x on netgen_8_12a: no weight reset, no tuner.)"""
    for entry, inst in load_synthetic():
        exp = entry["expected"].get("devex")
        if not exp or "iterations" not in exp:
            continue
        res, _ = _solve(gpu_engine_module, inst, 1)
        assert res.status == "optimal" and res.objective == int(round(exp["objective"]))
        assert res.stats["pivots"] <= 1.2 * exp["iterations"], (entry["name"], res.stats["pivots"], exp["iterations"])


@pytest.mark.parametrize("rule", [0, 2], ids=["dantzig", "candidate_list"])
def test_forward_first_keys_on_every_engine_path(gpu_engine_module, rule):
    """options.forward_first (the reference's min-cost rule for assignment problems, specialized_pivots.py:191-223:
    forward candidates before backward ones): every engine path pivots exactly like the CPU emulation with the same
    key, takes a different route than the plain rule, and ends at the same optimum."""
    for idx, kws in ((3, ({}, {"fused": False}, {"fused": False, "mid_loop": -1})), (7, ({}, {"mid_loop": -1}, {"resident_rc": False}))):
        _, inst = load_synthetic()[idx]
        em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule | 0x100)
        plain, _ = _solve(gpu_engine_module, inst, rule)
        for kw in kws:
            res, tree = _solve(gpu_engine_module, inst, rule, forward_first=True, **kw)
            assert res.status == "optimal" and res.objective == em["objective"] == plain.objective
            assert res.stats["pivots"] == em["pivots"] and np.array_equal(res.flow, em["flow"])
            assert np.array_equal(tree["order"], em["order"])
        assert em["pivots"] != plain.stats["pivots"]
    # the key bit never leaks through the parity hook
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, forward_first=True) as eng:
        got = eng.price_once(0)
        pi = eng.tree()["pi"]
        assert got[2] == abs(int(inst.cost[got[0]] + pi[inst.tail[got[0]]] - pi[inst.head[got[0]]]))


@pytest.mark.parametrize("rule", [0, 2], ids=["dantzig", "candidate_list"])
@pytest.mark.parametrize("mode", ["priority", "capacity"])
def test_key_variants_on_every_engine_path(gpu_engine_module, rule, mode):
    """mcf_options.key_mode 2 / 3 (the reference's shortest-path / bipartite-matching preference classes and its max-flow
    merit capacity x violation, specialized_pivots.py:233-424, as keys of the one sweep): every engine path pivots
    exactly like the CPU emulation with the same key and ends at the plain rule's optimum."""
    e = gpu_engine_module
    for idx, kws in ((3, ({}, {"fused": False}, {"fused": False, "mid_loop": -1})), (7, ({}, {"mid_loop": -1}, {"resident_rc": False}))):
        _, inst = load_synthetic()[idx]
        rng = np.random.default_rng(idx)
        prio = rng.integers(0, 4, size=inst.m).astype(np.int8) if mode == "priority" else None
        key_mode = e.KEY_PRIORITY if mode == "priority" else e.KEY_CAPACITY
        em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule | (key_mode << 8), arc_priority=prio)
        plain, _ = _solve(e, inst, rule)
        for kw in kws:
            res, tree = _solve(e, inst, rule, key_mode=key_mode, arc_priority=prio, **kw)
            assert res.status == "optimal" and res.objective == em["objective"] == plain.objective
            assert res.stats["pivots"] == em["pivots"] and np.array_equal(res.flow, em["flow"])
            assert np.array_equal(tree["order"], em["order"])
        assert em["pivots"] != plain.stats["pivots"]
    # one selection against a direct restatement of the two keys
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, key_mode=key_mode, arc_priority=prio,
                     fused=False, mid_loop=-1) as eng:
        eng.solve(max_pivots=50)
        res, pi = eng.result(), eng.tree()["pi"]
        rc = inst.cost + pi[inst.tail] - pi[inst.head]
        at_upper = ~res.in_tree & (inst.cap > 0) & (res.flow == inst.cap)
        state = np.where(res.in_tree | (inst.cap == 0), 0, np.where(at_upper, -1, 1))
        viol = -state * rc
        elig = viol > 0
        if mode == "priority":
            merit = np.where(elig, viol.astype(np.int64) + ((prio & np.where(state > 0, 1, 2)) != 0).astype(np.int64) * (1 << 61), -1)
        else:
            merit = np.where(elig, np.where(inst.cap < 0, np.inf, inst.cap.astype(np.float64)) * viol, -1.0)
        got = eng.price_once(0)
        assert merit[got[0]] == merit.max() and got[0] == int(np.flatnonzero(merit == merit.max())[0])


def _structured_instances():
    """(kind, nodes, arcs, what the reference itself returned) of tests/golden/structured_cases.json."""
    data = json.loads((Path(__file__).parent / "golden" / "structured_cases.json").read_text())
    return [(c["network_type"], c["nodes"], c["arcs"], c["expected"]) for c in data]


def test_the_shim_maps_every_structured_class_to_its_key(gpu_engine_module):
    """Shortest-path, bipartite-matching and max-flow problems through the shim: the structure analysis agrees with the
    restated reference classification, selects the key variant (specialized_pivots.py:452-527), and the optimum equals
    the one the restated reference (with ITS specialised strategy) reaches.  The reference's own fixtures of these
    classes (an unbounded cycle, a capacity-starved instance) keep their outcome."""
    e = gpu_engine_module
    want = {"shortest_path": e.KEY_PRIORITY, "bipartite_matching": e.KEY_PRIORITY, "max_flow": e.KEY_CAPACITY, "assignment": e.KEY_FORWARD_FIRST}
    for kind, nodes, arcs, expected in _structured_instances():
        assert oracle.detect_network_type(nodes, arcs, True, 1e-6)[0] == kind
        ref = oracle.solve_dicts(nodes, arcs, True, 1e-6, "devex", max_iterations=2000)
        assert (ref.status, ref.iterations) == (expected["devex"]["status"], expected["devex"]["iterations"])
        if kind == "bipartite_matching":
            # the reference's matching heuristic enters the first arc out of an unmatched node whatever its reduced cost
            # (:253-281) and runs into the iteration limit on a real matching instance (the fixture holds what the
            # reference itself returned; the oracle reproduces it); the optimum to meet is the general rule's
            assert ref.status == "iteration_limit"
            ref = oracle.solve_dicts(nodes, arcs, True, 1e-6, "devex", special=oracle.SPECIAL_TYPES["general"])
        assert ref.status == "optimal"
        for strategy in ("devex", "dantzig"):
            problem = nfs.build_problem(nodes, arcs, True, 1e-6)
            solver = nfs.NetworkSimplex(problem, nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True))
            try:
                assert solver.network_structure.network_type.value == kind
                assert solver.pricing_rule == e.RULE_DANTZIG and solver.engine.key_mode == want[kind]
                res = solver.solve()
            finally:
                solver.engine.close()
            assert res.status == "optimal" and res.objective == pytest.approx(ref.objective, abs=1e-9)
            if ref.min_nonbasic_abs_rc is not None and ref.min_nonbasic_abs_rc > 1e-9:     # unique optimum: same flows
                assert {k: v for k, v in res.flows.items() if abs(v) > 1e-9} == pytest.approx(ref.flows)
    seen = set()
    for case in CASES:
        if case["network_type"] not in want:
            continue
        exp = case["expected"]["devex"]
        problem = nfs.build_problem(case["nodes"], case["arcs"], case["directed"], case["tolerance"])
        solver = nfs.NetworkSimplex(problem, nfs.SolverOptions(pricing_strategy="devex", explicit_pricing_strategy=True))
        try:
            assert solver.network_structure.network_type.value == case["network_type"]
            assert solver.engine.key_mode == want[case["network_type"]]
            if exp["status"] == "unbounded":
                with pytest.raises(nfs.UnboundedProblemError):
                    solver.solve()
            else:
                res = solver.solve()
                assert res.status == exp["status"] and res.objective == pytest.approx(exp["objective"], abs=1e-9)
        finally:
            solver.engine.close()
        seen.add(case["network_type"])
    assert seen == set(want)


def test_structured_problems_take_the_specialised_rules(gpu_engine_module):
    """Transportation and assignment fixtures through the shim: the structure analysis picks the row-scan (Dantzig)
    and the forward-first rule whatever strategy was asked for, and the reference's optimum comes back."""
    from network_flow_solver_amd.specializations import NetworkType

    seen = set()
    for case in CASES:
        if case["network_type"] not in ("transportation", "assignment"):
            continue
        exp = case["expected"]["devex"]
        problem = nfs.build_problem(case["nodes"], case["arcs"], case["directed"], case["tolerance"])
        solver = nfs.NetworkSimplex(problem, nfs.SolverOptions(pricing_strategy="devex", explicit_pricing_strategy=True))
        try:
            assert solver.network_structure.network_type.value == case["network_type"]
            assert solver.pricing_rule == gpu_engine_module.RULE_DANTZIG
            res = solver.solve()
        finally:
            solver.engine.close()
        assert res.status == exp["status"] and res.objective == pytest.approx(exp["objective"], abs=1e-9)
        seen.add(solver.network_structure.network_type)
    assert seen == {NetworkType.TRANSPORTATION, NetworkType.ASSIGNMENT}


def test_sharded_handle_refuses_a_standalone_solve(gpu_engine_module):
    """A handle that prices 1/G of the arcs must not be solved on its own (it would call its share's optimum
    the optimum): mcf_solve returns MCF_E_STATE."""
    _, inst = load_synthetic()[3]
    e = gpu_engine_module
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, shard=(1, 2)) as eng:
        with pytest.raises(e.EngineError) as err:
            eng.solve()
        assert err.value.code == -6 and "shard_count" in str(err.value)


@pytest.mark.parametrize("idx", [3, 7], ids=["fused_lds_path", "kernel_path"])
def test_candidate_list_survives_budget_and_resume(gpu_engine_module, idx):
    """The candidate list lives on the device between solve() calls (and is not clobbered by the
    re-pricing at a budget limit or by mcf_price_once), so a solve cut into pieces takes the very
    same pivots as an uninterrupted one."""
    _, inst = load_synthetic()[idx]
    e = gpu_engine_module
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2) as eng:
        eng.solve()
        whole = eng.result()
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2) as eng:
        for budget in (1, 1, 3, 10, 57):
            eng.solve(max_pivots=budget)
            eng.price_once(0)
        eng.solve()
        pieces = eng.result()
    assert whole.status == pieces.status == "optimal"
    assert pieces.stats["pivots"] == whole.stats["pivots"] and np.array_equal(pieces.flow, whole.flow)
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2)
    assert whole.stats["pivots"] == em["pivots"] and whole.stats["arcs_priced"] == em["arcs_priced"]


# ------------------------------------------------------------------ solve-control edge cases
def test_pivot_budget_resume_and_reset(gpu_engine_module):
    _, inst = load_synthetic()[3]
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0) as eng:
        eng.solve(max_pivots=10)
        r = eng.result()
        assert r.status == "iteration_limit" and r.stats["pivots"] == 10
        eng.solve(max_pivots=25)
        assert eng.result().stats["pivots"] == 35
        eng.solve()
        full = eng.result()
        assert full.status == "optimal"
        eng.reset()
        assert eng.result().stats["pivots"] == 0
        eng.solve()
        again = eng.result()
        assert again.objective == full.objective and again.stats["pivots"] == full.stats["pivots"]
        assert np.array_equal(again.flow, full.flow)


def test_progress_callback_cadence(gpu_engine_module):
    case = next(c for c in CASES if c["name"] == "perf_chain_seed24")
    problem = nfs.build_problem(case["nodes"], case["arcs"], True, 1e-6)
    seen = []
    res = nfs.solve_min_cost_flow(problem, nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True),
                                  progress_callback=seen.append, progress_interval=25)
    assert res.status == "optimal"
    assert [p.iteration for p in seen] == list(range(25, res.iterations + 1, 25))[: len(seen)]
    assert len(seen) == res.iterations // 25 or len(seen) == (res.iterations - 1) // 25
    assert all(p.phase in (1, 2) and p.elapsed_time >= 0 for p in seen)
    # on a chain nothing can flow before the whole path is basic, so early estimates are 0
    assert all(0.0 <= p.objective_estimate <= res.objective + 1e-6 for p in seen)


def test_iteration_limit_semantics(gpu_engine_module):
    # tests/unit/test_simplex.py:105-123: budget exhausted before feasibility -> iteration_limit, no flows
    p = nfs.build_problem([{"id": "s", "supply": 2.0}, {"id": "m", "supply": 0.0}, {"id": "t", "supply": -2.0}],
                          [{"tail": "s", "head": "m", "capacity": 2.5, "cost": 1.5},
                           {"tail": "m", "head": "t", "capacity": 2.5, "cost": 1.5}], True, 1e-6)
    r = nfs.solve_min_cost_flow(p, max_iterations=1)
    assert r.status == "iteration_limit" and r.flows == {}
    full = nfs.solve_min_cost_flow(p)
    assert full.status == "optimal" and full.objective == pytest.approx(6.0)
    # budget == exact pivot count still reports optimal (simplex.py:1678-1699 re-prices at the limit)
    again = nfs.solve_min_cost_flow(p, max_iterations=full.iterations)
    assert again.status == "optimal"


def test_empty_and_degenerate_inputs(gpu_engine_module):
    e = gpu_engine_module
    z32, z64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
    with e.McfEngine(2, z32, z32, z64, z64, [0, 0]) as eng:        # no arcs, nothing to ship
        eng.solve()
        assert eng.result().status == "optimal" and eng.price_once(0) is None
    with e.McfEngine(2, z32, z32, z64, z64, [3, -3]) as eng:       # no arcs, something to ship
        eng.solve()
        assert eng.result().status == "infeasible"
    with e.McfEngine(2, [0], [1], [5], [0], [0, 0]) as eng:        # zero-capacity arc
        eng.solve()
        assert eng.result().objective == 0
    with e.McfEngine(2, [0, 0], [1, 1], [5, 2], [3, 3], [4, -4]) as eng:   # parallel arcs
        eng.solve()
        r = eng.result()
        assert r.objective == 2 * 3 + 5 * 1 and r.flow.tolist() == [1, 3]
    with pytest.raises(e.EngineError):
        e.McfEngine(2, [0], [0], [1], [1], [0, 0])                # self loop
    with pytest.raises(e.EngineError):
        e.McfEngine(2, [0], [1], [1], [1], [1, 0])                # unbalanced
    with pytest.raises(e.EngineError):
        e.McfEngine(2, [0], [1], [2 ** 40], [1], [0, 0])          # cost beyond int32


# ------------------------------------------------------------------ BASELINE.json sizes: certificates
@pytest.mark.parametrize("name,rule", [("netgen_8_14a", 0), ("gridgen_8_14a", 1), ("goto_8_16a", 0)])
def test_baseline_sizes_certified_optimal(gpu_engine_module, name, rule):
    inst = generators.named_instance(name)
    res, tree = _solve(gpu_engine_module, inst, rule)
    assert res.status == "optimal" and res.stats["artificial_flow"] == 0
    check_optimality(inst, res.flow, res.potential)               # optimal for THIS instance, oracle-free
    assert res.objective == int(np.dot(res.flow, inst.cost))
    fix = _baseline_objectives().get(name)                         # ... and the pinned value (goto_8_16a: certified on the GPU by two
    if fix:                                                        # rules and recomputed by the CPU emulation of the integer algorithm)
        assert inst.sha256() == fix["sha256"] and res.objective == fix["objective"]
    n = inst.n                                                     # vectorised tree invariants
    order, pos, size, parent = tree["order"], tree["pos"], tree["size"], tree["parent"]
    assert np.array_equal(np.sort(order), np.arange(n + 1)) and np.array_equal(order[pos], np.arange(n + 1))
    v = np.arange(n)
    assert (pos[parent[v]] < pos[v]).all() and (pos[v] + size[v] <= pos[parent[v]] + size[parent[v]]).all()
    assert np.array_equal(np.bincount(parent[v], weights=size[v], minlength=n + 1).astype(np.int64) + 1, size)
    if name == "netgen_8_14a":                                    # the other rule must land on the same optimum
        pass
    if name == "netgen_8_14a":
        other, _ = _solve(gpu_engine_module, inst, 1)
        assert other.objective == res.objective


def test_million_node_sweep_and_partial_solve(gpu_engine_module):
    """Config 5 shape (1M nodes / 16M arcs): the full Dantzig sweep agrees with numpy on the
    start basis, and after 300 pivots flow conservation and the tree invariants still hold."""
    inst = generators.named_instance("netgen_1m_16m")
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0) as eng:
        t = eng.tree()
        viol = -(inst.cost + t["pi"][inst.tail] - t["pi"][inst.head])       # every arc starts at its lower bound
        got = eng.price_once(0)
        assert got[0] == int(np.argmax(viol)) and got[2] == int(viol.max()) and got[1] == 1
        eng.solve(max_pivots=300)
        r = eng.result()
        assert r.stats["pivots"] == 300
        bal = inst.supply.astype(np.int64).copy()
        np.subtract.at(bal, inst.tail, r.flow)
        np.add.at(bal, inst.head, r.flow)
        t = eng.tree()
        art = np.zeros(inst.n, np.int64)                                     # what the artificial arcs still carry
        assert (r.flow >= 0).all() and (r.flow <= inst.cap).all()
        assert np.abs(bal).sum() == 2 * r.stats["artificial_flow"] or np.abs(bal).sum() <= 2 * r.stats["artificial_flow"]
        order, pos = t["order"], t["pos"]
        assert np.array_equal(order[pos], np.arange(inst.n + 1))
        basic = t["state"] == 0
        rc = inst.cost + t["pi"][inst.tail] - t["pi"][inst.head]
        assert (rc[basic] == 0).all()                                        # tree arcs keep rc == 0


# ------------------------------------------------------------------ DIMACS file -> native reader -> engine
@pytest.mark.parametrize("strategy", ["dantzig", "devex", "adaptive"])
def test_dimacs_file_to_flat_problem_to_solve(gpu_engine_module, tmp_path, strategy):
    """write DIMACS -> parse_dimacs_file(native=True) (mcf_dimacs_scan / mcf_dimacs_load, no Python object per arc)
    -> solve_min_cost_flow on the SoAProblem -> the reference's golden status / objective / flows: its three .min
    fixtures, the netgen_8_08a stand-in, and a variant with lower bounds (shifted natively, simplex.py:413-428)."""
    opts = nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True, auto_scale=False)
    for case in CASES:
        if "dimacs_text" not in case:
            continue
        f = tmp_path / (case["name"] + ".min")
        f.write_text(case["dimacs_text"])
        prob = nfs.parse_dimacs_file(f, native=True)
        assert isinstance(prob, nfs.SoAProblem)
        res = nfs.solve_min_cost_flow(prob, opts)
        exp = next(iter(case["expected"].values()))
        assert res.status == exp["status"] == "optimal" and res.objective == exp["objective"]
        ref = oracle.solve_dicts(case["nodes"], case["arcs"], case["directed"], case["tolerance"], "dantzig")
        if ref.min_nonbasic_abs_rc > 1e-6:        # unique optimum (tiny_transportation has two flows of cost 111)
            assert res.flows == {(t, h): fl for t, h, fl in exp["flows"]}
        else:
            bal = {str(nd["id"]): float(nd.get("supply", 0.0)) for nd in case["nodes"]}
            for (t, h), fl in res.flows.items():
                bal[t] -= fl
                bal[h] += fl
            assert all(abs(v) <= 1e-9 for v in bal.values())
        assert isinstance(res.flows.array, np.ndarray) and len(res.duals) == prob.n   # flat views stay available
    entry, inst = load_synthetic()[3]                                # netgen_8_08a(synthetic)
    f = tmp_path / "netgen_8_08a.min"
    generators.write_dimacs(inst, f)
    prob = nfs.parse_dimacs_file(f, native=True)
    res = nfs.solve_min_cost_flow(prob, opts)
    exp = next(iter(entry["expected"].values()))
    assert res.status == "optimal" and res.objective == exp["objective"]
    assert np.array_equal(np.asarray(res.flows.array), np.asarray(res.flows.array, dtype=np.int64))
    rc = check_optimality(inst, res.flows.array, res.duals.array.astype(np.int64))
    if optimum_is_unique(inst, res.flows.array, res.basis.in_tree.astype(bool), rc):
        assert {(int(t) - 1, int(h) - 1): v for (t, h), v in res.flows.items()} == golden_flows(exp)
    # warm start from the flat basis: no pivots left to make
    again = nfs.solve_min_cost_flow(prob, opts, warm_start_basis=res.basis)
    assert again.objective == res.objective and again.iterations <= 2
    # lower bounds: the same instance with lower = 1 on every third capacitated arc of width >= 2 has the optimum of the
    # object-model path (which applies the reference's shift in flatten_problem)
    lower = np.where((np.arange(inst.m) % 3 == 0) & (inst.cap >= 2), 1, 0).astype(np.int64)
    low = nfs.SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, lower=lower)
    a = nfs.solve_min_cost_flow(low, opts)
    b = nfs.solve_min_cost_flow(low.to_network_problem(), opts)
    assert a.status == b.status and a.objective == b.objective
    if a.status == "optimal":
        assert (a.flows.array >= lower).all()


# ------------------------------------------------------------------ BASELINE.json sizes: solved to optimality
def _baseline_objectives():
    import json
    from conftest import GOLDEN
    return json.loads((GOLDEN / "baseline_objectives.json").read_text())


@pytest.mark.parametrize("name", ["netgen_8_14a", "gridgen_8_14a"])
def test_baseline_14a_objectives_equal_the_oracle(gpu_engine_module, name):
    """gridgen_8_14a / netgen_8_14a: every rule lands on the objective the C restatement of the reference
    computes (tests/golden/baseline_objectives.json, made by tests/golden/make_baseline_objectives.py in the
    build container: ~30 s of oracle time each, too long for the GPU-box test run).  The reference itself cannot
    run these sizes (dense (n-1)^2 basis), so this is pinned by the oracle, which in turn is pinned by the goldens."""
    fix = _baseline_objectives()[name]
    inst = generators.named_instance(name)
    assert inst.sha256() == fix["sha256"]
    pivots = {}
    for rule in RULES:
        res, _ = _solve(gpu_engine_module, inst, rule)
        assert res.status == "optimal" and res.stats["artificial_flow"] == 0
        assert res.objective == fix["objective"], (name, rule)
        check_optimality(inst, res.flow, res.potential)
        pivots[rule] = res.stats["pivots"]
    assert pivots[1] <= 1.25 * max(pivots[0], pivots[2])          # Devex is no longer the inefficient rule


def test_million_node_instance_solved_to_certified_optimality(gpu_engine_module, capsys):
    """configs[4]'s shape (1 M nodes / 16 M arcs), solved to the end: optimality certificate (conservation, bounds,
    complementary slackness -- needs no oracle), no artificial flow, objective == sum(flow * cost) recomputed on the
    host and == the pinned value (tests/golden/baseline_objectives.json).  Two routes to the same optimum: the raw
    engine with the candidate-list rule, and the public API on the flat SoAProblem with default options (adaptive ->
    candidate list), warm-started from the first run's basis so that it only has to CONFIRM optimality (a second cold
    solve would double a multi-minute test).  Progress lines keep the GPU box's silence watchdog quiet."""
    import time

    inst = generators.named_instance("netgen_1m_16m")
    fix = _baseline_objectives().get("netgen_1m_16m")
    t0 = time.time()
    last = [t0]

    def progress(pivots, cap, elapsed):
        if time.time() - last[0] > 25:
            last[0] = time.time()
            with capsys.disabled():
                print(f"\n  [netgen_1m_16m] {pivots} pivots, {time.time() - t0:.0f} s", flush=True)
        return False

    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2) as eng:
        eng.solve(max_pivots=60_000_000, progress=progress, progress_interval=250_000)
        res = eng.result()
    assert res.status == "optimal", (res.status, res.stats["pivots"])
    assert res.stats["artificial_flow"] == 0
    check_optimality(inst, res.flow, res.potential)
    assert res.objective == int(np.dot(res.flow.astype(object), inst.cost.astype(object)))
    with capsys.disabled():
        print(f"\n  [netgen_1m_16m] optimal: {res.stats['pivots']} pivots, {time.time() - t0:.0f} s, objective {res.objective}", flush=True)
    if fix:
        assert inst.sha256() == fix["sha256"] and res.objective == fix["objective"]
    # the public API on the flat problem, default options, warm start: the certified basis stays optimal
    from network_flow_solver_amd.data import ArrayBasis

    prob = nfs.SoAProblem(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply)
    at_upper = ~res.in_tree & (inst.cap > 0) & (res.flow == inst.cap)
    api = nfs.solve_min_cost_flow(prob, warm_start_basis=ArrayBasis(inst.tail, inst.head, res.in_tree, at_upper, res.flow))
    assert api.status == "optimal" and api.objective == float(res.objective)
    # A Basis names REAL arcs only (as the reference's does: artificial arcs never leave the solver, simplex.py:1744-1765), so
    # the node each component of the basis hung on is not handed over.  Round 2 hung every component on its lowest node (like
    # simplex.py:826-873): every degenerate basic arc on the path between that node and the old one then points the wrong way
    # for strong feasibility, the repair in mcf_apply_basis replaced each by an artificial arc, and one degenerate pivot each
    # won them back -- the 132 pivots measured then (30 on netgen_8_14a; profiles/r03_warm_start_pivots.log).  [r3]
    # mcf_apply_basis picks the hanging node with the fewest wrong-way arcs (zero for a basis of this engine): with one
    # component (k == 1, the usual case) the certified optimum is confirmed without a single pivot.
    k = int(inst.n - int(res.in_tree.sum()))
    with capsys.disabled():
        print(f"\n  [netgen_1m_16m] warm start: {api.iterations} pivots for {k} forest components", flush=True)
    # (k > 1: the components' potentials may shift against each other -- 42 pivots for k = 3 on gridgen_8_14a, same log)
    assert api.iterations == 0 if k == 1 else api.iterations <= 64 * k, (api.iterations, k)
    assert np.array_equal(api.flows.array, res.flow)


def test_batched_small_instances_equal_one_by_one(gpu_engine_module):
    """mcf_solve_batch: independent small instances, one persistent LDS-resident workgroup each in ONE launch -- every
    instance ends exactly where its own mcf_solve ends (pivots, flows, potentials, tree), rules mixed, budgets and
    resumes included; handles that are not on the LDS path are refused."""
    e = gpu_engine_module
    insts, rules = [], []
    for k in range(40):
        n = (40, 96, 160, 256)[k % 4]
        insts.append(generators.netgen_style(n, n * (4, 8)[k % 2], seed=100 + k) if k % 5 else generators.gridgen_style(8 + k % 7, 9, seed=k))
        rules.append(k % 3)
    single = []
    for inst, rule in zip(insts, rules):
        single.append(_solve(e, inst, rule))
    engines = [e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule) for inst, rule in zip(insts, rules)]
    try:
        assert all(eng.stats()["pricing_mode"] == 2 for eng in engines)
        ms = e.solve_batch(engines, max_pivots=17)                   # a budget first ...
        assert ms > 0 and all(eng.stats()["pivots"] == min(17, s[0].stats["pivots"]) for eng, s in zip(engines, single))
        e.solve_batch(engines[:7], max_pivots=[1, 2, 3, 4, 5, 6, 7])     # ... per-handle budgets on a part of the batch ...
        e.solve_batch(engines)                                       # ... then to the end
        for eng, (res0, tree0), inst in zip(engines, single, insts):
            res, tree = eng.result(), eng.tree()
            assert res.status == res0.status == "optimal" and res.objective == res0.objective
            assert res.stats["pivots"] == res0.stats["pivots"] and res.stats["degenerate"] == res0.stats["degenerate"]
            assert np.array_equal(res.flow, res0.flow) and np.array_equal(res.potential, res0.potential)
            assert np.array_equal(tree["order"], tree0["order"]) and np.array_equal(tree["parent"], tree0["parent"])
            check_optimality(inst, res.flow, res.potential)
        e.solve_batch(engines)                                       # solved handles: a no-op
        assert engines[0].result().stats["pivots"] == single[0][0].stats["pivots"]
        big = generators.named_instance("netgen_8_12a")
        with e.McfEngine(big.n, big.tail, big.head, big.cost, big.cap, big.supply, rule=0) as other:
            with pytest.raises(e.EngineError) as err:
                e.solve_batch([engines[0], other])
            assert err.value.code == -6
    finally:
        for eng in engines:
            eng.close()


def test_solve_many_equals_solving_one_by_one(gpu_engine_module):
    """solve_many: the reference's small fixtures (optimal, infeasible, unbounded, alternative optima, every structured
    class) in one batched launch -- each result is what solve_min_cost_flow returns for that problem."""
    problems = [nfs.build_problem(c["nodes"], c["arcs"], c["directed"], c["tolerance"]) for c in CASES]
    batch = nfs.solve_many(problems, nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True), return_exceptions=True)
    assert len(batch) == len(CASES)
    n_exc = 0
    for case, problem, got in zip(CASES, problems, batch):
        try:
            one = nfs.solve_min_cost_flow(problem, nfs.SolverOptions(pricing_strategy="dantzig", explicit_pricing_strategy=True))
        except nfs.NetworkSolverError as exc:
            assert type(got) is type(exc) and str(got) == str(exc), case["name"]
            n_exc += 1
            continue
        assert (got.status, got.iterations, got.objective) == (one.status, one.iterations, one.objective), case["name"]
        assert dict(got.flows) == dict(one.flows) and dict(got.duals) == dict(one.duals), case["name"]
        exp = case["expected"]["dantzig"]
        assert got.status == exp["status"] and got.objective == pytest.approx(exp["objective"], abs=1e-9)
    assert n_exc >= 1
    with pytest.raises(nfs.UnboundedProblemError):
        nfs.solve_many(problems)


@pytest.mark.parametrize("width", ["512", "1024"])
def test_batched_persistent_loops_equal_one_by_one(gpu_engine_module, monkeypatch, width):
    """mcf_solve_batch over persistent-loop handles (state in global memory, one workgroup per instance -- of 1 024 threads,
    or of 512 so that two instances share a CU: the launch picks by count and size, the test forces each), mixed with LDS-loop
    handles in the same call: every instance ends exactly where its own solve ends (candidate-list handles sweep for themselves inside the loop);
    graph-path handles are refused."""
    e = gpu_engine_module
    insts = [generators.netgen_style((300, 700, 1500, 3000)[k % 4], (300, 700, 1500, 3000)[k % 4] * 8, seed=7 + k) for k in range(12)]
    insts += [generators.netgen_style(128, 1024, seed=50 + k) for k in range(4)]
    rules = [k % 3 for k in range(len(insts))]
    single = [_solve(e, inst, rule) for inst, rule in zip(insts, rules)]
    monkeypatch.setenv("MCF_BATCH_THREADS", width)
    engines = [e.McfEngine(i.n, i.tail, i.head, i.cost, i.cap, i.supply, rule=r, mid_loop=1) for i, r in zip(insts, rules)]
    try:
        assert sorted({eng.stats()["pricing_mode"] for eng in engines}) == [2, 3]
        e.solve_batch(engines, max_pivots=123)
        assert all(eng.stats()["pivots"] == min(123, s[0].stats["pivots"]) for eng, s in zip(engines, single))
        e.solve_batch(engines)
        for eng, (res0, tree0), inst in zip(engines, single, insts):
            res, tree = eng.result(), eng.tree()
            assert res.status == res0.status == "optimal" and res.objective == res0.objective
            assert res.stats["pivots"] == res0.stats["pivots"] and np.array_equal(res.flow, res0.flow)
            assert np.array_equal(res.potential, res0.potential) and np.array_equal(tree["order"], tree0["order"])
            rc, resident = eng.reduced_costs()
            if resident:
                assert np.array_equal(rc, inst.cost + tree["pi"][inst.tail] - tree["pi"][inst.head])
        big = insts[3]   # 3 000 nodes on the kernel-per-phase graph: not one persistent workgroup
        with e.McfEngine(big.n, big.tail, big.head, big.cost, big.cap, big.supply, rule=0, mid_loop=-1) as grapher:
            with pytest.raises(e.EngineError) as err:
                e.solve_batch([engines[0], grapher])
            assert err.value.code == -6
    finally:
        for eng in engines:
            eng.close()


@pytest.mark.parametrize("strategy", ["devex", "dantzig", "candidate_list"])
def test_solve_many_batches_mid_size_problems_too(gpu_engine_module, strategy):
    """solve_many over flat problems of 300 ... 3 000 nodes: Dantzig / Devex problems run as one persistent workgroup each
    in the batched launch (a candidate-list loop sweeps for itself); every result equals the problem's own solve."""
    insts = [generators.netgen_style(n, 8 * n, seed=11 + k) for k, n in enumerate((300, 700, 1500, 3000, 200, 900))]
    problems = [nfs.SoAProblem(i.n, i.tail, i.head, i.cost, i.cap, i.supply) for i in insts]
    opts = nfs.SolverOptions(pricing_strategy=strategy, explicit_pricing_strategy=True)
    many = nfs.solve_many(problems, opts)
    for problem, got, inst in zip(problems, many, insts):
        one = nfs.solve_min_cost_flow(problem, opts)
        assert (got.status, got.iterations, got.objective) == (one.status, one.iterations, one.objective) and got.status == "optimal"
        assert np.array_equal(got.flows.array, one.flows.array)
        ref = oracle.solve_soa(inst, "dantzig", reference_order=False)
        assert got.objective == ref["objective"]


def test_adapter_solves_a_benchmark_group_at_once(gpu_engine_module):
    """Mi355xAdapter.solve_many: one SolverResult per problem, equal to what the per-problem ``solve`` reports."""
    from network_flow_solver_amd.adapter import Mi355xAdapter

    problems = [nfs.build_problem(c["nodes"], c["arcs"], c["directed"], c["tolerance"]) for c in CASES[:16]]
    group = Mi355xAdapter.solve_many(problems)
    assert len(group) == 16
    for problem, got in zip(problems, group):
        one = Mi355xAdapter.solve(problem)
        assert (got.status, got.objective, got.iterations) == (one.status, one.objective, one.iterations)
        assert got.solver_name == "network_solver_mi355x" and got.solve_time_ms >= 0


# ------------------------------------------------------------------ blocked preorder list, candidate cache, resident-rc drop
@pytest.mark.parametrize("rule", RULES, ids=RULE_IDS)
def test_blocked_preorder_list_equals_dense_array_on_gpu(gpu_engine_module, rule):
    """mcf_options.tree_blocks: the tree's preorder in physical blocks with a logical base each (k_update_bpl: O(subtree +
    block) element moves per basis swap; replaces the per-pivot rebuild basis.py:82-125 / simplex.py:1103-1107).  Same logical
    preorder as the dense array: pivots, flows, potentials, order, positions, sizes, depths equal the CPU emulation of the
    DENSE array for every block size, with a generous pool, a small one and none (a dense rewrite into the other arena on
    every pivot), resident reduced costs or gathers, graph or eager, scan or climb."""
    e = gpu_engine_module
    cases = [load_synthetic()[0][1], load_synthetic()[4][1], generators.goto_style(12, 12, seed=4), generators.netgen_style(1024, 8192, seed=5)]
    for inst in cases:
        em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)
        for shift, pool in ((2, 0), (2, -1), (3, 5), (6, 0), (6, -1), (8, 3)):
            for opts in ({}, {"cycle_scan": -1}, {"resident_rc": False}, {"use_graph": False, "climb_depth": -1}, {"full_sweeps": -1}):
                with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, tree_blocks=shift, tree_pool=pool, **opts) as eng:
                    eng.solve()
                    res, tree = eng.result(), eng.tree()
                assert res.stats["tree_blocks"] == shift and res.stats["pricing_mode"] in (0, 1)
                assert res.status == em["status"] == "optimal" and res.objective == em["objective"] and res.stats["pivots"] == em["pivots"]
                assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"])
                for key in ("order", "pos", "psize", "parent", "depth", "size"):
                    assert np.array_equal(tree[key], em[key]), key
                if pool < 0:
                    assert res.stats["tree_rebuilds"] > 0.5 * res.stats["pivots"]
                else:
                    assert res.stats["nodes_moved"] <= res.stats["subtree_nodes"] + 2 * (1 << shift) * res.stats["pivots"] + (inst.n + 1) * res.stats["tree_rebuilds"]
        check_tree_invariants(inst.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])


def test_candidate_cache_and_reduced_cost_drop(gpu_engine_module):
    """Candidate-list rule on the grid path: the records of the live list (end points, state, exact reduced cost) are written by
    the sweep and kept current by every pivot's update pass, so a minor iteration (simplex_pricing.py:419-456) is one read of
    the list; and a handle may give up its resident reduced costs in mid-solve (mcf_options.rc_drop).  Neither changes a pivot:
    budgets and resumes, incremental sweeps, gathers, both tree layouts -- always the CPU emulation's pivots, flows, tree."""
    e = gpu_engine_module
    for inst in (generators.netgen_style(3000, 24000, seed=11), generators.goto_style(40, 40, seed=12)):
        em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2)
        emf = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2 | 0x100)
        for layout in (-1, 6):
            for opts in ({}, {"resident_rc": False}, {"full_sweeps": -1}, {"rc_drop": 1}, {"rc_drop": 1, "full_sweeps": -1}, {"use_graph": False, "rc_drop": 2},
                         {"forward_first": True}, {"batch_pivots": 7, "rc_drop": 1}, {"pivot_run": 4}, {"pivot_run": 2, "rc_drop": 1}):
                # (pivot_run: the opt-in run shape -- minor pivots back to back in one workgroup with their updates in place;
                #  it needs the blocked list and is ignored on the dense layout)
                ref = emf if opts.get("forward_first") else em
                with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2, tree_blocks=layout, fused=False, mid_loop=-1, **opts) as eng:
                    for budget in (1, 50, 4999):
                        eng.solve(max_pivots=budget)
                    eng.solve()
                    res, tree = eng.result(), eng.tree()
                    rc, resident = eng.reduced_costs()
                assert res.status == "optimal" and res.objective == ref["objective"] and res.stats["pivots"] == ref["pivots"], (inst.name, layout, opts)
                assert np.array_equal(res.flow, ref["flow"]) and np.array_equal(res.potential, ref["potential"]) and np.array_equal(tree["order"], ref["order"])
                assert np.array_equal(rc, inst.cost + tree["pi"][inst.tail] - tree["pi"][inst.head])
                if "pivot_run" in opts and layout > 0 and "rc_drop" not in opts:
                    assert res.stats["run_pairs"] > 0 or res.stats["run_left_at"] > 0, (inst.name, opts, res.stats)
                if "rc_drop" in opts:   # the switch happened (after the first batches) and the handle says so
                    assert 0 < res.stats["rc_dropped_at"] < res.stats["pivots"] and res.stats["pricing_mode"] == 0 and not resident
                else:
                    assert res.stats["rc_dropped_at"] == 0
        # Devex gives its reduced costs up too when asked to; a two-stream graph (pricing beside the permutation) is only valid
        # from resident values and ends with them (found by scripts/fuzz_gpu.py: 3 of 130 runs diverged before that was enforced)
        emd = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=1)
        for opts in ({"rc_drop": 1}, {"rc_drop": 1, "overlap_update": 1}, {"rc_drop": 3, "overlap_update": 1, "batch_pivots": 32}):
            with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=1, fused=False, mid_loop=-1, **opts) as eng:
                eng.solve()
                res, tree = eng.result(), eng.tree()
            assert res.status == "optimal" and res.stats["pivots"] == emd["pivots"] and res.stats["rc_dropped_at"] > 0, (inst.name, opts, res.stats["pivots"], emd["pivots"])
            assert np.array_equal(res.flow, emd["flow"]) and np.array_equal(res.potential, emd["potential"]) and np.array_equal(tree["order"], emd["order"])
        # a reset brings the resident reduced costs back
        with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2, rc_drop=1, fused=False, mid_loop=-1) as eng:
            eng.solve()
            assert eng.stats()["rc_dropped_at"] > 0
            eng.reset()
            eng.solve(max_pivots=100)
            rc, resident = eng.reduced_costs()
            assert resident and eng.stats()["rc_dropped_at"] == 0
            eng.solve()
            assert eng.result().objective == em["objective"] and eng.stats()["pivots"] == em["pivots"]


def _drive_shards(e, inst, rule, G, budget, listing, **opts):
    """`G` sharded handles on this GPU driven like distributed.PivotLoop drives them over RCCL (the all-gather is a device
    copy here): per-pivot protocol (one 16-byte candidate per rank) or, `listing`, the candidate-list protocol (one list
    per rank per minor_cap + 1 pivots).  Stops at `budget` total pivots or at a final status.  Returns the engines (open)."""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    engs = [e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, shard=(r, G), device=0, **opts) for r in range(G)]
    K, minor_cap = engs[0].shard_info() if listing else (1, 0)
    buf = ctypes.c_void_p()
    nbytes = 16 * K * G
    assert hip.hipMalloc(ctypes.byref(buf), 2 * nbytes) == 0 and hip.hipMemset(buf, 0xff, 2 * nbytes) == 0
    local = [buf.value + 16 * K * r for r in range(G)]
    gathered = buf.value + nbytes
    try:
        for eng in engs:
            eng.set_max_pivots(budget)
        for _ in range(100000):
            for _ in range(8):
                for r, eng in enumerate(engs):
                    (eng.enqueue_price_list if listing else eng.enqueue_price)(0, local[r])
                assert hip.hipMemcpyAsync(gathered, buf.value, nbytes, 3, None) == 0
                for eng in engs:
                    if listing:
                        eng.enqueue_pivots(0, gathered, K * G, minor_cap + 1)
                    else:
                        eng.enqueue_pivot(0, gathered, G)
            assert hip.hipDeviceSynchronize() == 0
            polls = [eng.poll() for eng in engs]
            assert len(set(polls)) == 1
            if polls[0][0] is not None:
                break
    finally:
        hip.hipFree(buf)
    return engs


def _check_shard_state(e, inst, engs, keyed):
    """Replicas bit-identical; every arc's resident reduced cost exact on the rank that owns it (reduced_costs() merges the
    rank's own shard with values computed from the potentials); every arc's key code exact on at least its owner."""
    trees = [eng.tree() for eng in engs]
    res = [eng.result() for eng in engs]
    for r, t in zip(res[1:], trees[1:]):
        assert np.array_equal(r.flow, res[0].flow) and np.array_equal(r.potential, res[0].potential)
        assert np.array_equal(t["order"], trees[0]["order"]) and np.array_equal(t["parent"], trees[0]["parent"]) and np.array_equal(t["state"], trees[0]["state"])
    pi = trees[0]["pi"]
    truth = inst.cost + pi[inst.tail] - pi[inst.head]
    for eng in engs:
        rc, resident = eng.reduced_costs()
        assert resident and np.array_equal(rc, truth)
    if keyed:
        bigm = (int(np.abs(inst.cost).max()) + 1) * (inst.n + 2)
        want = _vkey_code(-(trees[0]["state"].astype(np.int64)) * truth, bigm, 1 << 28)
        exact_somewhere = np.zeros(inst.m, bool)
        for eng in engs:
            keys, present = eng.pricing_keys()
            assert present
            exact_somewhere |= keys == want
        assert exact_somewhere.all()
    return res[0], trees[0]


@pytest.mark.parametrize("protocol", ["per_pivot_dantzig", "candidate_lists"])
def test_sharded_handles_in_the_configuration_they_really_run_in(gpu_engine_module, protocol):
    """BASELINE.json configs[3] / configs[4] put sharded handles on arcs >= 4 M, where a Dantzig / candidate-list handle sweeps
    4-byte key codes, incrementally, and patches only its own shard's reduced costs (mcf_engine.hip: rc_partial, vkey, dirty).
    That combination with shard_count > 1: three handles on this GPU, key codes + incremental sweeps forced on, (a) netgen_8_14a
    to optimality and (b) 1 M nodes / 16 M arcs for a budget of 5 000 pivots, on the blocked tree layout.  Replicas bit-identical;
    reduced costs and key codes exact on every rank's shard; the per-pivot Dantzig protocol pivots exactly like the unsharded
    engine; the result of (a) is the certified optimum."""
    e = gpu_engine_module
    listing = protocol == "candidate_lists"
    rule = 2 if listing else 0
    opts = dict(compressed_keys=1, full_sweeps=-1)
    # (a) to optimality
    inst = generators.named_instance("netgen_8_14a")
    engs = _drive_shards(e, inst, rule, 3, 10 ** 9, listing, tree_blocks=6, **opts)
    try:
        assert all(eng.stats()["sweep_variant"] & 5 == 5 for eng in engs)      # key codes + incremental really on
        r0, t0 = _check_shard_state(e, inst, engs, keyed=True)
    finally:
        for eng in engs:
            eng.close()
    assert r0.status == "optimal"
    check_optimality(inst, r0.flow, r0.potential)
    single, ts = _solve(e, inst, rule, fused=False, mid_loop=-1)
    assert single.objective == r0.objective
    if not listing:
        assert single.stats["pivots"] == r0.stats["pivots"] and np.array_equal(single.flow, r0.flow) and np.array_equal(ts["order"], t0["order"])
    # (b) the million-node shape, a budget of pivots: key codes and incremental sweeps together again, the blocked list by default
    big = generators.named_instance("netgen_1m_16m")
    budget = 5000
    engs = _drive_shards(e, big, rule, 3, budget, listing, **opts)
    try:
        st = engs[0].stats()
        assert st["tree_blocks"] > 0 and st["sweep_variant"] & 5 == 5
        rb, tb = _check_shard_state(e, big, engs, keyed=True)
    finally:
        for eng in engs:
            eng.close()
    assert rb.stats["pivots"] >= budget
    if not listing:   # the unsharded engine, same budget: the same pivots
        with e.McfEngine(big.n, big.tail, big.head, big.cost, big.cap, big.supply, rule=0) as eng:
            eng.solve(max_pivots=int(rb.stats["pivots"]))
            rs, tsb = eng.result(), eng.tree()
        assert rs.stats["pivots"] == rb.stats["pivots"] and np.array_equal(rs.flow, rb.flow) and np.array_equal(tsb["order"], tb["order"])
