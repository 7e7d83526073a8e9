"""The post-solve device passes on PLANTED trees, across the caps of their launch geometry.

Every case is ``McfEngine(...)``, ``set_basis(in_tree, at_upper)`` -- which has to return ``True`` and to arrive at exactly the
planted parents, states and flows -- and then the passes; no case calls ``solve()``.  ``planted_trees`` chooses shape, size
and depth of the tree and knows every answer from the construction (``test_planted_trees_cpu.py`` tests that yardstick, and
shows that the host code keeps every basis used here whole).  Nothing has a tolerance: all of it is integer arithmetic.

  a. boundary sweep: n_nodes on both sides of a wave, a workgroup, a scan chunk; m on both sides of a bottleneck chunk; dense and
     blocked preorder; path / star / random / forest;
  b. depth: greatest depths 1, 2^k, 2^k +- 1 for the pointer-jumping rounds and the ray's placement by depth differences,
     residual chains on both sides of a batch of 32 search rounds;
  c. past the lane cap of the node passes (2 048 workgroups x 256 lanes): a second grid-stride trip with a ragged tail;
  d. past 1 024 scan chunks (two chunks per scan thread, 128-bit prefixes beyond 2^64) and past 2^22 arcs (non-temporal loads).
"""

from __future__ import annotations

import numpy as np
import pytest

import farkas_yardsticks as fy
import planted_trees as pt
from conftest import check_tree_invariants

pytestmark = pytest.mark.gpu

MCF_INF = 1 << 60
CERT_DROP = ("arc_pass_ms", "node_pass_ms", "status", "proves_status", "rc_compared", "key_compared")


def _engine(e, pl, **kw):
    i = pl.inst
    return e.McfEngine(i.n, i.tail, i.head, i.cost, i.cap, i.supply, **kw)


def _check_tree(pl, tree, large):
    if large:
        pt.check_tree_arrays(pl.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])
    else:
        check_tree_invariants(pl.n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"], tree["psize"])


def _install(e, pl, kw, tree_blocks=None, large=False):
    """A handle holding the planted basis: no arc dropped, the planted parents, states and flows."""
    eng = _engine(e, pl, **kw)
    if pl.in_tree.any():
        assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
    else:                                              # nothing basic to name: the cold start IS the planted forest
        assert not pl.at_upper.any() and not pl.flow.any()
    tree = eng.tree()
    _check_tree(pl, tree, large)
    assert np.array_equal(tree["parent"][: pl.n], pl.parent) and np.array_equal(tree["pred_arc"][: pl.n], pl.tree_arc)
    assert np.array_equal(tree["state"], pl.state)
    assert np.array_equal(eng.result().flow, pl.flow)
    if tree_blocks is not None:
        got = eng.stats()["tree_blocks"]
        assert got == max(tree_blocks, 0) if tree_blocks else got > 0
    return eng, tree


def _assert_cert(eng, pl, tree, cost, flow, art, bigm, supply=None):
    """certify(): every field; and the potentials of tree() are the recomputed ones."""
    pi = pt.potentials(pl, tree, cost, bigm, art)
    assert np.array_equal(tree["pi"], pi)
    cert = eng.certify()
    want = pt.certificate(pl, cost, flow, pi, art, bigm, supply)
    assert set(cert) - set(want) == set(CERT_DROP), set(cert) ^ set(want)
    assert {k: cert[k] for k in want} == want, {k: (cert[k], want[k]) for k in want if cert[k] != want[k]}
    assert cert["status"] == "running" and not cert["proves_status"] and cert["rc_compared"] in (0, pl.m)
    return pi


def _assert_rays(eng, pl, tree, cost, flow, pi, art, bigm, rng, count=32):
    nonbasic = np.flatnonzero(~pl.in_tree)
    if len(nonbasic) > count:
        pick = rng.choice(nonbasic, count, replace=False)
        if pl.at_upper.any() and not pl.at_upper[pick].any():
            pick[0] = np.flatnonzero(pl.at_upper)[0]
        nonbasic = pick
    walker = pt.RayWalker(pl, tree, cost, flow, pi, art, bigm)
    backward_seen = False
    for arc in nonbasic.tolist():
        got = eng.certify_ray(arc)
        want = walker.ray(arc, bool(pl.at_upper[arc]))
        assert got["arcs"].tolist() == want["arcs"], arc
        assert {k: got[k] for k in pt.RAY_FIELDS} == {k: want[k] for k in pt.RAY_FIELDS}, arc
        backward_seen |= got["entering_backward"]
    assert backward_seen == bool(pl.at_upper.any())


def _cut_sets(pl, rng):
    return (np.zeros(pl.n, bool), pt.subtree_set(pl, pl.n // 2), rng.random(pl.n) < 0.5)


def _assert_cut(got, want, S=None):
    assert {k: got[k] for k in want} == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    if S is not None:
        assert np.array_equal(got["S"], S)


def _assert_caller_cuts(eng, pl, rng, supply=None):
    for S in _cut_sets(pl, rng):
        _assert_cut(eng.certify_cut(in_S=S), pt.cut_answer(pl, S, supply), S)


def _assert_computed_cut(eng, pl, flow, art, supply=None):
    S, levels = pt.residual_levels(pl, flow, art)
    _assert_cut(eng.certify_cut(), pt.cut_answer(pl, S, supply, flow, art, levels), S)
    return levels


def _assert_bottlenecks(eng, pl, flow):
    for num, den in ((1, 1), (19, 20)):
        want = pt.bottleneck_list(pl, flow, num, den)
        for limit in (0, 10, pl.m):
            idx, count = eng.bottlenecks(num, den, limit=limit)
            assert count == len(want) and np.array_equal(idx, want[:limit]), (num, den, limit)


def _cost_changes(pl, rng, count=0):
    """(arcs, costs, the cost array afterwards): the tree arc nearest the root, a leaf's, a non-tree arc priced above the
    create-time maximum (big-M grows), an index named twice (the last entry wins), and `count` random ones besides."""
    top_children = np.flatnonzero((pl.parent < pl.n) & (np.append(pl.parent, pl.n)[np.minimum(pl.parent, pl.n)] == pl.n))
    leaves = np.setdiff1d(np.flatnonzero(pl.parent < pl.n), pl.parent)
    arcs, costs = [], []
    if len(top_children):
        near = int(pl.tree_arc[top_children[0]])
        arcs += [near, int(pl.tree_arc[leaves[-1]])]
        costs += [12345, int(pl.inst.cost[arcs[1]]) - 77]
    nontree = np.flatnonzero(~pl.in_tree)
    if len(nontree):
        arcs.append(int(nontree[0]))
        costs.append(int(np.abs(pl.inst.cost).max()) + 1000)
    if len(top_children):
        arcs.append(near)                                     # named twice: this one counts
        costs.append(int(pl.inst.cost[near]) + 31)
    if count:
        extra = rng.choice(pl.m, count, replace=False)
        arcs += extra.tolist()
        costs += rng.integers(-900, 900, count).tolist()
    cost = pl.inst.cost.copy()
    cost[np.array(arcs, np.int64)] = np.array(costs, np.int64)
    if len(top_children) and not count:
        assert cost[near] == pl.inst.cost[near] + 31
    return np.array(arcs, np.int64), np.array(costs, np.int64), cost


def _assert_update_costs(eng, pl, rng, art, flow, count=0, large=False, supply=None):
    arcs, costs, cost = _cost_changes(pl, rng, count)
    bigm = pt.big_m(pl, cost)
    assert bigm > pt.big_m(pl) or pl.m == pl.in_tree.sum()
    eng.update_costs(arcs, costs)
    tree = eng.tree()
    _check_tree(pl, tree, large)
    pi = _assert_cert(eng, pl, tree, cost, flow, art, bigm, supply)
    rc, _ = eng.reduced_costs()
    assert np.array_equal(rc, cost + pi[pl.inst.tail] - pi[pl.inst.head])
    assert np.array_equal(eng.result().flow, flow) and np.array_equal(tree["state"], pl.state)
    return cost, bigm, tree, pi


def _assert_update_rhs_clean(eng, pl, cost, bigm, large=False):
    """To the second planted vector: the basis stays, the flows are the planted ones, artificial arcs turn where planted."""
    rep = eng.update_rhs(nodes=np.arange(pl.n), supplies=pl.supply2)
    assert rep["path"] == 0 and rep["tree_violations"] == rep["wrong_way"] == rep["arcs_cut"] == rep["upper_moved"] == 0, rep
    tops = pl.parent == pl.n
    assert rep["art_flips"] == int(((pl.art >= 0) != (pl.art2 >= 0))[tops].sum())
    assert np.array_equal(eng.result().flow, pl.flow2)
    tree = eng.tree()
    _check_tree(pl, tree, large)
    assert np.array_equal(tree["parent"][: pl.n], pl.parent) and np.array_equal(tree["state"], pl.state)
    pi = _assert_cert(eng, pl, tree, cost, pl.flow2, pl.art2, bigm, pl.supply2)      # (conservation and bounds clean among all the rest)
    return tree, pi


def _assert_update_rhs_defects(eng, pl, tree, large=False):
    """To the second vector with defects: the census counts them, the basis is repaired and certifies clean."""
    rep = eng.update_rhs(nodes=np.arange(pl.n), supplies=pl.supply3)
    assert rep["tree_violations"] == len(pl.out_of_bounds) >= 1 and rep["wrong_way"] == pt.wrong_way(pl, tree, pl.on_bound, pl.flow3), rep
    assert rep["path"] == 1 and rep["arcs_cut"] >= 1, rep
    cert = eng.certify()
    assert cert["negative_flow_count"] == cert["over_capacity_count"] == cert["imbalance_count"] == 0, cert
    assert cert["tree_shape_count"] == cert["state_flow_count"] == cert["strong_count"] == cert["tree_rc_count"] == cert["basic_count_mismatch"] == 0, cert
    _check_tree(pl, eng.tree(), large)


def _all_passes(e, pl, kw, tree_blocks, seed, large=False, defects=None):
    rng = np.random.default_rng([77, seed])
    bigm = pt.big_m(pl)
    eng, tree = _install(e, pl, kw, tree_blocks, large)
    with eng:
        pi = _assert_cert(eng, pl, tree, pl.inst.cost, pl.flow, pl.art, bigm)
        _assert_rays(eng, pl, tree, pl.inst.cost, pl.flow, pi, pl.art, bigm, rng)
        _assert_caller_cuts(eng, pl, rng)
        if not large:
            _assert_computed_cut(eng, pl, pl.flow, pl.art)
        _assert_bottlenecks(eng, pl, pl.flow)
        cost, bigm2 = pl.inst.cost, bigm
        if pl.m:
            cost, bigm2, tree, pi = _assert_update_costs(eng, pl, rng, pl.art, pl.flow, large=large)
        tree, pi = _assert_update_rhs_clean(eng, pl, cost, bigm2, large)
        _assert_rays(eng, pl, tree, cost, pl.flow2, pi, pl.art2, bigm2, rng, count=4)
        _assert_caller_cuts(eng, pl, rng, pl.supply2)
        _assert_bottlenecks(eng, pl, pl.flow2)
    with _engine(e, pl, **kw) as fresh:                 # no basis: the artificial arcs carry the supplies
        _assert_computed_cut(fresh, pl, np.zeros(pl.m, np.int64), pl.inst.supply)
    for p, q in (pt.sweep_defects(pl) if defects is None else defects):
        bad = pt.plant_defects(pl, p, q)
        eng, tree = _install(e, bad, kw, tree_blocks, large)
        with eng:
            _assert_update_rhs_defects(eng, bad, tree, large)


# ------------------------------------------------------------------ a. boundary sweep
@pytest.mark.parametrize("n,shape,tree_blocks,m", [c[1:] for c in pt.sweep_cases()], ids=[c[0] for c in pt.sweep_cases()])
def test_boundary_sweep(gpu_engine_module, n, shape, tree_blocks, m):
    pl = pt.sweep_plant(n, shape, m)
    assert pl.n + 1 in (2, 3, 64, 65, 256, 257, 2048, 2049, 4097) and pl.m == m
    _all_passes(gpu_engine_module, pl, dict(tree_blocks=tree_blocks), tree_blocks, n)


def test_set_basis_refuses_a_flow_of_seventeen_times_the_capacity(gpu_engine_module):
    """The 64-bit edge of mcf_apply_basis (test_planted_trees_cpu.py): a surplus of 17 * (2^60 - 1) must not wrap into the bounds."""
    e = gpu_engine_module
    inst, in_tree, at_upper, _ = pt.int64_edge(17, shared_return=True)
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply) as eng:
        assert eng.set_basis(in_tree, at_upper) is False and "incompatible" in eng.last_error()
        assert not eng.result().flow.any() and (eng.tree()["state"] == 1).all()      # the cold start
    inst, in_tree, at_upper, flow = pt.int64_edge(16, shared_return=False)
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply) as eng:
        assert eng.set_basis(in_tree, at_upper) is True and np.array_equal(eng.result().flow, flow)
        cert = eng.certify()
        assert cert["imbalance_count"] == cert["negative_flow_count"] == cert["over_capacity_count"] == 0


# ------------------------------------------------------------------ b. depth
@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("d", pt.DEPTHS)
def test_depths_around_powers_of_two(gpu_engine_module, d, tree_blocks):
    e = gpu_engine_module
    kw = dict(tree_blocks=tree_blocks)
    pl = pt.cold_plant() if d == 1 else pt.depth_plant(d)
    bigm = pt.big_m(pl)
    eng, tree = _install(e, pl, kw, tree_blocks)
    with eng:
        assert int(tree["depth"].max()) == d
        pi0 = tree["pi"].copy()
        assert np.array_equal(pi0, pt.potentials(pl, tree, pl.inst.cost, bigm))
        if d == 1:
            # no real arc in the tree: a dearer non-tree arc grows big-M, and every potential moves by exactly the growth
            cost = pl.inst.cost.copy()
            cost[0] = int(np.abs(cost).max()) + 500
            eng.update_costs([0], [cost[0]])
            bigm2 = pt.big_m(pl, cost)
            pi1 = eng.tree()["pi"]
            assert bigm2 > bigm and np.array_equal(pi1 - pi0, np.append(np.where(pl.art >= 0, -1, 1) * (bigm2 - bigm), 0))
            arc = 0
            ray = eng.certify_ray(arc)
            want = pt.RayWalker(pl, tree, cost, pl.flow, pi1, pl.art, bigm2).ray(arc, False)
            assert ray["length"] == 3 == want["length"] and ray["arcs"].tolist() == want["arcs"] and ray["join"] == pl.n
            assert {k: ray[k] for k in pt.RAY_FIELDS} == {k: want[k] for k in pt.RAY_FIELDS}
            flip, other = 0, 1                          # supplies 5, -20, 7, 8 -> -5, -10, 7, 8: node 0's artificial arc turns round
            sup = pl.inst.supply.copy()
            sup[other] += 2 * sup[flip]
            sup[flip] = -sup[flip]
            assert sup[flip] < 0 < pl.inst.supply[flip] and sup[other] < 0 and sup.sum() == 0
            rep = eng.update_rhs(nodes=[flip, other], supplies=[sup[flip], sup[other]])
            assert rep["path"] == 0 and rep["art_flips"] == 1, rep
            moved = np.zeros(pl.n + 1, np.int64)
            moved[flip] = 2 * bigm2
            assert np.array_equal(eng.tree()["pi"] - pi1, moved)
            return
        # the arc at depth 1 joins node 0 (depth 1) and node 1: every potential below it moves by the change, nothing else does
        a = int(pl.tree_arc[1])
        cost = pl.inst.cost.copy()
        cost[a] += 37
        eng.update_costs([a], [cost[a]])
        assert pt.big_m(pl, cost) == bigm
        pi1 = eng.tree()["pi"]
        moved = np.zeros(pl.n + 1, np.int64)
        moved[1:d] = -37 if pl.inst.tail[a] == 1 else 37
        assert np.array_equal(pi1 - pi0, moved)
        assert np.array_equal(eng.reduced_costs()[0], cost + pi1[pl.inst.tail] - pi1[pl.inst.head])
        # the chords from the deepest node (depth d) to the node at depth 1: d arcs, in push order
        chords = np.flatnonzero(~pl.in_tree & (pl.inst.tail == d - 1) & (pl.inst.head == 0))
        assert len(chords) >= 2 and pl.at_upper[chords].any() and not pl.at_upper[chords].all()
        walker = pt.RayWalker(pl, tree, cost, pl.flow, pi1, pl.art, bigm)
        for arc in chords.tolist():
            ray = eng.certify_ray(arc)
            want = walker.ray(arc, bool(pl.at_upper[arc]))
            assert ray["length"] == d == want["length"] and ray["arcs"].tolist() == want["arcs"]
            assert {k: ray[k] for k in pt.RAY_FIELDS} == {k: want[k] for k in pt.RAY_FIELDS}
            tree_part = [int(pl.tree_arc[v]) for v in range(1, d)]
            # (entered backward, the push arrives at the deepest node and climbs; forward, it arrives at depth 1 and descends)
            assert want["arcs"][1:] == (tree_part[::-1] if pl.at_upper[arc] else tree_part)
        # the path's artificial arc turns round (supply sign change): every potential of the component moves by 2 big-M
        tree2, pi2 = _assert_update_rhs_clean(eng, pl, cost, bigm)
        moved = np.zeros(pl.n + 1, np.int64)
        moved[:d] = 2 * bigm
        assert pl.art[0] > 0 > pl.art2[0] and np.array_equal(pi2 - pi1, moved)
        _assert_computed_cut(eng, pl, pl.flow2, pl.art2, pl.supply2)


@pytest.mark.parametrize("tree_blocks", (-1, 3), ids=["dense", "blocked"])
@pytest.mark.parametrize("levels", pt.CUT_CHAINS)
def test_cut_search_stops_at_and_just_past_a_batch_of_rounds(gpu_engine_module, levels, tree_blocks):
    e = gpu_engine_module
    inst = fy.chain_cut_instance(length=levels, cut_at=levels // 2)       # (no flow yet: every arc of the chain has room)
    with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, tree_blocks=tree_blocks) as eng:
        got = eng.certify_cut()
    zero = np.zeros(inst.m, np.int64)
    art = fy.artificial_flows(inst, zero)
    S, lv = fy.residual_search(inst, zero, art)
    want = fy.cut_sums(inst, S, zero, art)
    want["rounds"] = lv
    assert lv == levels == got["rounds"] and np.array_equal(got["S"], S) and S.all() and inst.n == levels
    assert {k: got[k] for k in want} == want and got["seeds"] == 1 and got["deficit_in_S"] == 1


# ------------------------------------------------------------------ c. past the lane cap of the node passes
@pytest.mark.parametrize("tree_blocks", (-1, 0), ids=["dense", "auto"])
@pytest.mark.parametrize("shape", ("random", "caterpillar"))
def test_past_the_lane_cap(gpu_engine_module, shape, tree_blocks):
    pl = pt.large_plant(shape)
    assert pl.n + 1 > pt.LANE_CAP and (pl.n + 1) % 256 != 0 and pl.n >= 200000
    _all_passes(gpu_engine_module, pl, dict(tree_blocks=tree_blocks), tree_blocks, 5, large=True, defects=[(3, 2)])


# ------------------------------------------------------------------ d. past the scan's 1 024 chunks and the non-temporal threshold
def test_past_the_scan_chunks_and_the_non_temporal_threshold(gpu_engine_module):
    e = gpu_engine_module
    pl = pt.scan_plant()
    chunks = -(-(pl.n + 1) // 2048)
    # (1 026 chunks of 2 048 positions: two per scan thread, and the last one holds the two positions past 1 025 whole chunks)
    assert pl.n == 2097152 + 2049 and chunks == 1026 and (pl.n + 1) - 1025 * 2048 == 2 and pl.m == (1 << 22) + 5
    assert pt.max_prefix(pl, pl.art) > 1 << 64 and pt.max_prefix(pl, pl.art2) > 1 << 64
    rng = np.random.default_rng(4)
    bigm = pt.big_m(pl)
    eng, tree = _install(e, pl, dict(), 0, large=True)
    with eng:
        tree, pi = _assert_update_rhs_clean(eng, pl, pl.inst.cost, bigm, large=True)      # the 128-bit scan; certify(): k_cert_arcs<true>
        S = rng.random(pl.n) < 0.5
        _assert_cut(eng.certify_cut(in_S=S), pt.cut_answer(pl, S, pl.supply2), S)          # k_cut_arcs<true>
        cost, bigm2, tree, pi = _assert_update_costs(eng, pl, rng, pl.art2, pl.flow2, count=1000, large=True, supply=pl.supply2)
        _assert_rays(eng, pl, tree, cost, pl.flow2, pi, pl.art2, bigm2, rng, count=4)
        _assert_bottlenecks(eng, pl, pl.flow2)
        _assert_update_rhs_defects(eng, pl, tree, large=True)                              # p = 3: census and path only
    with _engine(e, pl) as fresh:
        assert 1 <= _assert_computed_cut(fresh, pl, np.zeros(pl.m, np.int64), pl.inst.supply) <= 8
