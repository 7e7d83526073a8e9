"""The yardstick of ``test_gpu_passes_geometry.py`` tested without a device: ``planted_trees`` builds instances, bases and
expected answers; here they are held against plain Python-int restatements, against the host repair (``mcf_repair_basis``:
the planted basis is kept whole, arc for arc, in every case the GPU file uses), against the host restatements of the
certificate and the witnesses, and ``mcf_apply_basis`` is taken to the edge of 64 bits.  Every comparison is exact."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import planted_trees as pt
import test_certify_cpu as tcc
import test_farkas_cpu as tfc
import test_update_rhs_cpu as tur

MCF_INF = 1 << 60
SIZES = (1, 2, 3, 64, 257, 2049)


@pytest.fixture(scope="module")
def repair_lib():
    lib = ctypes.CDLL(str(ge.build_repair_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    lib.mcf_repair_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i8p, i8p, i8p,
                                    i32p, i32p, i8p, i32p, i8p, i64p, i64p, i64p, ctypes.c_char_p, ctypes.c_int32]
    lib.mcf_repair_host.restype = ctypes.c_int
    lib.mcf_apply_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i8p, i8p, i8p, i64p, i64p, ctypes.c_char_p, ctypes.c_int32]
    lib.mcf_apply_host.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def cert_lib():
    lib = ctypes.CDLL(str(ge.build_certify_host()))
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.mcf_certify_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i64p, i64p, ctypes.c_uint32, i64p]
    lib.mcf_certify_host.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def farkas_lib():
    lib = ctypes.CDLL(str(ge.build_farkas_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    lib.mcf_ray_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i32p, i32p, i32p, i32p, i32p, i64p, i64p,
                                 ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, i64p, ctypes.c_int64, i64p]
    lib.mcf_ray_host.restype = ctypes.c_int
    lib.mcf_cut_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i64p, i8p, ctypes.c_int64, i8p, i64p]
    lib.mcf_cut_host.restype = ctypes.c_int
    return lib


def _apply(lib, inst, in_tree, at_upper):
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    arr = lambda a, t: np.ascontiguousarray(a, t)                                            # noqa: E731
    state, flow, art = np.zeros(max(inst.m, 1), np.int8), np.zeros(max(inst.m, 1), np.int64), np.zeros(inst.n, np.int64)
    err = ctypes.create_string_buffer(256)
    p = tur._p
    rc = lib.mcf_apply_host(inst.n, inst.m, p(arr(inst.tail, np.int32), i32), p(arr(inst.head, np.int32), i32), p(arr(inst.cost, np.int64), i64),
                            p(arr(inst.cap, np.int64), i64), p(arr(inst.supply, np.int64), i64), p(arr(in_tree, np.int8), i8), p(arr(at_upper, np.int8), i8),
                            p(state, i8), p(flow, i64), p(art, i64), err, 256)
    return rc, err.value.decode(), state[: inst.m], flow[: inst.m], art


def _kept_whole(lib, pl, supply=None, flow=None, art=None):
    """mcf_repair_basis on the planted basis: nothing cut, the planted flows, the planted parents."""
    supply, flow, art = (pl.inst.supply if supply is None else supply), (pl.flow if flow is None else flow), (pl.art if art is None else art)
    rc, msg, out = tur._repair(lib, pl.inst, supply, pl.inst.cap, pl.in_tree, pl.at_upper)
    assert rc == 0, msg
    assert out["report"].tolist()[:3] == [0, 0, 0], out["report"]
    assert np.array_equal(out["flow"], flow) and np.array_equal(out["state"], pl.state)
    assert np.array_equal(out["art_flow"], np.abs(art))
    assert np.array_equal(out["parent"][: pl.n], pl.parent) and np.array_equal(out["pred_arc"][: pl.n], pl.tree_arc)
    return out


def _tree_of(pl, out) -> dict:
    """The arrays mcf_get_tree reports, from the repair's parent / order."""
    N = pl.n + 1
    order = out["order"].tolist()
    parent = out["parent"].tolist()
    pos, size, depth = [0] * N, [1] * N, [0] * N
    for k, v in enumerate(order):
        pos[v] = k
        if parent[v] >= 0:
            depth[v] = depth[parent[v]] + 1
    for v in reversed(order[1:]):
        size[parent[v]] += size[v]
    return {"parent": out["parent"], "pred_arc": out["pred_arc"], "order": out["order"], "pos": np.array(pos, np.int32),
            "size": np.array(size, np.int32), "depth": np.array(depth, np.int32)}


# ------------------------------------------------------------------ conservation, bounds, the basis kept
@pytest.mark.parametrize("shape", pt.SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_planted_instances_conserve_flow_and_stay_in_bounds(repair_lib, shape, n):
    """plant() checks itself on numpy; the same once more on Python ints, for both vectors, and the host repair keeps the basis."""
    magnitudes = ("small", "wide") if shape == "forest" and n >= 257 else ("small",)     # (wide needs 80 components and more)
    for magnitude in magnitudes:
        pl = pt.plant(shape, n, seed=5, magnitude=magnitude, k=96 if magnitude == "wide" else 3)
        T, H, U = pl.inst.tail.tolist(), pl.inst.head.tolist(), pl.inst.cap.tolist()
        assert pl.m == (2 * n if n > 1 else 0) and int(pl.in_tree.sum()) + int((pl.parent == n).sum()) == n
        for supply, flow, art in ((pl.inst.supply, pl.flow, pl.art), (pl.supply2, pl.flow2, pl.art2)):
            bal = [int(s) for s in supply.tolist()]
            for t, h, u, f, basic, au in zip(T, H, U, flow.tolist(), pl.in_tree.tolist(), pl.at_upper.tolist()):
                bal[t] -= f
                bal[h] += f
                capped = 0 <= u < MCF_INF
                assert 0 < f < (u if capped else MCF_INF) if basic else f == (u if au else 0)
            assert bal == [int(a) for a in art.tolist()] and sum(bal) == 0
            assert all(a == 0 for v, a in enumerate(bal) if pl.parent[v] != n)
            assert sum(s for s in supply.tolist() if s > 0) < MCF_INF
            _kept_whole(repair_lib, pl, supply, flow, art)
        if magnitude == "wide":
            assert pt.max_prefix(pl, pl.art) > 1 << 64 and max(pl.flow.tolist()) < MCF_INF
            run = [0]
            for a in pl.art[pl.parent == n].tolist():
                run.append(run[-1] + a)
            assert max(abs(r) for r in run) == pt.max_prefix(pl, pl.art)
            same = [a > 0 for a in pl.art[pl.parent == n].tolist()]
            assert any(all(same[i: i + 40]) or not any(same[i: i + 40]) for i in range(len(same) - 39))   # 40 components in a row, one sign


def test_every_case_of_the_gpu_file_is_kept_whole_by_the_host_repair(repair_lib):
    """The condition that lets the GPU tests assert "no arc was dropped": violations = wrong_way = arcs_cut = 0 and the planted
    flows, for both planted vectors of every case (the defect vectors are the GPU file's business: they are meant to be cut)."""
    cases = [pt.sweep_plant(n, shape, m) for _, n, shape, _, m in pt.sweep_cases()] + [pt.depth_plant(d) for d in pt.DEPTHS if d > 1] + [pt.cold_plant()]
    for pl in cases:
        _kept_whole(repair_lib, pl)
        _kept_whole(repair_lib, pl, pl.supply2, pl.flow2, pl.art2)


@pytest.mark.parametrize("which", ["random", "caterpillar", "scan"])
def test_the_large_cases_of_the_gpu_file_are_kept_whole(repair_lib, which):
    pl = pt.scan_plant() if which == "scan" else pt.large_plant(which)
    _kept_whole(repair_lib, pl)
    _kept_whole(repair_lib, pl, pl.supply2, pl.flow2, pl.art2)
    if which == "scan":
        S, levels = pt.residual_levels(pl, np.zeros(pl.m, np.int64), pl.inst.supply)
        assert 1 <= levels <= 8                                          # the computed cut of the GPU test: a handful of rounds, no chain


def test_defects_are_planted_where_the_helper_says(repair_lib):
    """The second vector with defects: p tree arcs outside their bounds, q basic arcs on a bound; the wrong-way count follows the
    orientation, and the host repair finds something to cut."""
    for p, q in pt.DEFECTS:
        pl = pt.sweep_plant(257, "random", 4097, p, q)
        tree = _tree_of(pl, _kept_whole(repair_lib, pl))
        f2, cap = pl.flow3, np.where(pl.capped, pl.inst.cap, MCF_INF)
        assert len(pl.out_of_bounds) == p and ((f2 < 0) | (f2 > cap))[pl.out_of_bounds].all()
        assert len(pl.on_bound) == q and ((f2 == 0) | (f2 == cap))[pl.on_bound].all()
        assert int(((f2 < 0) | (f2 > cap)).sum()) == p and int((pl.in_tree & ((f2 == 0) | (f2 == cap))).sum()) == q
        child_is_tail = pl.parent[pl.inst.tail[pl.on_bound]] == pl.inst.head[pl.on_bound]           # parent[v] < v: the child is the higher node
        assert (child_is_tail == (pl.inst.tail[pl.on_bound] > pl.inst.head[pl.on_bound])).all()
        want = int((np.where(child_is_tail, f2[pl.on_bound] == cap[pl.on_bound], f2[pl.on_bound] == 0)).sum())
        assert pt.wrong_way(pl, tree, pl.on_bound, f2) == want
        rc, msg, out = tur._repair(repair_lib, pl.inst, pl.supply3, pl.inst.cap, pl.in_tree, pl.at_upper)
        assert rc == 0 and out["report"][0] >= 1 and out["report"][2] == out["report"][0] + out["report"][1], (msg, out["report"])


# ------------------------------------------------------------------ the yardstick against the host restatements
@pytest.mark.parametrize("shape", pt.SHAPES)
@pytest.mark.parametrize("n", (2, 3, 64, 257))
def test_yardsticks_agree_with_the_host_code(repair_lib, cert_lib, farkas_lib, shape, n):
    pl = pt.plant(shape, n, seed=9)
    inst = pl.inst
    tree = _tree_of(pl, _kept_whole(repair_lib, pl))
    pt.check_tree_arrays(n, tree["parent"], tree["size"], tree["pos"], tree["order"], tree["depth"])
    bigm = pt.big_m(pl)
    pi = pt.potentials(pl, tree, inst.cost, bigm)
    # potentials by the plain recurrence, in preorder
    want = [0] * (n + 1)
    for v in tree["order"].tolist()[1:]:
        a, par = int(tree["pred_arc"][v]), int(tree["parent"][v])
        c = bigm if a >= pl.m else int(inst.cost[a])
        up = pl.art[v] >= 0 if a >= pl.m else int(inst.tail[a]) == v
        want[v] = want[par] - c if up else want[par] + c
    assert pi.tolist() == want
    # certificate: the caller's-arrays groups against the host restatement and the Python-int one
    got = tcc.certify_host(cert_lib, inst, pl.flow, pi[:n])
    mine = pt.np_cert(inst, inst.cost, pl.flow, pi[:n])
    assert {k: got[k] for k in mine} == mine == {k: tcc.int_cert(inst, pl.flow, pi[:n])[k] for k in mine}
    full = pt.certificate(pl, inst.cost, pl.flow, pi, pl.art, bigm)
    assert full["imbalance_count"] == 0 and full["artificial_flow"] == int(np.abs(pl.art).sum())
    assert full["gap"] == full["primal"] + bigm * full["artificial_flow"] - full["dual"]
    # rays: every non-basic arc (at most 32), against the host restatement of the kernels' interval method
    r = dict(tree, potential=pi[:n], flow=pl.flow)
    walker = pt.RayWalker(pl, tree, inst.cost, pl.flow, pi, pl.art, bigm)
    for arc in np.flatnonzero(~pl.in_tree)[:32].tolist():
        backward = bool(pl.at_upper[arc])
        assert tfc.ray_host(farkas_lib, inst, r, arc, backward, pl.art, chunk=7) == walker.ray(arc, backward), arc
    # cuts: caller's sets and the search
    rng = np.random.default_rng(n)
    for S in (np.zeros(n, bool), pt.subtree_set(pl, n // 2), rng.random(n) < 0.5):
        got = tfc.cut_host(farkas_lib, inst, in_S=S.astype(np.int8))
        want = pt.cut_answer(pl, S)
        assert {k: got[k] for k in want} == want
    for flow, art in ((pl.flow, pl.art), (np.zeros(pl.m, np.int64), inst.supply)):
        got = tfc.cut_host(farkas_lib, inst, flow, art)
        S, levels = pt.residual_levels(pl, flow, art)
        want = pt.cut_answer(pl, S, flow=flow, art=art, rounds=levels)
        assert np.array_equal(got["S"], S) and {k: got[k] for k in want} == want


def test_bottleneck_lists_and_exact_sums():
    pl = pt.plant("forest", 600, 2000, seed=3, magnitude="wide", k=96)
    U, F = pl.inst.cap.tolist(), pl.flow.tolist()
    for num, den in ((1, 1), (19, 20), (1, 2)):
        want = [i for i, (u, f) in enumerate(zip(U, F)) if 0 <= u < MCF_INF and f > 0 and f * den >= u * num]
        assert pt.bottleneck_list(pl, pl.flow, num, den).tolist() == want and len(want) >= int(pl.at_upper.sum())
    assert pt.exact_sum(pl.flow) == sum(F) and pt.exact_dot(pl.flow, pl.inst.cost) == sum(f * c for f, c in zip(F, pl.inst.cost.tolist()))
    assert pt.exact_dot(-pl.flow, pl.flow) == -sum(f * f for f in F)


# ------------------------------------------------------------------ mcf_apply_basis at the edge of 64 bits
def test_apply_basis_accepts_sixteen_arcs_at_capacity_with_their_own_returns(repair_lib):
    """(a) node 0's balance is about -2^64, every flow is below 2^60: the basis is valid and has to be installed as planted."""
    inst, in_tree, at_upper, flow = pt.int64_edge(16, shared_return=False)
    assert inst.n < 40 and -sum(flow[at_upper].tolist()) < -(1 << 63) and int(flow.max()) < MCF_INF
    rc, msg, state, got, art = _apply(repair_lib, inst, in_tree, at_upper)
    assert rc == 0, msg
    assert np.array_equal(got, flow) and np.array_equal(state, np.where(in_tree, 0, -1)) and not art.any()
    rc, msg, out = tur._repair(repair_lib, inst, inst.supply, inst.cap, in_tree, at_upper)
    assert rc == 0 and np.array_equal(out["flow"], flow) and out["report"].tolist()[:3] == [0, 0, 0]


def test_apply_basis_refuses_a_return_flow_of_seventeen_times_the_capacity(repair_lib):
    """(b) the hub's tree arc would carry 17 * (2^60 - 1): in 64 bits that surplus wraps to 2^60 - 22, which passes the bounds
    check of an uncapacitated arc.  The basis has to be refused and the image left at the cold start."""
    inst, in_tree, at_upper, _ = pt.int64_edge(17, shared_return=True)
    assert inst.n < 40 and (17 * (MCF_INF - 1) - 5) % (1 << 64) == MCF_INF - 22
    rc, msg, state, flow, art = _apply(repair_lib, inst, in_tree, at_upper)
    assert rc == 1 and "incompatible" in msg, (rc, msg)
    assert (state == 1).all() and not flow.any() and np.array_equal(art, np.abs(inst.supply))      # the cold start
    rc, msg, _ = tur._repair(repair_lib, inst, inst.supply, inst.cap, in_tree, at_upper)
    assert rc == 1 and "2^60" in msg                                                                # the repair says the same
