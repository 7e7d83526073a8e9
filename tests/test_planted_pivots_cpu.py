"""The planted pivots of ``planted_pivots.py`` and its reference simplex, checked without a GPU: every case really is what it
claims to be (recomputed from scratch), and ``RefSimplex`` -- written from the documented rules -- and the CPU emulation --
compiled from the kernels' own header -- make the same pivots on it."""

from __future__ import annotations

import numpy as np
import pytest

import oracle
import planted_pivots as pp
from planted_trees import MCF_INF, exact_balances, exact_sum, pl_list


def _emul(p: pp.PivotPlant, max_pivots: int) -> dict:
    inst = p.inst
    return oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, max_pivots=max_pivots,
                             warm_in_tree=p.pl.in_tree, warm_at_upper=p.pl.at_upper)


def _subtree_size(parent, top: int, n: int) -> int:
    inside = np.zeros(n + 1, bool)
    inside[top] = True
    par = parent.tolist()
    for v in range(top + 1, n):          # labels are preorder numbers: parent[v] < v
        inside[v] = inside[par[v]]
    return int(inside.sum())


def _path_up(parent, v: int, stop: int) -> list:
    out = []
    while v != stop:
        out.append(v)
        v = int(parent[v])
    return out


@pytest.mark.parametrize("cid", pp.CASE_IDS)
def test_case_is_what_it_claims(cid):
    """Conservation, the numeric domain, flows inside their bounds, and |T2|, stem, cycle length, blocking arc and Dantzig's
    choice recomputed from the arrays alone; the emulation's host walk installs the basis whole, at the planted positions."""
    p = pp.planted(cid)
    pl, inst, args = p.pl, p.inst, p.args
    n, m = inst.n, inst.m
    assert exact_balances(n, inst.tail, inst.head, pl.flow, inst.supply) == pl_list(pl.art), "conservation"
    assert exact_sum(inst.supply) == 0 and exact_sum(inst.supply[inst.supply > 0]) < MCF_INF
    assert (np.abs(inst.cost) <= pp.INT32_MAX).all() and (np.abs(inst.cost[pl.in_tree]) <= 100).all()
    capped = pl.capped
    assert (pl.flow >= 0).all() and (pl.flow[capped] <= inst.cap[capped]).all()
    assert (pl.flow[~pl.in_tree] == np.where(pl.at_upper, inst.cap, 0)[~pl.in_tree]).all()
    # ---- Dantzig's choice, from potentials computed here (labels are preorder numbers: one pass in label order)
    bigm = pp.big_m(inst)
    pi = np.zeros(n + 1, np.int64)
    par, arc = pl.parent.tolist(), pl.tree_arc.tolist()
    pil = pi.tolist()
    for v in range(n):
        if arc[v] >= m:
            pil[v] = -bigm if pl.art[v] >= 0 else bigm
        else:
            c = int(inst.cost[arc[v]])
            pil[v] = pil[par[v]] - c if int(inst.tail[arc[v]]) == v else pil[par[v]] + c
    pi = np.array(pil, np.int64)
    viol = -pl.state.astype(np.int64) * (inst.cost + pi[inst.tail] - pi[inst.head])
    best = int(viol.max())
    winners = np.flatnonzero(viol == best)
    assert winners[0] == p.entering and best > 0
    assert len(winners) == (2 if args["equal_violation"] else 1)
    assert len(np.unique(viol[viol > 0])) == int((viol > 0).sum()) - (1 if args["equal_violation"] else 0), "violations are distinct"
    assert int((viol > 0).sum()) == 1 if args["lone"] else int((viol > 0).sum()) >= 8
    assert best == pp.V0 or (args["through_root"] and best > bigm)
    # ---- the cycle and its residuals
    fwd = pl.state[p.entering] > 0
    assert fwd != args["backward"]
    first, second = (int(inst.tail[p.entering]), int(inst.head[p.entering])) if fwd else (int(inst.head[p.entering]), int(inst.tail[p.entering]))
    assert (first, second) == (p.first, p.second) and {first, second} == {p.u, p.w}
    anc = set(_path_up(pl.parent, first, n)) | {n}
    join = second
    while join not in anc:
        join = int(pl.parent[join])
    assert join == p.join and (join == n) == args["through_root"]
    side1, side2 = _path_up(pl.parent, first, join), _path_up(pl.parent, second, join)
    assert len(side1) + len(side2) + 1 == p.cycle_len == args["stem"] + args["above"] + args["other"] + 2

    def residual(v, second_side):
        a = arc[v]
        if a >= m:
            up, cap, f = pl.art[v] >= 0, None, abs(int(pl.art[v]))
        else:
            up, cap, f = int(inst.tail[a]) == v, (int(inst.cap[a]) if capped[a] else None), int(pl.flow[a])
        gains = up == second_side
        return (MCF_INF if cap is None else cap - f) if gains else f
    r1, r2 = [residual(v, False) for v in side1], [residual(v, True) for v in side2]
    re = int(inst.cap[p.entering]) if capped[p.entering] else MCF_INF
    theta = min(r1 + r2 + [re])
    assert theta == p.theta == (0 if args["theta0"] else pp.THETA)
    blocking = {"first": theta in r1, "entering": re == theta, "second": theta in r2}
    if args["ties"]:
        assert {k for k, b in blocking.items() if b} == set(args["ties"])
        assert sum(r == theta for r in r1) != 1 and sum(r == theta for r in r2) != 1, "a tying side holds two blocking arcs"
    else:
        assert sum(blocking.values()) == 1 and (r1 + r2 + [re]).count(theta) == 1
    # the documented rule: the last blocking arc from the join along first side (downwards), entering arc, second side (upwards)
    if blocking["second"]:
        leaver = arc[[v for v, r in zip(side2, r2) if r == theta][-1]]
    elif blocking["entering"]:
        leaver = p.entering
    else:
        leaver = arc[[v for v, r in zip(side1, r1) if r == theta][0]]
    assert leaver == p.leaving
    if p.leaving == p.entering:
        assert p.t2 == 0 and args["leave"] == "entering"
    else:
        assert leaver == arc[p.a] and (leaver >= m) == args["leave"].startswith("artificial")
        assert _subtree_size(pl.parent, p.a, n) == p.t2 == args["t2"]
        assert len(_path_up(pl.parent, p.u, p.a)) == p.stem == args["stem"]
        assert p.u in (side1[0] if side1 else -1, side2[0] if side2 else -1)
    # every other tree flow strictly inside its bounds
    loose = pl.in_tree.copy()
    on_cycle = [arc[v] for v in side1 + side2 if arc[v] < m]
    loose[on_cycle] = False
    assert (pl.flow[loose] > 0).all() and (pl.flow[loose & capped] < inst.cap[loose & capped]).all()
    for v, r in zip(side1 + side2, r1 + r2):
        assert r == theta or (r > theta and (arc[v] >= m or 0 < pl.flow[arc[v]]))
    # ---- the host walk keeps the basis whole and puts the nodes where the construction says
    em = _emul(p, 0)
    assert em["warm_applied"] and em["pivots"] == 0
    assert np.array_equal(em["flow"], pl.flow) and np.array_equal(em["in_tree"].astype(bool), pl.in_tree)
    assert np.array_equal(em["parent"][:n], pl.parent)
    assert np.array_equal(em["pos"][:n], np.arange(1, n + 1)), "labels are the preorder"
    if args["align"] is not None:
        k, d = args["align"]
        assert (p.pos_a - d) % (1 << k) == 0
    if args["tail_end"]:
        assert p.pos_a + p.t2 == n + 1
    assert (p.pos_w < p.pos_a) == (args["direction"] == "before" or args["other"] == 0) or p.t2 == 0
    depth = em["depth"]
    assert p.deep == max(int(depth[p.u]), int(depth[p.w]))


@pytest.mark.parametrize("cid", pp.CASE_IDS)
def test_reference_and_emulation_make_the_same_pivots(cid):
    """RefSimplex against oracle.emul_solve(max_pivots=j) for j = 1 .. K: flows, potentials, parents, pivot, degenerate and flip
    counts, cycle lengths and subtree sizes; the first pivot is the planted one."""
    p = pp.planted(cid)
    n = p.inst.n
    snaps, objective, status, total = pp.trajectory(cid)
    assert len(snaps) == min(pp.K_PIVOTS, total) and total >= 1
    assert total == 1 or not p.args["lone"], "a lone planted pivot is the whole solve"
    s = snaps[0]
    assert (s["entering"], s["leaving"], s["theta"], s["t2"], s["cycle_len"], s["deep"]) == (p.entering, p.leaving, p.theta, p.t2, p.cycle_len, p.deep)
    assert s["flip"] == (p.t2 == 0) and s["degenerate"] == (p.theta == 0)
    deg = flips = cyc = sub = 0
    for j, s in enumerate(snaps, 1):
        em = _emul(p, j)
        deg, flips, cyc, sub = deg + s["degenerate"], flips + s["flip"], cyc + s["cycle_len"], sub + s["t2"]
        assert (em["pivots"], em["degenerate"], em["bound_flips"], em["cycle_arcs"], em["subtree_nodes"]) == (j, deg, flips, cyc, sub), (cid, j)
        assert np.array_equal(em["flow"], s["flow"]), (cid, j)
        assert np.array_equal(em["in_tree"] != 0, s["state"] == 0)
        assert np.array_equal(em["potential"], s["potential"][:n])
        for k in ("parent", "pred_arc", "depth", "size"):
            assert np.array_equal(em[k], s[k]), (cid, j, k)
        assert em["artificial_flow"] == int(s["art_flow"].sum())
    em = _emul(p, -1)
    assert em["status"] == status and em["objective"] == objective and em["pivots"] == total


@pytest.mark.parametrize("cid", [c for c in pp.CASE_IDS if pp.planted(c).inst.n <= 2000])
def test_reference_reaches_the_restated_simplex_objective(cid):
    p = pp.planted(cid)
    _, objective, status, _ = pp.trajectory(cid)
    ref = oracle.solve_soa(p.inst, strategy="dantzig", reference_order=False)
    assert ref["status"] == status
    if status == "optimal":
        assert ref["objective"] == objective


def test_case_table_covers_every_constant():
    """Below / at / above for every in-kernel capacity, by the arithmetic of the cases themselves."""
    t2s = {pp.BY_ID[c][1]["t2"] for c in pp.CASE_IDS}
    stems = {pp.BY_ID[c][1]["stem"] for c in pp.CASE_IDS}
    cycles = {pp.planted(c).cycle_len for c in pp.CASE_IDS if not c.startswith(("t2_8", "align_8", "after_8", "same_block_8", "tail_end_8", "blocks"))}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193} <= t2s
    assert {1, 127, 128, 129, 511, 512, 513} <= stems
    assert {511, 512, 513, 514, 4095, 4096, 4097, 4098} <= cycles
    for ts in pp.TIE_SETS:
        assert "ties_" + "_".join(ts) in pp.BY_ID
