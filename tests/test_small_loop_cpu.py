"""The inputs of ``test_gpu_small_loop.py``, checked without a GPU: they are what they claim to be, fit the fused loop's LDS
plan, and the CPU emulation / ``RefSimplex`` solve them."""

from __future__ import annotations

import numpy as np
import pytest

import oracle
import planted_pivots as pp
import small_loop_instances as sl
from planted_trees import exact_balances, pl_list


def _fits_lds(inst) -> bool:
    """small_plan of csrc/mcf_engine.hip with Devex weights: its estimate, and its sum of 16-byte-rounded pieces against the
    dynamic-LDS limit (the control block counted as 1 KiB, more than it takes).  The GPU tests assert pricing_mode == 2 itself."""
    m_pad = (inst.m + 1023) // 1024 * 1024
    nn, arcw = inst.n + 1, inst.m + inst.n
    r = lambda b: (b + 15) // 16 * 16
    total = 5 * r(m_pad * 4) + r(m_pad) + r(arcw * 16) + r(nn * 8) + 3 * r(nn * 16) + 8 * r(nn * 4) + r((2 * nn + 2) * 16) + 1024
    return m_pad * 21 + arcw * 16 + nn * 112 + 4096 < 150 * 1024 and total <= 158 * 1024


def _emul(inst, rule):
    return oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)


@pytest.mark.parametrize("n, m", sl.NODE_COUNT_SHAPES + sl.PADDING_SHAPES)
def test_netgen_shapes_fit_and_are_solved(n, m):
    inst = sl.netgen(n, m)
    assert (inst.n, inst.m) == (n, m) and _fits_lds(inst)
    ref = oracle.solve_soa(inst, "dantzig")
    for rule in (0, 1, 2):
        em = _emul(inst, rule)
        assert em["status"] == ref["status"] == "optimal" and em["objective"] == int(round(ref["objective"]))


def test_node_counts_straddle_the_passes_of_a_256_lane_workgroup():
    nodes = [n + 1 for n, _ in sl.NODE_COUNT_SHAPES]
    assert nodes == [255, 256, 257, 258, 511, 512, 513, 514]
    assert sorted({-(-x // 256) for x in nodes}) == [1, 2, 3]


def test_padding_shapes_straddle_a_step_of_m_pad():
    assert [(m + 1023) // 1024 for _, m in sl.PADDING_SHAPES] == [1, 2, 2]
    assert [m % 1024 for _, m in sl.PADDING_SHAPES] == [1023, 1, 0]


@pytest.mark.parametrize("m", sl.TRANSPORT_ARCS)
def test_transport_instance_is_skewed_and_optimal(m):
    inst = sl.transport(m)
    assert inst.m == m and _fits_lds(inst)
    assert int(inst.supply.sum()) == 0 and (inst.supply[:32] == -7).all() and (inst.supply[32:] == 1).all()
    assert np.array_equal(inst.tail[:224], np.arange(32, 256)) and (inst.tail >= 32).all()
    per = -(-inst.n // 8)                                        # nodes per head bucket (mcf_topo_per)
    assert (inst.head // per == 0).all(), "every arc lies in the first head bucket"
    assert m > 384, "more arcs in that bucket than either lane map keeps in registers"
    assert (inst.cost >= 1).all() and (inst.cost <= 100).all() and (inst.cap == 256).all()
    ref = oracle.solve_soa(inst, "dantzig")
    for rule in (0, 1, 2):
        em = _emul(inst, rule)
        assert em["status"] == ref["status"] == "optimal" and em["objective"] == int(round(ref["objective"]))


@pytest.mark.parametrize("k", sl.BUCKET_ARCS)
def test_first_bucket_sits_at_the_register_capacity(k):
    inst = sl.bucket_at(k)
    assert _fits_lds(inst) and inst.n == 256
    per = -(-inst.n // 8)
    assert int((inst.head // per == 0).sum()) == k
    assert {319, 320, 321} <= set(sl.BUCKET_ARCS) and {383, 384, 385} <= set(sl.BUCKET_ARCS)      # 32 x 10 and 128 x 3, +-1
    ref = oracle.solve_soa(inst, "dantzig")
    for rule in (0, 1, 2):
        em = _emul(inst, rule)
        assert em["status"] == ref["status"] == "optimal" and em["objective"] == int(round(ref["objective"]))


@pytest.mark.parametrize("n1, n2, ts", sl.SIDE_PARAMS, ids=sl.SIDE_IDS)
def test_side_plants_are_valid_and_reach_the_intended_lengths(n1, n2, ts):
    p = sl.side_plant(n1, n2, ts)
    pl, inst = p.pl, p.inst
    assert inst.n == (138 if n1 < 100 else 266) and _fits_lds(inst)
    assert exact_balances(inst.n, inst.tail, inst.head, pl.flow, inst.supply) == pl_list(pl.art), "conservation"
    assert (pl.flow >= 0).all() and (pl.flow[pl.capped] <= inst.cap[pl.capped]).all()
    assert p.cycle_len == n1 + n2 + 1 and p.deep > 3
    snaps, objective, status, total = sl.side_trajectory(n1, n2, ts)
    s = snaps[0]
    assert (s["entering"], s["leaving"], s["theta"], s["t2"], s["cycle_len"], s["deep"]) == (p.entering, p.leaving, p.theta, p.t2, p.cycle_len, p.deep)
    up = lambda v: len(_path(pl.parent, v, p.join))
    assert sorted((up(p.u), up(p.w))) == sorted((n1, n2))
    assert status == "optimal" and total >= 1
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, max_pivots=1,
                           warm_in_tree=pl.in_tree, warm_at_upper=pl.at_upper)
    assert em["pivots"] == 1 and em["cycle_arcs"] == n1 + n2 + 1 and np.array_equal(em["flow"], s["flow"])
    em = oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0,
                           warm_in_tree=pl.in_tree, warm_at_upper=pl.at_upper)
    assert em["status"] == status and em["objective"] == objective and em["pivots"] == total


def _path(parent, v: int, stop: int) -> list:
    out = []
    while v != stop:
        out.append(v)
        v = int(parent[v])
    return out
