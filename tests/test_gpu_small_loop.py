"""The fused LDS loop (``k_solve_small``) at every compiled workgroup width, against the CPU emulation of the same algorithm and
the planted pivots' reference: the width changes which lane prices which arc, how many passes the node-parallel cycle search
makes and how the per-bucket candidates are reduced -- never a pivot.  ``MCF_SMALL_THREADS`` forces the width (read by
``mcf_create`` for ``solve`` and by ``mcf_solve_batch`` at the call).  The inputs are those of ``small_loop_instances.py``;
``test_small_loop_cpu.py`` checks them without a GPU."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle
import planted_pivots as pp
import small_loop_instances as sl
from conftest import load_synthetic
from test_gpu_planted_pivots import STAT_KEYS, _compare

pytestmark = pytest.mark.gpu

EXACT_STATS = ("pivots", "degenerate", "arcs_priced")


@functools.lru_cache(maxsize=None)
def _emul(inst_key, rule):
    inst = _INSTANCES[inst_key]
    return oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)


_INSTANCES = {}


def _key(inst):
    _INSTANCES.setdefault(inst.name, inst)
    return inst.name


def _solve_at(e, inst, rule, width):
    with pytest.MonkeyPatch.context() as mp:         # (mcf_create reads the environment)
        mp.setenv("MCF_SMALL_THREADS", str(width))
        with e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule) as eng:
            eng.solve()
            return eng.result(), eng.tree()


def _same_as_emulation(res, tree, em, tag):
    assert res.stats["pricing_mode"] == 2, tag
    assert res.status == em["status"] == "optimal", tag
    for k in EXACT_STATS:
        assert res.stats[k] == em[k], tag + (k, res.stats[k], em[k])
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"]), tag
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"]), tag


def _every_width_against_emulation(e, inst, rule):
    em = _emul(_key(inst), rule)
    runs = []
    for width in sl.WIDTHS:
        res, tree = _solve_at(e, inst, rule, width)
        _same_as_emulation(res, tree, em, (inst.name, rule, width))
        runs.append((res, tree))
    (r0, t0) = runs[0]
    for r, t in runs[1:]:                            # (follows from the above; stated because it is the point)
        assert {k: r.stats[k] for k in EXACT_STATS} == {k: r0.stats[k] for k in EXACT_STATS}
        assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential)
        assert np.array_equal(t["order"], t0["order"]) and np.array_equal(t["parent"], t0["parent"])


@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("idx", (0, 3, 6))
def test_parity_on_the_synthetic_goldens(gpu_engine_module, idx, rule):
    _, inst = load_synthetic()[idx]
    _every_width_against_emulation(gpu_engine_module, inst, rule)


@pytest.mark.parametrize("rule", (0, 2))
@pytest.mark.parametrize("n, m", sl.NODE_COUNT_SHAPES)
def test_node_count_against_the_width(gpu_engine_module, n, m, rule):
    _every_width_against_emulation(gpu_engine_module, sl.netgen(n, m), rule)


@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("n, m", sl.PADDING_SHAPES)
def test_padded_arcs_are_never_priced(gpu_engine_module, n, m, rule):
    _every_width_against_emulation(gpu_engine_module, sl.netgen(n, m), rule)


@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("m", sl.TRANSPORT_ARCS)
def test_one_bucket_holds_every_arc(gpu_engine_module, m, rule):
    _every_width_against_emulation(gpu_engine_module, sl.transport(m), rule)


@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("k", sl.BUCKET_ARCS)
def test_bucket_at_the_register_capacity(gpu_engine_module, k, rule):
    _every_width_against_emulation(gpu_engine_module, sl.bucket_at(k), rule)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("n1, n2, ts", sl.SIDE_PARAMS, ids=sl.SIDE_IDS)
def test_ratio_test_across_wave_boundaries_with_ties(gpu_engine_module, n1, n2, ts, width):
    """The planted protocol of test_gpu_planted_pivots.py: set_basis, solve(1) K times next to RefSimplex.step(), solve()."""
    e = gpu_engine_module
    p = sl.side_plant(n1, n2, ts)
    pl, inst = p.pl, p.inst
    n = inst.n
    snaps, objective, status, total = sl.side_trajectory(n1, n2, ts)
    bigm = pp.big_m(inst)
    cid = (n1, n2, ts, width)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCF_SMALL_THREADS", str(width))
        with e.McfEngine(n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=0, fused=True) as eng:
            assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
            res, tree = eng.result(), eng.tree()
            assert np.array_equal(res.flow, pl.flow) and np.array_equal(tree["state"], pl.state)
            assert np.array_equal(tree["parent"][:n], pl.parent) and np.array_equal(tree["pred_arc"][:n], pl.tree_arc)
            assert np.array_equal(tree["pos"][:n], np.arange(1, n + 1)), "labels are the preorder"
            st = res.stats
            assert st["pricing_mode"] == 2
            prev = {k: st[k] for k in STAT_KEYS}
            for j, s in enumerate(snaps, 1):
                eng.solve(1)
                res, tree = eng.result(), eng.tree()
                _compare(cid, j, eng, inst, s, res, tree, bigm)
                st = res.stats
                delta = {k: st[k] - prev[k] for k in STAT_KEYS}
                prev = {k: st[k] for k in STAT_KEYS}
                want = dict(pivots=1, degenerate=int(s["degenerate"]), bound_flips=int(s["flip"]), cycle_arcs=s["cycle_len"], subtree_nodes=s["t2"],
                            cycle_scans=0)
                assert {k: delta[k] for k in want} == want, (cid, j, delta)
                if j == 1:
                    assert delta["cycle_arcs"] == n1 + n2 + 1 and s["deep"] > 3, "the pivot reached the intended path lengths, by the parallel search"
            eng.solve()
            res = eng.result()
            assert res.status == status and res.objective == objective and res.stats["pivots"] == total, cid
            cert = eng.certify()
            assert cert["verdict"] == status and cert["proves_status"]


def _batch_cases():
    insts = [sl.netgen(254, 1016), sl.netgen(257, 1028), sl.netgen(513, 1026), sl.netgen(256, 1023), sl.netgen(256, 2048),
             sl.transport(1024), sl.transport(2049), load_synthetic()[3][1]]
    return list(zip(insts, (0, 2, 0, 1, 2, 0, 2, 1)))


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_batch_equals_one_by_one(gpu_engine_module, width):
    e = gpu_engine_module
    cases = _batch_cases()
    with pytest.MonkeyPatch.context() as mp:         # (mcf_solve_batch reads the environment at the call)
        mp.setenv("MCF_SMALL_THREADS", str(width))
        single = [_solve_at(e, inst, rule, width) for inst, rule in cases]
        engines = [e.McfEngine(i.n, i.tail, i.head, i.cost, i.cap, i.supply, rule=rule) for i, rule in cases]
        try:
            assert all(eng.stats()["pricing_mode"] == 2 for eng in engines)
            e.solve_batch(engines)
            for eng, (r0, t0), (inst, rule) in zip(engines, single, cases):
                r, t = eng.result(), eng.tree()
                tag = (inst.name, rule, width)
                assert r.status == r0.status == "optimal" and r.objective == r0.objective, tag
                assert {k: r.stats[k] for k in EXACT_STATS} == {k: r0.stats[k] for k in EXACT_STATS}, tag
                assert np.array_equal(r.flow, r0.flow) and np.array_equal(r.potential, r0.potential), tag
                assert np.array_equal(t["order"], t0["order"]) and np.array_equal(t["parent"], t0["parent"]), tag
        finally:
            for eng in engines:
                eng.close()
