"""The fused LDS loop (``k_solve_small``) keeps its control state in every wave's registers and writes it back once per launch:
what has to survive a launch boundary, and iterations that pivot on nothing, at both compiled widths against the CPU emulation.
The inputs are those of ``small_loop_control_instances.py``; ``test_small_loop_control_cpu.py`` checks them without a GPU.

``mcf_stats`` does not expose ``minor_pivots`` / ``major_sweeps``; ``arcs_priced`` (eight per minor iteration, a whole sweep per
major one) moves with both and is compared after every launch."""

from __future__ import annotations

import numpy as np
import pytest

import small_loop_control_instances as ci
import small_loop_instances as sl

pytestmark = pytest.mark.gpu


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _same_stats(res, em, tag, status=None):
    """`status`: what the engine reports where it knows more than the emulation -- stopped at a budget of exactly the solve's
    pivot count, the kernel's own check at the budget finds no eligible arc and reports optimal; the emulation stops at the limit."""
    want_status = status or em["status"]
    assert res.status == want_status, tag + (res.status, want_status)
    got, want = {k: res.stats[k] for k in ci.STATS}, {k: em[k] for k in ci.STATS}
    assert got == want, tag + (got, want)


def _same_state(res, tree, em, tag):
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"]), tag
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"]), tag


def _chopped(eng, inst, rule, k, tag, block_size=0):
    """solve(k) to the end; after every launch the statistics and the status of the emulation with the same total budget."""
    assert eng.stats()["pricing_mode"] == 2, tag
    P = ci.emul(inst, rule, -1, block_size)["pivots"]
    total = 0
    while True:
        eng.solve(k)
        total += k
        res = eng.result()
        em = ci.emul(inst, rule, total, block_size)
        _same_stats(res, em, tag + (total,), "optimal" if total == P else None)
        if res.status != "iteration_limit":
            break
        assert total < 10 ** 5
    _same_state(res, eng.tree(), em, tag)
    return res


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("k", ci.CHOP_STEPS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("n, m", ci.CHOP_SHAPES)
def test_chopped_solves(gpu_engine_module, monkeypatch, n, m, rule, k, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(n, m)
    with _engine(gpu_engine_module, inst, rule) as eng:
        res = _chopped(eng, inst, rule, k, (inst.name, rule, k, width))
        assert res.status == "optimal"


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_budget_edges(gpu_engine_module, monkeypatch, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(64, 512)
    P = ci.emul(inst, rule)["pivots"]
    for budget, status in ((0, "iteration_limit"), (P - 1, "iteration_limit"), (P, "optimal"), (P + 1, "optimal")):
        with _engine(gpu_engine_module, inst, rule) as eng:
            eng.solve(budget)
            res = eng.result()
            tag = (inst.name, rule, width, budget)
            _same_stats(res, ci.emul(inst, rule, budget), tag, status)
            assert res.stats["pivots"] == min(budget, P), tag
            if budget >= P:
                _same_state(res, eng.tree(), ci.emul(inst, rule), tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_devex_blocks_without_a_candidate(gpu_engine_module, monkeypatch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(64, 512)
    with _engine(gpu_engine_module, inst, 1, block_size=ci.DEVEX_BLOCK) as eng:
        _chopped(eng, inst, 1, 7, (inst.name, "devex", ci.DEVEX_BLOCK, width), block_size=ci.DEVEX_BLOCK)
    with _engine(gpu_engine_module, inst, 1, block_size=ci.DEVEX_BLOCK) as eng:
        eng.solve()
        res = eng.result()
        em = ci.emul(inst, 1, -1, ci.DEVEX_BLOCK)
        _same_stats(res, em, (inst.name, "devex whole", width))
        _same_state(res, eng.tree(), em, (inst.name, "devex whole", width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_optimal_at_the_start_basis(gpu_engine_module, monkeypatch, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = ci.optimal_at_start()
    with _engine(gpu_engine_module, inst, rule) as eng:
        eng.solve()
        res = eng.result()
        assert res.stats["pricing_mode"] == 2 and res.status == "optimal" and res.stats["pivots"] == 0 and res.objective == 0
        _same_stats(res, ci.emul(inst, rule), (inst.name, rule, width))
        cert = eng.certify()
        assert cert["verdict"] == "optimal" and cert["proves_status"]


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("name", sorted(ci.verdict_cases()))
def test_unbounded_and_infeasible(gpu_engine_module, monkeypatch, name, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst, verdict = ci.verdict_cases()[name]
    em = ci.emul(inst, rule)
    with _engine(gpu_engine_module, inst, rule, fused=True) as eng:
        eng.solve()
        res = eng.result()
        tag = (name, rule, width)
        assert res.stats["pricing_mode"] == 2 and res.status == verdict == em["status"], tag + (res.status,)
        assert res.stats["pivots"] == em["pivots"] and res.stats["degenerate"] == em["degenerate"], tag
        assert res.stats["unbounded_arc"] == em["unbounded_arc"] and res.stats["artificial_flow"] == em["artificial_flow"], tag
        _same_state(res, eng.tree(), em, tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_bound_flips_and_degenerate_pivots(gpu_engine_module, monkeypatch, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = ci.capped_transport()
    em = ci.emul(inst, rule)
    with _engine(gpu_engine_module, inst, rule) as eng:
        eng.solve()
        res = eng.result()
        assert res.stats["pricing_mode"] == 2
        _same_stats(res, em, (inst.name, rule, width))
        _same_state(res, eng.tree(), em, (inst.name, rule, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_largest_tree_on_the_fused_path(gpu_engine_module, monkeypatch, rule, width):
    """(No instance above 1 024 tree nodes fits the LDS plan, test_small_loop_control_cpu.py: this one is searched in parallel.)"""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = ci.largest_tree()
    em = ci.emul(inst, rule)
    with _engine(gpu_engine_module, inst, rule) as eng:
        eng.solve()
        res = eng.result()
        assert res.stats["pricing_mode"] == 2, (inst.name, inst.n, inst.m)
        _same_stats(res, em, (inst.name, rule, width))
        _same_state(res, eng.tree(), em, (inst.name, rule, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("k", (1, 7))
def test_chopped_batch_equals_one_by_one(gpu_engine_module, monkeypatch, k, width):
    """The chopped protocol through solve_batch over three instances with mixed rules, against one engine each driven alone."""
    e = gpu_engine_module
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    cases = [(sl.netgen(64, 512), 2), (ci.capped_transport(), 1), (sl.netgen(257, 1028), 0)]
    batch = [_engine(e, i, r) for i, r in cases]
    alone = [_engine(e, i, r) for i, r in cases]
    try:
        assert all(eng.stats()["pricing_mode"] == 2 for eng in batch + alone)
        for _ in range(10 ** 5):
            e.solve_batch(batch, max_pivots=k)
            for eng in alone:
                eng.solve(k)
            rs = [(b.result(), a.result()) for b, a in zip(batch, alone)]
            for (rb, ra), (inst, rule) in zip(rs, cases):
                tag = (inst.name, rule, k, width, ra.stats["pivots"])
                assert rb.status == ra.status, tag
                assert {s: rb.stats[s] for s in ci.STATS} == {s: ra.stats[s] for s in ci.STATS}, tag
            if all(ra.status != "iteration_limit" for _, ra in rs):
                break
        for b, a, (inst, rule) in zip(batch, alone, cases):
            rb, ra, tb, ta = b.result(), a.result(), b.tree(), a.tree()
            assert rb.status == ra.status == "optimal", (inst.name, rule)
            assert np.array_equal(rb.flow, ra.flow) and np.array_equal(rb.potential, ra.potential), (inst.name, rule)
            assert np.array_equal(tb["order"], ta["order"]) and np.array_equal(tb["parent"], ta["parent"]), (inst.name, rule)
    finally:
        for eng in batch + alone:
            eng.close()
