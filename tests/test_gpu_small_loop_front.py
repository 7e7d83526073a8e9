"""The front of a pivot in the fused LDS loop (``k_solve_small``): 32-bit pricing keys where ``mcf_small_narrow_ok`` allows them,
64-bit ones otherwise or under ``MCF_SMALL_NARROW=0``, and an arg-max that hands the winner's record to ``begin``.  Both paths
against the CPU emulation -- statistics, flow, potential, order, parent -- at both compiled widths.  Inputs:
``small_loop_front_instances.py``; ``test_small_loop_front_cpu.py`` checks them without a GPU."""

from __future__ import annotations

import numpy as np
import pytest

import small_loop_control_instances as ci
import small_loop_front_instances as fi
import small_loop_instances as sl

pytestmark = pytest.mark.gpu


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _same(res, tree, em, tag, status=None):
    assert res.status == (status or em["status"]), tag + (res.status, em["status"])
    got, want = {k: res.stats[k] for k in ci.STATS}, {k: em[k] for k in ci.STATS}
    assert got == want, tag + (got, want)
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"]), tag
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"]), tag


def _whole(e, inst, rule, narrow, tag):
    with _engine(e, inst, rule) as eng:
        assert eng.stats()["pricing_mode"] == 2 and eng.stats()["small_narrow"] == 0, tag   # (no launch yet)
        eng.solve()
        res = eng.result()
        assert res.stats["small_narrow"] == narrow, tag
        _same(res, eng.tree(), ci.emul(inst, rule), tag)


def _stepped(e, inst, rule, narrow, steps, tag):
    """solve(1) launches: after each the whole state of the emulation with that budget, which pins the entering arc."""
    P = ci.emul(inst, rule)["pivots"]
    with _engine(e, inst, rule) as eng:
        for k in range(1, steps + 1):
            eng.solve(1)
            res = eng.result()
            assert res.stats["small_narrow"] == narrow, tag + (k,)
            _same(res, eng.tree(), ci.emul(inst, rule, k), tag + (k,), "optimal" if k == P else None)
            if res.status != "iteration_limit":
                break


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("switch", (None, "0"))
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("n, m", fi.SHAPES)
def test_narrow_and_wide_equal_the_emulation(gpu_engine_module, monkeypatch, n, m, rule, switch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    if switch is None:
        monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    else:
        monkeypatch.setenv("MCF_SMALL_NARROW", switch)
    inst = sl.netgen(n, m)
    narrow = 1 if switch is None else 0
    tag = (inst.name, rule, switch, width)
    _whole(gpu_engine_module, inst, rule, narrow, tag)
    _stepped(gpu_engine_module, inst, rule, narrow, fi.STEPS, tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("above", (0, 1))
def test_the_edge_of_the_range(gpu_engine_module, monkeypatch, above, rule, width):
    """max|cost| at the largest value the predicate accepts (32-bit keys, violations above 2^30) and one above it (64-bit keys);
    negative costs included."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    inst = fi.edge(above)
    tag = (inst.name, rule, width)
    _whole(gpu_engine_module, inst, rule, 1 - above, tag)
    _stepped(gpu_engine_module, inst, rule, 1 - above, 12, tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("switch", (None, "0"))
@pytest.mark.parametrize("rule", (0, 2))
def test_ties_on_the_unit_grid(gpu_engine_module, monkeypatch, rule, switch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    if switch is None:
        monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    else:
        monkeypatch.setenv("MCF_SMALL_NARROW", switch)
    inst = fi.unit_grid()
    P = ci.emul(inst, rule)["pivots"]
    _stepped(gpu_engine_module, inst, rule, 1 if switch is None else 0, P + 1, (inst.name, rule, switch, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("switch", (None, "0"))
@pytest.mark.parametrize("rule", (0, 2))
@pytest.mark.parametrize("name", ("bucket_385", "transport_1024"))
def test_bucket_fuller_than_the_register_slots(gpu_engine_module, monkeypatch, name, rule, switch, width):
    """The LDS tail of the sweep competes with the register arcs, in the packed form and in the 64-bit one."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    if switch is None:
        monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    else:
        monkeypatch.setenv("MCF_SMALL_NARROW", switch)
    inst = sl.bucket_at(385) if name == "bucket_385" else sl.transport(1024)
    narrow = 1 if switch is None else 0
    tag = (inst.name, rule, switch, width)
    _whole(gpu_engine_module, inst, rule, narrow, tag)
    _stepped(gpu_engine_module, inst, rule, narrow, 12, tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("switch", (None, "0"))
@pytest.mark.parametrize("rule", (0, 2))
def test_chopped_solves_and_budget_edges(gpu_engine_module, monkeypatch, rule, switch, width):
    """The candidate record crosses LDS at every pivot, and an iteration that pivots on nothing follows one that does."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    if switch is None:
        monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    else:
        monkeypatch.setenv("MCF_SMALL_NARROW", switch)
    e = gpu_engine_module
    inst = fi.edge(0)
    P = ci.emul(inst, rule)["pivots"]
    for k in (1, 7):
        with _engine(e, inst, rule) as eng:
            total = 0
            while True:
                eng.solve(k)
                total += k
                res = eng.result()
                em = ci.emul(inst, rule, total)
                tag = (inst.name, rule, switch, width, k, total)
                assert res.status == ("optimal" if total == P else em["status"]), tag
                assert {s: res.stats[s] for s in ci.STATS} == {s: em[s] for s in ci.STATS}, tag
                if res.status != "iteration_limit":
                    break
                assert total < 10 ** 5
            _same(res, eng.tree(), em, tag, "optimal")
    for budget, status in ((P - 1, "iteration_limit"), (P, "optimal"), (P + 1, "optimal")):
        with _engine(e, inst, rule) as eng:
            eng.solve(budget)
            res = eng.result()
            _same(res, eng.tree(), ci.emul(inst, rule, budget), (inst.name, rule, switch, width, "budget", budget), status)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 2))
def test_update_costs_takes_a_resident_handle_across_the_edge(gpu_engine_module, monkeypatch, rule, width):
    """Narrow, then -- one cost raised so that big-M leaves the range -- wide; big-M never shrinks (mcf_update_costs), so the
    handle stays wide when the cost comes back down.  Each time the result of a fresh handle on the same costs."""
    e = gpu_engine_module
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    inst = sl.netgen(64, 512)
    arc = int(np.argmax(np.abs(inst.cost)))
    raised = inst.cost.copy()
    raised[arc] = fi.edge_cost(inst.n) + 1

    def fresh(cost):
        with e.McfEngine(inst.n, inst.tail, inst.head, cost, inst.cap, inst.supply, rule=rule) as f:
            f.solve()
            return f.result()

    with _engine(e, inst, rule) as eng:
        eng.solve(10)
        assert eng.stats()["small_narrow"] == 1
        eng.solve()
        r0 = eng.result()
        _same(r0, eng.tree(), ci.emul(inst, rule), (inst.name, rule, width, "before"))
        for cost, narrow_fresh, step in ((raised, 0, "raised"), (inst.cost, 1, "back down")):
            eng.update_costs(np.array([arc]), np.array([cost[arc]]))
            eng.solve()
            res, want = eng.result(), fresh(cost)
            tag = (inst.name, rule, width, step)
            assert res.stats["small_narrow"] == 0 and want.stats["small_narrow"] == narrow_fresh, tag
            assert res.status == want.status == "optimal" and res.objective == want.objective, tag
            cert = eng.certify()
            assert cert["verdict"] == "optimal" and cert["proves_status"], tag


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_batch_mixing_both_sides_of_the_edge(gpu_engine_module, monkeypatch, width):
    e = gpu_engine_module
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.delenv("MCF_SMALL_NARROW", raising=False)
    cases = [(fi.edge(0), 0, 1), (fi.edge(1), 0, 0), (sl.netgen(64, 512), 2, 1), (fi.edge(1), 2, 0), (fi.unit_grid(), 0, 1), (sl.netgen(256, 2048), 1, 1)]
    batch = [_engine(e, i, r) for i, r, _ in cases]
    try:
        e.solve_batch(batch)
        for eng, (inst, rule, narrow) in zip(batch, cases):
            res = eng.result()
            assert res.stats["small_narrow"] == narrow, (inst.name, rule, width)
            _same(res, eng.tree(), ci.emul(inst, rule), (inst.name, rule, width, "batch"))
    finally:
        for eng in batch:
            eng.close()
