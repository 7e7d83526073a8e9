"""The fused LDS loop's 32-bit reductions (``k_solve_small``): a ratio-test side whose residuals are all ``MCF_INF`` or below
2^32 - 1 is reduced on 32-bit keys, any other on 64-bit ones; the front kernel takes its arg-max in 32-bit stages; at 256 lanes a
one-sided ancestor of the search files itself in one branch for both sides.  The protocol of ``test_gpu_small_loop_back.py``: at both compiled widths, one launch per pivot,
the whole resident state after every launch against the CPU emulation, then the whole solve and growing budgets; planted pivots
against ``RefSimplex`` snapshots.  The inputs are those of ``small_loop_reduce_instances.py``; ``test_small_loop_reduce_cpu.py``
checks them, and the selection arithmetic itself, without a GPU."""

from __future__ import annotations

import pytest

import small_loop_control_instances as ci
import small_loop_instances as sl
import small_loop_reduce_instances as ri
from test_gpu_small_loop_back import _engine, _planted, _same, _stepped

pytestmark = pytest.mark.gpu


def _whole_and_growing(e, inst, rule, tag):
    """One launch for the whole solve, and launches of 1, 2, 3, ... pivots."""
    em = ci.emul(inst, rule)
    with _engine(e, inst, rule) as eng:
        eng.solve()
        assert eng.stats()["pricing_mode"] == 2
        _same(eng.result(), eng.tree(), em, tag + ("whole",))
    with _engine(e, inst, rule) as eng:
        total = 0
        for k in range(1, 10 ** 4):
            eng.solve(k)
            total += k
            res = eng.result()
            _same(res, eng.tree(), ci.emul(inst, rule, total), tag + (total,), "optimal" if total == em["pivots"] else None)
            if res.status != "iteration_limit":
                break
        assert res.status == "optimal", tag


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("qmax, tie_rich", ri.WIDE_PARAMS, ids=ri.WIDE_IDS)
def test_stepped_pivots_on_both_sides_of_the_32_bit_limit(gpu_engine_module, monkeypatch, qmax, tie_rich, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = ri.wide(qmax, tie_rich)
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, ri.STEPS, (inst.name, rule, width))
        if rule == 0:
            assert eng.stats()["small_narrow"] == 1          # (costs up to 1 000: the front kernel)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("qmax, tie_rich", ri.WIDE_PARAMS, ids=ri.WIDE_IDS)
def test_stepped_pivots_with_64_bit_keys(gpu_engine_module, monkeypatch, qmax, tie_rich, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", "0")
    inst = ri.wide(qmax, tie_rich)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, ri.STEPS, (inst.name, "narrow=0", width))
        assert eng.stats()["small_narrow"] == 0


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("which", ("wide_2_33_ties", "wide_2_32_m1", "open_ring"))
def test_whole_solve_and_growing_budgets_across_the_limit(gpu_engine_module, monkeypatch, which, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = {"wide_2_33_ties": lambda: ri.wide(1 << 33, True), "wide_2_32_m1": lambda: ri.wide((1 << 32) - 1, False), "open_ring": ri.open_ring}[which]()
    _whole_and_growing(gpu_engine_module, inst, rule, (inst.name, rule, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("n, m", ri.NODE_SHAPES)
def test_stepped_pivots_on_the_node_shapes(gpu_engine_module, monkeypatch, n, m, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(n, m)
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, ri.STEPS, (inst.name, rule, width))
        eng.solve()
        _same(eng.result(), eng.tree(), ci.emul(inst, rule), (inst.name, rule, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule, narrow", ((0, "1"), (1, "1"), (2, "1"), (0, "0")))   # (MCF_SMALL_NARROW only changes Dantzig's front)
def test_bound_flips_and_shared_violations(gpu_engine_module, monkeypatch, rule, narrow, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", narrow)
    inst = ci.capped_transport()
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, ri.STEPS, (inst.name, rule, narrow, width))
        eng.solve()
        _same(eng.result(), eng.tree(), ci.emul(inst, rule), (inst.name, rule, narrow, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("n1, n2, ts", ri.SIDE_PARAMS, ids=ri.SIDE_IDS)
def test_planted_sides_of_one_and_two_strides(gpu_engine_module, n1, n2, ts, width):
    _planted(gpu_engine_module, ri.side_plant(n1, n2, ts), ri.side_trajectory(n1, n2, ts), width, ("side", n1, n2, ts, width))
