"""The front kernel of the fused LDS loop (``k_solve_small``) budgeted in issue slots: a register sweep that computes the violation
without a compare and keeps two accumulators per lane, and a pick that reads the waves' slots whole and unpacks with selects.  None of
it may change a pivot: the protocol of ``test_gpu_small_loop_back.py`` -- one launch per pivot, the whole resident state after every
launch against the CPU emulation -- on the inputs of ``small_loop_slots_instances.py`` (``test_small_loop_slots_cpu.py`` checks
without a GPU that they are what they are meant to be).  The changed code is compiled for 256 lanes only; the 1 024-lane kernels run
the same inputs through the forms they kept.

* arc counts at which the sweep can go wrong: 1, 255 .. 257, 2 047 .. 2 049 (the 8-slot sweep hands over to the 10-slot one) and
  2 561 (the first arc priced from LDS);
* first pivots whose two largest violations tie: in two slots of one accumulator, in the two accumulators of a lane, in two lanes of
  a wave, in waves 0 / 3 and 1 / 2, the ids either way round; the only eligible arc in wave 3's last slot; no eligible arc at all;
* both states with either sign of the reduced cost in the sweeps, and the instance at the narrow limit of the reduced costs;
* the seven counters a launch carries in registers (``arcs_priced`` is added directly behind the pick) across resumed launches of 1,
  2 and 7 pivots: ``stats()`` after every launch against the emulation stopped at the same budget, over runs that hold bound flips,
  degenerate pivots and an unbounded verdict."""

from __future__ import annotations

import pytest

import small_loop_control_instances as ci
import small_loop_decide_instances as di
import small_loop_instances as sl
import small_loop_slots_instances as si
from test_gpu_small_loop_back import _engine, _same, _stepped

pytestmark = pytest.mark.gpu


def _front(eng):
    st = eng.stats()
    assert st["pricing_mode"] == 2 and st["small_narrow"] == 1, "the fused loop's front kernel (of either width)"


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("m", si.ARC_COUNTS)
def test_arc_counts_round_the_lanes_the_slots_and_the_lds_loop(gpu_engine_module, monkeypatch, m, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.arc_count(m)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, si.COUNT_STEPS, (inst.name, width))
        _front(eng)
    with _engine(gpu_engine_module, inst, 0) as eng:      # (a handle of its own: a stepped one that met its budget at the optimum priced one sweep less)
        eng.solve()
        _same(eng.result(), eng.tree(), ci.emul(inst, 0), (inst.name, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("kind", sorted(si.TIES))
def test_first_pivot_with_the_largest_violation_tied(gpu_engine_module, monkeypatch, kind, order, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.tie(kind, order)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, si.TIE_STEPS, (inst.name, width))
        _front(eng)


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_only_eligible_arc_in_the_last_slot_of_wave_3(gpu_engine_module, monkeypatch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.last_slot()
    with _engine(gpu_engine_module, inst, 0) as eng:
        res = _stepped(eng, inst, 0, si.TIE_STEPS, (inst.name, width))
        _front(eng)
        assert res.stats["pivots"] >= 1


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_no_eligible_arc_at_the_first_sweep(gpu_engine_module, monkeypatch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.nothing()
    with _engine(gpu_engine_module, inst, 0) as eng:
        eng.solve(1)
        res = eng.result()
        _front(eng)
        _same(res, eng.tree(), ci.emul(inst, 0), (inst.name, width))
        assert res.status == "optimal" and res.stats["pivots"] == 0


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_both_states_with_either_sign_of_the_reduced_cost(gpu_engine_module, monkeypatch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.states()
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, si.STATES_STEPS, (inst.name, width))
        _front(eng)
    with _engine(gpu_engine_module, inst, 0) as eng:
        eng.solve()
        _same(eng.result(), eng.tree(), ci.emul(inst, 0), (inst.name, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_reduced_costs_at_the_narrow_limit(gpu_engine_module, monkeypatch, width):
    """The instance whose reduced-cost BOUND is 2^31 - 1 (one more unit of cost and the host's range check sends it to the 64-bit
    kernel).  It does not plant a violation of exactly that size: none is reachable inside the range check; the value itself goes
    through the sweep's arithmetic in ``test_small_loop_slots_cpu.py``."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.limit()
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, si.LIMIT_STEPS, (inst.name, width))
        _front(eng)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("cap", si.COUNTER_CAPS)
@pytest.mark.parametrize("which", sorted(si.COUNTER_RUNS))
def test_counters_across_resumed_launches(gpu_engine_module, monkeypatch, which, cap, width):
    """solve(cap) until the solve ends; after EVERY launch all seven counters and the status of the emulation with the same total
    budget (at a budget of exactly an optimal solve's pivots the kernel's own check already reports optimal)."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.counter_run(which)
    whole = ci.emul(inst, 0)
    want_end, flips, degenerate = si.COUNTER_RUNS[which]
    assert whole["status"] == want_end and (whole["bound_flips"] > 0) == flips and (whole["degenerate"] > 0) == degenerate
    with _engine(gpu_engine_module, inst, 0, fused=True) as eng:
        total, seen = 0, dict(bound_flips=0, degenerate=0)
        while True:
            eng.solve(cap)
            total += cap
            res, em = eng.result(), ci.emul(inst, 0, total)
            tag = (inst.name, cap, width, total)
            want = "optimal" if want_end == "optimal" and total == whole["pivots"] else em["status"]
            assert res.status == want, tag + (res.status, want)
            got = {k: res.stats[k] for k in ci.STATS}
            assert got == {k: em[k] for k in ci.STATS}, tag + (got, {k: em[k] for k in ci.STATS})
            seen = {k: got[k] for k in seen}
            if res.status != "iteration_limit":
                break
            assert total <= whole["pivots"] + cap, tag
        _front(eng)
        assert res.status == want_end and res.stats["pivots"] == whole["pivots"]
        assert (seen["bound_flips"] > 0) == flips and (seen["degenerate"] > 0) == degenerate, "what the run was chosen for did occur"
        if want_end == "unbounded":
            assert res.stats["unbounded_arc"] == whole["unbounded_arc"]
