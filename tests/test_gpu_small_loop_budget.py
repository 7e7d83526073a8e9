"""The second part of the slot budget of the fused LDS loop (``k_solve_small``): side- and buffer-selected addresses by arithmetic,
ballots straight from their compares, a wave's two counts in one word, the finish pass's loads in one trip.  The protocol of
``test_gpu_small_loop_back.py``: one launch per pivot, the whole resident state and ``stats()`` after every launch against the CPU
emulation, exact, at both compiled widths.  The inputs are those of ``small_loop_budget_instances.py``;
``test_small_loop_budget_cpu.py`` checks them, and the functions themselves, without a GPU."""

from __future__ import annotations

import pytest

import small_loop_budget_instances as bu
import small_loop_control_instances as ci
import small_loop_instances as sl
import small_loop_reduce_instances as ri
import small_loop_slots_instances as si
from test_gpu_small_loop_back import _engine, _planted, _same, _stepped

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("which", ("tiny", "netgen_64", "netgen_256", "limit", "limit_first", "open_ring"))
def test_stepped_pivots_on_trees_of_3_65_257_nodes_and_at_the_narrow_limit(gpu_engine_module, monkeypatch, which, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = {"tiny": bu.tiny, "netgen_64": lambda: bu.netgen(64, 512), "netgen_256": lambda: bu.netgen(256, 1024), "limit": bu.limit, "limit_first": bu.limit_first,
            "open_ring": ri.open_ring}[which]()   # (open_ring: sides of nothing but MCF_INF)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, bu.STEPS, (inst.name, width))
        assert eng.stats()["small_narrow"] == 1
    with _engine(gpu_engine_module, inst, 0) as eng:   # (a fresh handle: a solve resumed at its last pivot skips the last sweep)
        eng.solve()
        _same(eng.result(), eng.tree(), ci.emul(inst, 0), (inst.name, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("which", ("netgen_256", "limit", "capped_transport"))
def test_two_pivots_a_launch_swap_behind_swap_and_flip_behind_swap(gpu_engine_module, monkeypatch, which, width):
    """Consecutive swaps inside one launch alternate the buffers; the capped instances put flips directly behind swaps."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = {"netgen_256": lambda: bu.netgen(256, 1024), "limit": bu.limit, "capped_transport": ci.capped_transport}[which]()
    em = ci.emul(inst, 0)
    with _engine(gpu_engine_module, inst, 0) as eng:
        total = 0
        for _ in range(bu.STEPS // 2):
            eng.solve(2)
            total += 2
            res = eng.result()
            _same(res, eng.tree(), ci.emul(inst, 0, total), (inst.name, width, total), "optimal" if total == em["pivots"] else None)
            if res.status != "iteration_limit":
                break


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("n1, n2", bu.SIDES)
def test_planted_sides_round_one_stride(gpu_engine_module, n1, n2, width):
    ts = ("first", "second")
    _planted(gpu_engine_module, ri.side_plant(n1, n2, ts), ri.side_trajectory(n1, n2, ts), width, ("side", n1, n2, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("leave", bu.EMPTY_SIDES)
def test_planted_side_of_length_0(gpu_engine_module, leave, width):
    _planted(gpu_engine_module, bu.empty_side_plant(leave), bu.empty_side_trajectory(leave), width, ("empty", leave, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_unbounded_verdict_behind_swaps_in_one_launch(gpu_engine_module, monkeypatch, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst, _ = ci.verdict_cases()["deep_unbounded"]
    em = ci.emul(inst, 0)
    assert em["status"] == "unbounded" and em["pivots"] - em["bound_flips"] > 0, "basis swaps in front of the verdict, in the same launch"
    with _engine(gpu_engine_module, inst, 0) as eng:
        eng.solve()
        res = eng.result()
        assert res.status == "unbounded" and {k: res.stats[k] for k in ci.STATS} == {k: em[k] for k in ci.STATS}


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("kind", sorted(si.TIES))
def test_tie_instances_of_the_publish(gpu_engine_module, monkeypatch, kind, order, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = si.tie(kind, order)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, si.TIE_STEPS, (inst.name, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_long_launch_then_resumed_twice(gpu_engine_module, monkeypatch, width):
    """The seven counters a launch carries in registers, over a launch of 297 pivots and two resumed ones: ``stats()`` and the whole
    state after every launch against the emulation stopped at the same budget."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = bu.fold_instance()
    em = ci.emul(inst, 0)
    with _engine(gpu_engine_module, inst, 0) as eng:
        total = 0
        for k in bu.FOLD_BUDGETS:
            if k < 0:
                eng.solve()
                _same(eng.result(), eng.tree(), em, (inst.name, width, "end"))
            else:
                eng.solve(k)
                total += k
                _same(eng.result(), eng.tree(), ci.emul(inst, 0, total), (inst.name, width, total))
        assert eng.stats()["pricing_mode"] == 2 and eng.stats()["small_narrow"] == 1
