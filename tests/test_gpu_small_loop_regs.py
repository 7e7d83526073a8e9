"""The even deal of the Dantzig register sweep in the fused LDS loop's front kernels (``k_solve_small<THREADS, true>``): lane ``t``
prices the engine arcs ``t, t + THREADS, ...`` whatever their head bucket, in as many unrolled slots as the arc count needs, the rest
from LDS; the general kernels -- 64-bit keys, the candidate list, Devex -- keep the deal per bucket and their granules.  The protocol
of ``test_gpu_small_loop_back.py``: at both compiled widths, one launch per pivot, the whole resident state after every launch
against the CPU emulation -- under every rule and with 64-bit keys, so that every kernel prices every shape.  The map itself is
checked without a GPU (``test_small_loop_regs_cpu.py``)."""

from __future__ import annotations

import numpy as np
import pytest

import small_loop_back_instances as bi
import small_loop_control_instances as ci
import small_loop_instances as sl
import small_loop_reduce_instances as ri
from test_gpu_small_loop_back import _engine, _same, _stepped

pytestmark = pytest.mark.gpu

STEPS = bi.STEPS

# name -> instance.  Tree nodes = n + 1 (the root).
INSTANCES = {
    "tree_41": lambda: sl.netgen(40, 200),                 # fewer lanes hold an arc than a wave has: one partly filled slot
    "tree_65": lambda: sl.netgen(64, 512),                 # two slots of 256 lanes, half a slot of 1 024
    "tree_257": lambda: sl.netgen(256, 1024),              # four full slots / one
    "tree_514": lambda: sl.netgen(513, 1026),              # a partly filled fifth / second slot
    "not_a_multiple": lambda: sl.netgen(256, 1025),        # one arc in the last slot
    "flagship_shape": lambda: sl.netgen(256, 2048),        # eight slots of 256 lanes, two of 1 024: the shorter compiled sweeps, full
    "past_the_short_sweep": lambda: sl.netgen(256, 2049),  # one arc more: the longer compiled sweeps
    "lds_tail": lambda: sl.netgen(96, 3100),               # more than 10 x 256 and 3 x 1 024 arcs: the rest is priced from LDS
    "one_bucket": lambda: sl.transport(1024),              # every arc in the first head bucket: the other buckets' lanes price too
    "capped_transport": ci.capped_transport,               # bound flips, violations shared by many arcs
    "wide_ties_31": lambda: ri.wide(1 << 31, True),        # tie-rich: equal violations across lanes, the lowest id must win
    "wide_ties_33": lambda: ri.wide(1 << 33, True),
}
WHOLE = ("lds_tail", "one_bucket")


def test_inputs_fit_the_lds_plan_and_hold_the_edges():
    for name, make in INSTANCES.items():
        inst = make()
        assert ci.fits_lds(inst.n, inst.m), name
    assert INSTANCES["tree_41"]().n + 1 < 64 and INSTANCES["not_a_multiple"]().m % 256 == 1
    assert INSTANCES["lds_tail"]().m > max(10 * 256, 3 * 1024)
    one = INSTANCES["one_bucket"]()
    assert (one.head // ((one.n + 7) // 8) == 0).all()
    assert INSTANCES["flagship_shape"]().m == 8 * 256 and INSTANCES["past_the_short_sweep"]().m == 8 * 256 + 1


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_stepped_pivots_under_every_rule(gpu_engine_module, monkeypatch, name, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = INSTANCES[name]()
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, STEPS, (name, rule, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_stepped_pivots_with_64_bit_keys(gpu_engine_module, monkeypatch, name, width):
    """MCF_SMALL_NARROW=0: Dantzig in the general kernel, whose plain register sweep deals per bucket."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", "0")
    inst = INSTANCES[name]()
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, STEPS, (name, "narrow=0", width))
        assert eng.stats()["small_narrow"] == 0


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("name", WHOLE)
def test_whole_solve_and_growing_budgets(gpu_engine_module, monkeypatch, name, rule, width):
    """One launch for the whole solve, and launches of 1, 2, 3, ... pivots: arcs_priced stays the constant it was."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = INSTANCES[name]()
    em = ci.emul(inst, rule)
    tag = (name, rule, width)
    with _engine(gpu_engine_module, inst, rule) as eng:
        eng.solve()
        assert eng.stats()["pricing_mode"] == 2
        _same(eng.result(), eng.tree(), em, tag + ("whole",))
    with _engine(gpu_engine_module, inst, rule) as eng:
        total = 0
        for k in range(1, 10 ** 4):
            eng.solve(k)
            total += k
            res = eng.result()
            _same(res, eng.tree(), ci.emul(inst, rule, total), tag + (total,), "optimal" if total == em["pivots"] else None)
            if res.status != "iteration_limit":
                break
        assert res.status == "optimal", tag

