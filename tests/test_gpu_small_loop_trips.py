"""The round trips the fused LDS loop (``k_solve_small``) saves behind its search barrier: the search reads a node's record in one
access, both ratio tests load their residuals beside the per-wave counts and -- when both sides fit one stride of 64 and are narrow --
reduce as one piece of straight-line code, the swap reads the leaving node's record and position together, the apply pass reads
potential and depth together and starts its catch-up range beside its first loop.  None of it may change a pivot: the protocol of
``test_gpu_small_loop_back.py``, at both compiled widths, one launch per pivot, the whole resident state after every launch against
``RefSimplex`` snapshots (planted pivots) or the CPU emulation (stepped solves).  The inputs are those of
``small_loop_trips_instances.py``; ``test_small_loop_trips_cpu.py`` checks without a GPU that they are what they are meant to be.

* planted cycle sides (first, second) of (0, 1), (1, 0), (1, 1), (63, 64), (64, 64), (64, 65) and (65, 1) arcs under a deep join, the
  re-hung subtree on either side: an empty side, and both sides of the one-stride test, with the leaving arc alone at the least
  residual and with ties on its own and on the other side (lowest index wins on the first side, highest on the second);
* one side narrow and the other holding a residual beyond 2^32 - 1, both ways round, and one side of nothing but ``MCF_INF``;
* consecutive swaps whose moved ranges are disjoint, nested, partly overlapping and identical, and catch-up ranges beyond 192 and
  256 positions, under rules 0, 1, 2 and with 64-bit keys (the relations are those of the Dantzig sequence)."""

from __future__ import annotations

import pytest

import small_loop_instances as sl
import small_loop_trips_instances as ti
from test_gpu_small_loop_back import _engine, _planted, _stepped

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("n1, n2, ts, leave", ti.SIDE_CASES, ids=ti.SIDE_IDS)
def test_planted_sides_from_none_to_two_strides(gpu_engine_module, n1, n2, ts, leave, width):
    _planted(gpu_engine_module, ti.side_plant(n1, n2, ts, leave), ti.side_trajectory(n1, n2, ts, leave), width, ("trips_side", n1, n2, ts, leave, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("wide_side, n1, n2", ti.MIXED)
def test_planted_sides_one_narrow_one_wide(gpu_engine_module, wide_side, n1, n2, width):
    p = ti.mixed_plant(wide_side, n1, n2)
    _planted(gpu_engine_module, p, ti.trajectory(p), width, ("trips_mixed", wide_side, n1, n2, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("inf_side", ("first", "second"))
def test_planted_side_of_nothing_but_inf(gpu_engine_module, inf_side, width):
    p = ti.inf_plant(inf_side)
    _planted(gpu_engine_module, p, ti.trajectory(p), width, ("trips_inf", inf_side, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule, narrow", ((0, "1"), (1, "1"), (2, "1"), (0, "0")))
@pytest.mark.parametrize("which", ("netgen_513", "netgen_41"))
def test_consecutive_swaps_and_their_catch_up_ranges(gpu_engine_module, monkeypatch, which, rule, narrow, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", narrow)
    inst = ti.range_instance(which)
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, ti.RANGE_STEPS, (inst.name, rule, narrow, width))
        if narrow == "0":
            assert eng.stats()["small_narrow"] == 0
