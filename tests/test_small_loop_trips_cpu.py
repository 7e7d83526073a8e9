"""The inputs of ``test_gpu_small_loop_trips.py`` (``small_loop_trips_instances.py``), vetted without a GPU: every planted pivot is the
one intended and reaches the node-parallel search; the mixed plants show the ratio tests one narrow side and one wide one; the
range traces hold consecutive swaps of every relation and catch-up ranges beyond 192 and 256 positions."""

from __future__ import annotations

import pytest

import planted_pivots as pp
import small_loop_control_instances as ci
import small_loop_trips_instances as ti


@pytest.mark.parametrize("n1, n2, ts, leave", ti.SIDE_CASES, ids=ti.SIDE_IDS)
def test_planted_sides(n1, n2, ts, leave):
    p = ti.side_plant(n1, n2, ts, leave)
    snaps, _, status, _ = ti.side_trajectory(n1, n2, ts, leave)
    first = ti.first_pivot(p)
    assert status == "optimal" and snaps[0]["leaving"] == p.leaving and not snaps[0]["flip"]
    assert (len(first["res1"]), len(first["res2"])) == (n1, n2) and first["deep"] > 3 and p.deep > 3       # searched, not climbed
    assert ci.fits_lds(p.inst.n, p.inst.m) and p.inst.n + 1 <= 1024
    theta = p.theta
    if "first" in ts:
        assert first["res1"].count(theta) >= (2 if leave == "first_side" else 1)
    if "second" in ts:
        assert first["res2"].count(theta) >= (2 if leave == "second_side" else 1)


def test_every_named_pair_of_sides_is_planted():
    assert {(a, b) for a, b, _, _ in ti.SIDE_CASES} == set(ti.SIDES)


@pytest.mark.parametrize("wide_side, n1, n2", ti.MIXED)
def test_mixed_plants_have_one_wide_and_one_narrow_side(wide_side, n1, n2):
    p = ti.mixed_plant(wide_side, n1, n2)
    first = ti.first_pivot(p)
    wide, narrow = (first["res1"], first["res2"]) if wide_side == "first" else (first["res2"], first["res1"])
    assert (len(first["res1"]), len(first["res2"])) == (n1, n2) and first["deep"] > 3
    assert any(ti.NARROW_LIMIT <= r < ti.MCF_INF for r in wide)
    assert all(0 <= r < ti.NARROW_LIMIT or r == ti.MCF_INF for r in narrow) and min(narrow) == p.theta
    ref = pp.RefSimplex(p)
    assert ref.step() and ref.leaving == p.leaving and not ref.flip
    assert ti.trajectory(p)[2] == "optimal"


@pytest.mark.parametrize("inf_side", ("first", "second"))
def test_inf_plants_have_a_side_of_nothing_but_inf(inf_side):
    p = ti.inf_plant(inf_side)
    first = ti.first_pivot(p)
    side = first["res1"] if inf_side == "first" else first["res2"]
    assert len(side) == 3 and all(r == ti.MCF_INF for r in side) and first["deep"] > 3
    ref = pp.RefSimplex(p)
    assert ref.step() and ref.leaving == p.leaving
    assert ti.trajectory(p)[2] == "optimal"


def test_range_traces_hold_every_relation_and_long_catch_up_ranges():
    big = ti.range_trace("netgen_513")
    small = ti.range_trace("netgen_41")
    kinds = {r[3] for r in big} | {r[3] for r in small}
    assert kinds == set(ti.RANGE_KINDS), kinds
    assert any(r[3] == "identical" for r in small)
    # the catch-up range is the swap before's: beyond 192 positions the finishing wave takes part in it, beyond 256 the
    # workgroup makes a second trip
    longest = lambda rows: max(prev[1] - prev[0] for _, prev, _, _ in rows)
    assert any(192 < prev[1] - prev[0] <= 256 for _, prev, _, _ in big) and longest(big) > 256
    # ... and, beyond 256, with positions outside the next swap's range on the second trip
    assert any(any(j < cur[0] or j >= cur[1] for j in range(prev[0] + 256, prev[1])) for _, prev, cur, _ in big)
    for which in ("netgen_513", "netgen_41"):
        inst = ti.range_instance(which)
        assert ci.fits_lds(inst.n, inst.m)
        assert ci.emul(inst, 0, ti.RANGE_STEPS)["status"] == "iteration_limit"      # (all RANGE_STEPS launches pivot)
