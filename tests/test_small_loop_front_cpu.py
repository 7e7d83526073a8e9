"""The range predicate of the fused LDS loop's 32-bit pricing keys (``mcf_small_narrow_ok``, csrc/mcf_host.h) at its edge, the
bound it rests on checked pivot by pivot through the CPU emulation, and the inputs of ``test_gpu_small_loop_front.py``."""

from __future__ import annotations

import numpy as np
import pytest

import small_loop_control_instances as ci
import small_loop_front_instances as fi
import small_loop_instances as sl
from network_flow_solver_amd import engine


def _ok(n, c):
    return engine.small_narrow_ok(fi.big_m(n, c), c)


def test_predicate_at_its_edge():
    c = fi.edge_cost(64)
    assert c == (2 ** 31 - 264) // 259
    ok, bound = _ok(64, c)
    assert ok and bound == fi.rc_bound(fi.big_m(64, c), c) <= fi.INT32_MAX
    ok1, bound1 = _ok(64, c + 1)
    assert not ok1 and bound1 == fi.rc_bound(fi.big_m(64, c + 1), c + 1) > fi.INT32_MAX
    # the predicate sees magnitudes: an instance whose largest |cost| is negative is the same instance to it
    for inst, want in ((fi.edge(0), True), (fi.edge(1), False)):
        cm = int(np.abs(inst.cost).max())
        assert int(inst.cost.min()) < 0 and _ok(inst.n, cm)[0] is want
    # every node count of the LDS plan has an edge of its own, and it is where the closed form says
    for n in (1, 2, 63, 64, 65, 256, 257, 1023, 1370):
        c = fi.edge_cost(n)
        assert _ok(n, c)[0] and not _ok(n, c + 1)[0], n
    # a big-M that stayed up after the costs came down (mcf_update_costs never shrinks it) decides, not the costs
    assert not engine.small_narrow_ok(fi.big_m(64, fi.edge_cost(64) + 1), 10)[0]
    assert not engine.small_narrow_ok(0, 0)[0] and not engine.small_narrow_ok(1 << 44, 0)[0]


def test_bound_is_above_the_derivation():
    """R = 2 B + (2 n - 1) C (csrc/mcf_host.h) stays below the bound the predicate tests, for B >= (C + 1)(n + 2)."""
    for n in (1, 2, 64, 256, 1370):
        for c in (0, 1, 100, 10 ** 4, fi.edge_cost(n)):
            for slack in (0, 1, 12345):
                b = fi.big_m(n, c) + slack
                assert 2 * b + (2 * n - 1) * c <= fi.rc_bound(b, c), (n, c, slack)


@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("name", ("netgen_64_512", "netgen_256_2048", "edge_0", "edge_1", "unit_grid", "bucket_385"))
def test_reduced_costs_stay_within_the_bound_at_every_pivot(name, rule):
    inst = {"netgen_64_512": lambda: sl.netgen(64, 512), "netgen_256_2048": lambda: sl.netgen(256, 2048), "edge_0": lambda: fi.edge(0),
            "edge_1": lambda: fi.edge(1), "unit_grid": fi.unit_grid, "bucket_385": lambda: sl.bucket_at(385)}[name]()
    c = int(np.abs(inst.cost).max())
    bm = fi.big_m(inst.n, c)
    bound = fi.rc_bound(bm, c)
    total = ci.emul(inst, rule)["pivots"]
    # every pivot of the small instances; the larger ones thin out after the first 64 (an emulation run per point)
    points = range(total + 1) if total <= 400 else sorted(set(range(64)) | set(range(64, total + 1, 8)) | {total})
    worst = 0
    for p in points:
        w, wpi = fi.emul_bounds(inst, rule, p)
        assert wpi <= bm + (inst.n - 1) * c, (name, rule, p)
        worst = max(worst, w)
    assert worst <= 2 * bm + (2 * inst.n - 1) * c <= bound, (name, rule, worst, bound)


def test_edge_instances_are_solved_and_sit_on_either_side():
    for above, want in ((0, True), (1, False)):
        inst = fi.edge(above)
        assert ci.fits_lds(inst.n, inst.m)
        assert _ok(inst.n, int(np.abs(inst.cost).max()))[0] is want
        for rule in (0, 1, 2):
            em = ci.emul(inst, rule)
            assert em["status"] == "optimal" and em["pivots"] > fi.STEPS
    # at the edge the violations really leave 30 bits: the 32-bit path is exercised near its limit
    assert fi.emul_bounds(fi.edge(0), 0, 0)[0] > 2 ** 30


def test_unit_grid_ties_everywhere():
    inst = fi.unit_grid()
    assert ci.fits_lds(inst.n, inst.m) and set(inst.cost.tolist()) == {1}
    for rule in (0, 1, 2):
        em = ci.emul(inst, rule)
        assert em["status"] == "optimal" and em["pivots"] >= 8
    # at the start basis every arc into a demand node has the same violation, 2 big-M - 1: eight equal keys in one head bucket
    pi = ci.emul(inst, 0, 0)["potential"]
    viol = -(inst.cost + pi[inst.tail] - pi[inst.head])
    top = viol.max()
    assert top > 0 and int((viol == top).sum()) >= 8


def test_first_bucket_is_fuller_than_the_register_slots():
    for inst in (sl.bucket_at(385), sl.transport(1024)):
        assert int((inst.head < 32).sum()) > 320 and ci.fits_lds(inst.n, inst.m)
        assert engine.small_narrow_ok(fi.big_m(inst.n, int(np.abs(inst.cost).max())), int(np.abs(inst.cost).max()))[0]


def test_update_costs_edge_arc():
    """The cost the resident-handle test raises: one arc of netgen(64, 512) to edge_cost + 1 takes big-M across the edge."""
    inst = sl.netgen(64, 512)
    c0 = int(np.abs(inst.cost).max())
    assert _ok(inst.n, c0)[0] and not _ok(inst.n, fi.edge_cost(inst.n) + 1)[0]
