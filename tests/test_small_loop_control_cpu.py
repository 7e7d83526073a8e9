"""The inputs of ``test_gpu_small_loop_control.py``, checked without a GPU: through the CPU emulation each of them has the
property its GPU test relies on."""

from __future__ import annotations

import numpy as np
import pytest

import oracle
import small_loop_control_instances as ci
import small_loop_instances as sl


@pytest.mark.parametrize("n, m", ci.CHOP_SHAPES)
def test_chopped_shapes_are_solved_under_every_rule_and_fit(n, m):
    inst = sl.netgen(n, m)
    assert ci.fits_lds(inst.n, inst.m)
    for rule in (0, 1, 2):
        em = ci.emul(inst, rule)
        assert em["status"] == "optimal" and em["pivots"] > 7 * 7


def test_cold_start_goes_from_the_climb_to_the_parallel_search():
    """End points no deeper than 3 are climbed by two lanes; the first pivots of a cold start are such, later ones are not:
    a cycle of more than 7 arcs has an end point deeper than 3 (n1 <= depth[first], n2 <= depth[second])."""
    inst = sl.netgen(257, 1028)
    for rule in (0, 1, 2):
        assert int(ci.emul(inst, rule, 5)["depth"].max()) <= 3, "the first five pivots see no node deeper than 3"
        total = ci.emul(inst, rule)["pivots"]
        prev, long_cycles = 0, 0
        for c in range(1, total + 1):
            cyc = ci.emul(inst, rule, c)["cycle_arcs"]
            long_cycles += cyc - prev > 7
            prev = cyc
        assert long_cycles > 0, "a later pivot goes through the parallel search"


def test_devex_block_meets_blocks_without_a_candidate_on_the_way():
    inst = sl.netgen(64, 512)
    st = oracle.EmulStepper(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=1, block_size=ci.DEVEX_BLOCK)
    try:
        out = np.zeros(2, np.int64)
        empties = trailing = passes = 0
        while True:
            st.price(0, 1, out)
            passes += 1
            empty = out[1] < 0
            empties += empty
            trailing = trailing + 1 if empty else 0
            st.pivot(out, 1)
            status, pivots, _, _ = st.poll()
            if status is not None:
                break
            assert passes < 100000
    finally:
        st.close()
    assert oracle.STATUS_NAMES[status] == "optimal" and pivots == ci.emul(inst, 1, -1, ci.DEVEX_BLOCK)["pivots"]
    assert empties - trailing > 0, "blocks without a candidate before the final round over every block"


def test_candidate_list_runs_dry_before_its_minor_cap():
    inst = sl.netgen(257, 1028)
    st = oracle.EmulStepper(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=2)
    try:
        _, minor_cap = st.set_shards(1)
    finally:
        st.close()
    em = ci.emul(inst, 2)
    assert em["major_sweeps"] > 1 and minor_cap > 0
    assert em["minor_pivots"] < minor_cap * em["major_sweeps"], "some minor iteration found its list exhausted"


def test_start_basis_is_optimal():
    inst = ci.optimal_at_start()
    for rule in (0, 1, 2):
        em = ci.emul(inst, rule)
        assert em["status"] == "optimal" and em["pivots"] == 0 and em["objective"] == 0


def test_verdict_instances_fit_and_have_their_verdicts():
    for name, (inst, verdict) in ci.verdict_cases().items():
        assert ci.fits_lds(inst.n, inst.m), name
        for rule in (0, 1, 2):
            assert ci.emul(inst, rule)["status"] == verdict, (name, rule)


def test_capped_transport_flips_bounds_and_degenerates():
    inst = ci.capped_transport()
    assert ci.fits_lds(inst.n, inst.m) and int(inst.cap.min()) == 1 and int(inst.cap.max()) == 3
    for rule in (0, 1, 2):
        em = ci.emul(inst, rule)
        assert em["status"] == "optimal" and em["bound_flips"] > 0 and em["degenerate"] > 0


def test_largest_tree_of_the_lds_plan():
    """The plan's estimate alone -- 112 B per tree node under 150 KiB -- keeps every tree below 1 024 nodes: no instance
    on the fused path is above kSmallCycleMaxNodes, so none is climbed for its size."""
    inst = ci.largest_tree()
    assert ci.fits_lds(inst.n, inst.m) and not ci.fits_lds(inst.n + 1, inst.m + 1 + (inst.n + 1) // 8 - inst.n // 8)
    assert 700 < inst.n + 1 <= 1024
    assert not any(ci.fits_lds(n, n) for n in range(1024, 1400))
    for rule in (0, 1, 2):
        assert ci.emul(inst, rule)["status"] == "optimal"
