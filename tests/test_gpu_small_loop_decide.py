"""The decision of a pivot in the fused LDS loop (``k_solve_small``): the 256-lane front kernel decides with
``mcf_pivot_decide_flat`` -- the three exits of ``mcf_pivot_decide`` (unbounded, bound flip, swap) as selects, the leaving node's
record fetched unconditionally -- carries the pivot descriptor across the loop and stores it once behind it, and the ratio tests
of both 256-lane kernels read their counts and residuals in one trip.  At both compiled widths, one launch per pivot, the whole resident state after every launch against ``RefSimplex``
snapshots for planted pivots or against the CPU emulation; the protocol is ``test_gpu_small_loop_back.py``'s.  The inputs are those
of ``small_loop_decide_instances.py``; ``test_small_loop_decide_cpu.py`` checks them, and the function itself, without a GPU."""

from __future__ import annotations

import pytest

import planted_pivots as pp
import small_loop_control_instances as ci
import small_loop_decide_instances as di
import small_loop_instances as sl
from test_gpu_planted_pivots import _compare
from test_gpu_small_loop_back import _engine, _planted, _same, _stepped

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("name", sorted(di.PLANTS))
def test_planted_decisions(gpu_engine_module, name, width):
    """Every exit and tie of the decision and every select of the swap as the FIRST pivot of a launch, then five more."""
    _planted(gpu_engine_module, di.plant(name), di.trajectory(name), width, (name, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_bound_flip_behind_a_swap_in_one_launch(gpu_engine_module, width):
    """The swap's descriptor is in the registers when the flip is decided: the flip must leave it alone."""
    p, (snaps, _, _, _) = di.plant("flip_behind_a_swap"), di.trajectory("flip_behind_a_swap")
    assert not snaps[0]["flip"] and snaps[1]["flip"]
    with pytest.MonkeyPatch.context() as mp:         # (mcf_create reads the environment)
        mp.setenv("MCF_SMALL_THREADS", str(width))
        with _engine(gpu_engine_module, p.inst, 0, fused=True) as eng:
            assert eng.set_basis(p.pl.in_tree, p.pl.at_upper) is True, eng.last_error()
            eng.solve(2)
            res = eng.result()
            assert res.stats["pricing_mode"] == 2 and res.stats["pivots"] == 2 and res.stats["bound_flips"] == 1
            assert res.stats["subtree_nodes"] == snaps[0]["t2"]
            _compare(("flip_behind_a_swap", width), 2, eng, p.inst, snaps[1], res, eng.tree(), pp.big_m(p.inst))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("name", di.UNBOUNDED)
def test_unbounded_cycle_behind_swaps_of_the_same_launch(gpu_engine_module, monkeypatch, name, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = di.unbounded(name)
    em = ci.emul(inst, rule)
    assert em["status"] == "unbounded" and em["pivots"] - em["bound_flips"] >= 1
    with _engine(gpu_engine_module, inst, rule, fused=True) as eng:
        eng.solve()
        res = eng.result()
        tag = (name, rule, width)
        assert res.stats["pricing_mode"] == 2, tag
        assert res.stats["unbounded_arc"] == em["unbounded_arc"], tag
        _same(res, eng.tree(), em, tag)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule, narrow", ((0, 1), (0, 0), (1, 1), (2, 1)))
@pytest.mark.parametrize("n, m", di.STEPPED_SHAPES)
def test_stepped_pivots(gpu_engine_module, monkeypatch, n, m, rule, narrow, width):
    """Dantzig with 32-bit keys runs the front kernels, with 64-bit keys and under the other rules the general ones."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", str(narrow))
    inst = di.stepped(n, m)
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, di.STEPS, (inst.name, rule, narrow, width))
        if rule == 0:
            assert eng.stats()["small_narrow"] == narrow
