"""The back half of a pivot in the fused LDS loop (``k_solve_small``): the LAST wave finishes (flows, states, sizes, the re-hung
stem) while the others already apply, from the recorded stem and not from a segment table; the node-parallel search passes over
the real nodes only and looks for no join.  At both compiled widths, one launch per pivot, the whole resident state after every
launch against the CPU emulation, or against ``RefSimplex`` snapshots for planted pivots.  The inputs are those of
``small_loop_back_instances.py``; ``test_apply_paths_cpu.py`` checks them, and the functions themselves, without a GPU."""

from __future__ import annotations

import numpy as np
import pytest

import planted_pivots as pp
import small_loop_back_instances as bi
import small_loop_control_instances as ci
import small_loop_instances as sl
from test_gpu_planted_pivots import STAT_KEYS, _compare

pytestmark = pytest.mark.gpu


def _engine(e, inst, rule, **kw):
    return e.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _same(res, tree, em, tag, status=None):
    """The whole state a launch leaves behind against the emulation stopped at the same budget.  `status`: see
    test_gpu_small_loop_control.py -- at a budget of exactly the solve's pivots the kernel's own check reports optimal."""
    assert res.status == (status or em["status"]), tag + (res.status, em["status"])
    got, want = {k: res.stats[k] for k in ci.STATS}, {k: em[k] for k in ci.STATS}
    assert got == want, tag + (got, want)
    assert np.array_equal(res.flow, em["flow"]) and np.array_equal(res.potential, em["potential"]), tag
    assert np.array_equal(tree["order"], em["order"]) and np.array_equal(tree["parent"], em["parent"]), tag


def _stepped(eng, inst, rule, steps, tag):
    """solve(1) `steps` times (or to the end), everything compared after every launch."""
    assert eng.stats()["pricing_mode"] == 2, tag
    P = ci.emul(inst, rule)["pivots"]
    for total in range(1, steps + 1):
        eng.solve(1)
        res = eng.result()
        _same(res, eng.tree(), ci.emul(inst, rule, total), tag + (total,), "optimal" if total == P else None)
        if res.status != "iteration_limit":
            break
    return res


def _planted(e, p, traj, width, cid, moved=None, stem_k=None):
    """The planted protocol of test_gpu_planted_pivots.py: set_basis, solve(1) K times next to RefSimplex.step(), solve()."""
    pl, inst = p.pl, p.inst
    n = inst.n
    snaps, objective, status, total = traj
    bigm = pp.big_m(inst)
    with pytest.MonkeyPatch.context() as mp:         # (mcf_create reads the environment)
        mp.setenv("MCF_SMALL_THREADS", str(width))
        with _engine(e, inst, 0, fused=True) as eng:
            assert eng.set_basis(pl.in_tree, pl.at_upper) is True, eng.last_error()
            st = eng.result().stats
            assert st["pricing_mode"] == 2
            prev = {k: st[k] for k in STAT_KEYS + ("nodes_moved",)}
            for j, s in enumerate(snaps, 1):
                eng.solve(1)
                res, tree = eng.result(), eng.tree()
                _compare(cid, j, eng, inst, s, res, tree, bigm)
                st = res.stats
                delta = {k: st[k] - prev[k] for k in prev}
                prev = {k: st[k] for k in prev}
                want = dict(pivots=1, degenerate=int(s["degenerate"]), bound_flips=int(s["flip"]), cycle_arcs=s["cycle_len"], subtree_nodes=s["t2"],
                            cycle_scans=0)
                assert {k: delta[k] for k in want} == want, (cid, j, delta)
                if j == 1:
                    assert s["deep"] > 3 and s["leaving"] == p.leaving, "the planted pivot, by the parallel search"
                    if moved is not None:
                        assert delta["nodes_moved"] == moved, (cid, delta)
                    if stem_k is not None:
                        assert p.stem == stem_k
            eng.solve()
            res = eng.result()
            assert res.status == status and res.objective == objective and res.stats["pivots"] == total, cid
            cert = eng.certify()
            assert cert["verdict"] == status and cert["proves_status"]


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("leave", ("first_side", "second_side"))
@pytest.mark.parametrize("r", bi.MOVED_RANGES)
def test_moved_range_around_the_finishing_wave(gpu_engine_module, r, leave, width):
    _planted(gpu_engine_module, bi.range_plant(r, leave), bi.range_trajectory(r, leave), width, ("range", r, leave, width), moved=r)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("leave", ("first_side", "second_side"))
@pytest.mark.parametrize("stem, above, other", bi.STEM_SIDES)
def test_stem_index_across_the_finishing_waves_strides(gpu_engine_module, stem, above, other, leave, width):
    _planted(gpu_engine_module, bi.stem_plant(stem, above, other, leave), bi.stem_trajectory(stem, above, other, leave), width,
             ("stem", stem, above, other, leave, width), stem_k=stem)


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("n, m", bi.NODE_SHAPES)
def test_stepped_pivots_around_a_pass_of_the_search(gpu_engine_module, monkeypatch, n, m, rule, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(n, m)
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, bi.STEPS, (inst.name, rule, width))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("n, m", bi.NODE_SHAPES)
def test_stepped_pivots_with_64_bit_keys(gpu_engine_module, monkeypatch, n, m, width):
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    monkeypatch.setenv("MCF_SMALL_NARROW", "0")
    inst = sl.netgen(n, m)
    with _engine(gpu_engine_module, inst, 0) as eng:
        _stepped(eng, inst, 0, bi.STEPS, (inst.name, "narrow=0", width))
        assert eng.stats()["small_narrow"] == 0


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_bound_flips_between_swaps(gpu_engine_module, monkeypatch, rule, width):
    """A bound flip is a finish pass without an apply pass: stepped through the first pivots, then to the end."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = ci.capped_transport()
    em = ci.emul(inst, rule)
    assert 0 < em["bound_flips"] < em["pivots"]
    with _engine(gpu_engine_module, inst, rule) as eng:
        _stepped(eng, inst, rule, bi.STEPS, (inst.name, rule, width))
        eng.solve()
        _same(eng.result(), eng.tree(), em, (inst.name, rule, width, "whole"))


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("which", ("netgen_257", "capped_transport"))
def test_whole_solve_and_growing_budgets(gpu_engine_module, monkeypatch, which, rule, width):
    """The image a launch leaves behind: one launch for the whole solve, and launches of 1, 2, 3, ... pivots."""
    monkeypatch.setenv("MCF_SMALL_THREADS", str(width))
    inst = sl.netgen(257, 1028) if which == "netgen_257" else ci.capped_transport()
    em = ci.emul(inst, rule)
    tag = (inst.name, rule, width)
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
