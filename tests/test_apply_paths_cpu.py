"""The back half of a pivot as the fused LDS loop runs it -- ``mcf_pivot_finish_t<true>`` beside an apply pass that takes its
sources from the recorded stem (``mcf_apply_source_paths``, ``mcf_apply_one_paths``) -- against the plain one
(``mcf_pivot_finish``, ``mcf_apply_source``, ``mcf_apply_one``), on the host: ``csrc/mcf_apply_paths_host.cpp`` runs whole pivots on
both and compares, at every pivot, every position of ``[lo, hi)`` and every array either side writes.  No GPU.

The last test builds that file and a stand-alone program round it with the compiler's address and undefined-behaviour checks and
runs the program on the same inputs."""

from __future__ import annotations

import ctypes
import functools
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import planted_pivots as pp
import small_loop_back_instances as bi
import small_loop_control_instances as ci
import small_loop_instances as sl

# the report of mcf_apply_paths_run_host (the enum in front of it)
(PIVOTS, SWAPS, FLIPS, POSITIONS, BAD_SOURCES, BAD_STATES, MAX_K, MULTI_PIECE, BEHIND_VIN, END_OF_BLOCK, FIRST_SIDE, SECOND_SIDE,
 EMPTY_RIGHT, TABLE_WRITTEN, STATUS, FIRST_BAD, MAX_RANGE, FIRST_K) = range(18)
MCF_OPTIMAL = 1                          # McfCtx::status (csrc/mcf_core.h)

NETGEN_SHAPES = ((64, 512), (256, 2048))
STEM_INDICES = (0, 1, 2, 63, 64, 65)     # stem index of the leaving arc: one and two strides of a 64-lane finish pass
# (insertion point, tree shape): with `other` >= 1 the new parent is a leaf, T2 goes directly behind it; with `other` = 0 the new
# parent is the join, whose block ends with T2's old place, three positions closer than the place directly behind the join
INSERTIONS = (("behind", dict(other=3, above=1)), ("end", dict(other=0, above=3)))
# leaves hung along the stem (t2 - stem - 1): none -- every piece's right segment is empty -- or five, strewn in front of and
# behind the stem's nodes
LEAVES = (0, 5)


@functools.lru_cache(maxsize=None)
def plant(stem, leaves, ins, leave):
    kw = dict(INSERTIONS)[ins]
    return pp.pivot_plant(stem=stem, t2=stem + 1 + leaves, leave=leave, direction="after" if leave == "second_side" and kw["other"] else "before",
                          seed=31, **kw)


PLANTS = [(s, lv, ins, leave) for s in STEM_INDICES for lv in LEAVES for ins, _ in INSERTIONS for leave in ("first_side", "second_side")]


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_apply_paths_host()))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.mcf_apply_paths_report_len.restype = i32
    lib.mcf_apply_paths_run_host.argtypes = [i32, i64] + [vp] * 7 + [i32, i64, i64] + [vp] * 5
    lib.mcf_apply_paths_run_host.restype = ctypes.c_int
    assert lib.mcf_apply_paths_report_len() == 18
    return lib


def _arrays(inst, basis):
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)
    out = [c(inst.tail, np.int32), c(inst.head, np.int32), c(inst.cost, np.int64), c(inst.cap, np.int64), c(inst.supply, np.int64)]
    if basis is not None:
        out += [c(basis[0], np.int8), c(basis[1], np.int8)]
    return out


def run(lib, inst, rule, basis=None, max_pivots=-1):
    arrs = _arrays(inst, basis)
    n, m = inst.n, inst.m
    rep, flow, pi = np.zeros(18, np.int64), np.zeros(m, np.int64), np.zeros(n + 1, np.int64)
    parent, depth = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.mcf_apply_paths_run_host(n, m, *[p(a) for a in arrs], *([None, None] if basis is None else []), rule, 0, max_pivots,
                                      p(rep), p(flow), p(pi), p(parent), p(depth))
    assert rc == 0, rc
    return rep, dict(flow=flow, potential=pi[:n] - pi[n], parent=parent, depth=depth)


def _clean(rep, tag):
    assert rep[BAD_SOURCES] == 0 and rep[BAD_STATES] == 0 and rep[TABLE_WRITTEN] == 0 and rep[FIRST_BAD] == -1, tag + (rep.tolist(),)


@pytest.mark.parametrize("rule", (0, 1))
@pytest.mark.parametrize("n, m", NETGEN_SHAPES)
def test_every_pivot_of_the_emulated_solves(host, n, m, rule):
    """Both sides make the emulation's pivots -- its counters and its final state -- and agree at every one of them."""
    inst = sl.netgen(n, m)
    em = ci.emul(inst, rule)
    rep, out = run(host, inst, rule)
    tag = (inst.name, rule)
    _clean(rep, tag)
    assert rep[STATUS] == MCF_OPTIMAL and em["status"] == "optimal", tag
    assert rep[PIVOTS] == em["pivots"] and rep[FLIPS] == em["bound_flips"] and rep[SWAPS] + rep[FLIPS] == rep[PIVOTS], tag
    assert rep[POSITIONS] == em["nodes_moved"], tag          # every position of every [lo, hi) was compared
    assert np.array_equal(out["flow"], em["flow"]) and np.array_equal(out["potential"], em["potential"]), tag
    assert np.array_equal(out["parent"], em["parent"]) and np.array_equal(out["depth"], em["depth"]), tag
    # what these solves cover by themselves: pieces beyond the first, both insertion points, both sides, empty right segments
    assert rep[MULTI_PIECE] > 0 and rep[MAX_K] >= 2 and rep[BEHIND_VIN] > 0 and rep[END_OF_BLOCK] > 0, tag
    assert rep[FIRST_SIDE] > 0 and rep[SECOND_SIDE] > 0 and rep[EMPTY_RIGHT] > 0, tag


@pytest.mark.parametrize("stem, leaves, ins, leave", PLANTS)
def test_planted_pivots(host, stem, leaves, ins, leave):
    p = plant(stem, leaves, ins, leave)
    ref = pp.RefSimplex(p)
    assert ref.step() and not ref.flip and ref.leaving == p.leaving and ref.t2 == p.t2
    rep, out = run(host, p.inst, 0, (p.pl.in_tree, p.pl.at_upper), 1)
    tag = (stem, leaves, ins, leave)
    _clean(rep, tag)
    assert rep[PIVOTS] == 1 and rep[SWAPS] == 1 and rep[FIRST_K] == stem == rep[MAX_K], tag
    assert rep[BEHIND_VIN if ins == "behind" else END_OF_BLOCK] == 1, tag
    assert rep[FIRST_SIDE if leave == "first_side" else SECOND_SIDE] == 1, tag
    if leaves == 0:
        assert rep[EMPTY_RIGHT] == stem, tag                 # every piece behind the first
    elif stem >= 2:
        assert 0 < rep[EMPTY_RIGHT] < stem, tag              # some pieces with a right segment, some without
    n = p.inst.n
    assert np.array_equal(out["flow"], ref.flow), tag
    assert np.array_equal(out["parent"][:n], ref.parent[:n]) and np.array_equal(out["depth"][:n], ref.depth[:n]), tag
    assert np.array_equal(out["potential"], ref.potential[:n] - ref.potential[n]), tag


def _write_case(path, inst, rule, basis, max_pivots):
    with open(path, "wb") as f:
        f.write(np.array([inst.n, inst.m, rule, 0, max_pivots, 0 if basis is None else 1], "<i8").tobytes())
        for a in _arrays(inst, basis):
            f.write(a.astype(a.dtype.newbyteorder("<")).tobytes())


def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    """The same code, compiled together with a program of its own with -fsanitize=address,undefined, on the same inputs."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "apply_paths_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_apply_paths_driver.cpp"), str(ge.CSRC / "mcf_apply_paths_host.cpp")], check=True, cwd=str(ge.CSRC))
    files = []
    for n, m in NETGEN_SHAPES:
        for rule in (0, 1):
            files.append(tmp_path / f"netgen_{n}_{m}_{rule}.bin")
            _write_case(files[-1], sl.netgen(n, m), rule, None, -1)
    for k, key in enumerate(PLANTS):
        p = plant(*key)
        files.append(tmp_path / f"plant_{k}.bin")
        _write_case(files[-1], p.inst, 0, (p.pl.in_tree, p.pl.at_upper), 1)
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files) and all(" rc 0 report " in ln for ln in lines)
    # the program made the pivots of the library call above: the pivot counts of the four solves
    for ln, (n, m), rule in zip(lines, [s for s in NETGEN_SHAPES for _ in (0, 1)], (0, 1, 0, 1)):
        assert int(ln.split(" report ")[1].split()[PIVOTS]) == ci.emul(sl.netgen(n, m), rule)["pivots"], ln


# ------------------------------------------------------------------ the inputs of test_gpu_small_loop_back.py

@pytest.mark.parametrize("leave", ("first_side", "second_side"))
@pytest.mark.parametrize("r", bi.MOVED_RANGES)
def test_gpu_inputs_move_the_intended_range(host, r, leave):
    p = bi.range_plant(r, leave)
    snaps, _, status, _ = bi.range_trajectory(r, leave)
    assert status == "optimal" and snaps[0]["leaving"] == p.leaving and snaps[0]["t2"] == r - 1 and snaps[0]["deep"] > 3
    rep, _ = run(host, p.inst, 0, (p.pl.in_tree, p.pl.at_upper), 1)
    _clean(rep, (r, leave))
    assert rep[MAX_RANGE] == r and rep[POSITIONS] == r and rep[FIRST_K] == 2, (r, leave, rep.tolist())


@pytest.mark.parametrize("leave", ("first_side", "second_side"))
@pytest.mark.parametrize("stem, above, other", bi.STEM_SIDES)
def test_gpu_inputs_leave_at_the_intended_stem_index(host, stem, above, other, leave):
    p = bi.stem_plant(stem, above, other, leave)
    snaps, _, status, _ = bi.stem_trajectory(stem, above, other, leave)
    assert status == "optimal" and snaps[0]["leaving"] == p.leaving and snaps[0]["deep"] > 3
    assert snaps[0]["cycle_len"] == (stem + above + 1) + other + 1 and 63 <= other <= 65 and 64 <= stem + above + 1 <= 66
    rep, _ = run(host, p.inst, 0, (p.pl.in_tree, p.pl.at_upper), 1)
    _clean(rep, (stem, leave))
    assert rep[FIRST_K] == stem, (stem, leave, rep.tolist())


def test_gpu_inputs_fit_the_fused_loop():
    for n, m in bi.NODE_SHAPES:
        assert ci.fits_lds(n, m), (n, m)
    for r in bi.MOVED_RANGES:
        p = bi.range_plant(r)
        assert ci.fits_lds(p.inst.n, p.inst.m) and p.inst.n + 1 <= 1024, r
    for s in bi.STEM_SIDES:
        p = bi.stem_plant(*s)
        assert ci.fits_lds(p.inst.n, p.inst.m) and p.inst.n + 1 <= 1024, s
