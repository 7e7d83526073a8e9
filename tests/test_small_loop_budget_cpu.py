"""The second part of the fused LDS loop's slot budget without a GPU: the pair arithmetic against the select form on the offsets
``mcf_small_plan`` gives, the packed per-wave counts, and whole host solves run twice -- as every path runs a pivot and as the
256-lane front kernel runs it (one planned buffer, ``mcf_pivot_decide_flat_t<true>``, ``mcf_pivot_finish_pairs``, the apply pass on
arithmetic addresses) -- by ``csrc/mcf_small_budget_host.cpp``.  Also vets the inputs of ``test_gpu_small_loop_budget.py``."""

from __future__ import annotations

import ctypes
import itertools
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import small_loop_budget_instances as bu
import small_loop_control_instances as ci
import small_loop_reduce_instances as ri


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_small_budget_host()))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.mcf_budget_pairs_host.argtypes = [i32, i64, i64, i32, i32, vp]
    lib.mcf_budget_counts_host.argtypes = [vp, vp, vp, vp]
    lib.mcf_budget_twin_host.argtypes = [i32, i64, vp, vp, vp, vp, vp, i64, i32, vp]
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("devex", (0, 1))
@pytest.mark.parametrize("nn", bu.TREES)
def test_pair_arithmetic_names_the_selected_arrays_element(host, nn, devex):
    out = np.zeros(7, np.int64)
    m_pad = 1024
    assert host.mcf_budget_pairs_host(nn, m_pad, m_pad - 7 + nn - 1, devex, 16, _ptr(out)) == 0
    compared, bad, unaligned, total, d4, d16, planned = out.tolist()
    assert bad == 0 and unaligned == 0, "every address the same, every record address a multiple of 16"
    assert compared >= 2 * 6 * nn and d4 == (nn + 3) // 4 * 4 and d16 == nn and d4 % 4 == 0
    assert planned == (nn < 1370), "every size but the bound itself is an instance the kernel can run"


def test_packed_counts_add_up_over_four_waves(host):
    cases = 0
    for a, b in itertools.product(bu.COUNTS, repeat=2):
        for wa, wb, split in itertools.product(range(4), range(4), (1, 2, 4)):
            n1, n2 = np.zeros(4, np.int32), np.zeros(4, np.int32)
            for q in range(split):                                   # spread over 1, 2 or 4 waves from wave wa / wb on
                n1[(wa + q) % 4] += a // split + (a % split if q == 0 else 0)
                n2[(wb + q) % 4] += b // split + (b % split if q == 0 else 0)
            s1, s2 = np.zeros(1, np.int32), np.zeros(1, np.int32)
            assert host.mcf_budget_counts_host(_ptr(n1), _ptr(n2), _ptr(s1), _ptr(s2)) == 0, (a, b, wa, wb, split)
            assert (int(s1[0]), int(s2[0])) == (a, b)
            cases += 1
    assert cases == 36 * 48
    assert host.mcf_budget_max_nodes_host() <= 1 << 16 and max(bu.COUNTS) < host.mcf_budget_max_nodes_host()


def _twin(host, inst, max_pivots=-1, finish_mode=0):
    rep = np.zeros(12, np.int64)
    cost, cap, supply = (np.ascontiguousarray(x, np.int64) for x in (inst.cost, inst.cap, inst.supply))
    tail, head = (np.ascontiguousarray(x, np.int32) for x in (inst.tail, inst.head))
    assert host.mcf_budget_twin_host(inst.n, inst.m, _ptr(tail), _ptr(head), _ptr(cost), _ptr(cap), _ptr(supply), max_pivots, finish_mode, _ptr(rep)) == 0
    return dict(zip(("pivots", "swaps", "flips", "first", "second", "cur1", "bad_ctx", "bad_arrays", "status", "first_bad", "first_cur1", "second_cur1"),
                    rep.tolist()))


@pytest.mark.parametrize("finish_mode", (0, 1, 2), ids=("one_lane", "64_lanes", "64_lanes_pass_by_pass"))
@pytest.mark.parametrize("which", ("tiny", "netgen_64", "netgen_256", "limit", "capped_transport"))
def test_whole_solves_the_kernels_way_and_everybodys(host, which, finish_mode):
    inst = {"tiny": bu.tiny, "netgen_64": lambda: bu.netgen(64, 512), "netgen_256": lambda: bu.netgen(256, 1024), "limit": bu.limit,
            "capped_transport": ci.capped_transport}[which]()
    r = _twin(host, inst, finish_mode=finish_mode)
    assert r["bad_ctx"] == 0 and r["bad_arrays"] == 0 and r["first_bad"] == -1, r
    em = ci.emul(inst, 0)
    assert r["pivots"] == em["pivots"] and r["flips"] == em["bound_flips"], (r, em["pivots"])
    if which != "tiny":
        assert r["first"] > 0 and r["second"] > 0 and 0 < r["cur1"] < r["swaps"], "either side leaves, from either buffer"
        assert 0 < r["first_cur1"] < r["first"] and 0 < r["second_cur1"] < r["second"], "each side leaves with cur 0 and with cur 1"
    if which in ("capped_transport", "tiny"):
        assert r["flips"] > 0


def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "small_budget_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_small_budget_driver.cpp"), str(ge.CSRC / "mcf_small_budget_host.cpp")], check=True, cwd=str(ge.CSRC))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert len(r.stdout.strip().splitlines()) == len(bu.TREES) + 1 + 3


# ------------------------------------------------------------------ the GPU file's inputs are what they are meant to be
def test_gpu_inputs_fit_the_plan_and_run_the_front_kernel():
    import small_loop_front_instances as fi

    for inst in (bu.tiny(), bu.netgen(64, 512), bu.netgen(256, 1024), bu.limit(), bu.limit_first()):
        assert ci.fits_lds(inst.n, inst.m)
        cmax = int(np.abs(inst.cost).max())
        assert fi.rc_bound(fi.big_m(inst.n, cmax), cmax) <= 2 ** 31 - 1, "narrow reduced costs: the front kernel runs"
    assert [i.n + 1 for i in (bu.tiny(), bu.netgen(64, 512), bu.netgen(256, 1024))] == [3, 65, 257]


def test_gpu_inputs_limit_meets_both_sides_of_the_narrow_limit():
    log = [r for r in bu.limit_log() if r["deep"] > 3]
    assert len(bu.limit_log()) == bu.STEPS and len(log) >= 30
    seen = {(side, v) for r in log for side in ("res1", "res2") for v in (bu.LIMIT - 2, bu.LIMIT - 1) if v in r[side]}
    # (the first side at 2^32 - 1: limit_first, below)
    assert seen == {("res1", bu.LIMIT - 2), ("res2", bu.LIMIT - 2), ("res2", bu.LIMIT - 1)}
    assert any(len(r["res1"]) == 1 or len(r["res2"]) == 1 for r in log), "a side of one arc"
    assert any(r["flip"] for r in bu.limit_log()) and any(a["flip"] and not b["flip"] for a, b in zip(bu.limit_log(), bu.limit_log()[1:]))
    assert any(not a["flip"] and b["flip"] for a, b in zip(bu.limit_log(), bu.limit_log()[1:])), "a flip directly behind a swap"


def test_gpu_inputs_long_launch_instance_leaves_two_resumes():
    inst = bu.fold_instance()
    em = ci.emul(inst, 0)
    first, second = bu.FOLD_BUDGETS[0], bu.FOLD_BUDGETS[1]
    assert ci.fits_lds(inst.n, inst.m)
    assert em["pivots"] > first + second + 1 and em["status"] == "optimal"
    assert ci.emul(inst, 0, first)["status"] == "iteration_limit" and ci.emul(inst, 0, first + second)["pivots"] == first + second


@pytest.mark.parametrize("which", ("netgen_64", "netgen_256", "limit"))
def test_gpu_inputs_stepped_pivots_hold_either_side_leaving_from_either_buffer(host, which):
    inst = {"netgen_64": lambda: bu.netgen(64, 512), "netgen_256": lambda: bu.netgen(256, 1024), "limit": bu.limit}[which]()
    r = _twin(host, inst, max_pivots=bu.STEPS)
    assert r["pivots"] == bu.STEPS and r["bad_ctx"] == 0 and r["bad_arrays"] == 0
    assert 0 < r["first_cur1"] < r["first"] and 0 < r["second_cur1"] < r["second"], r


@pytest.mark.parametrize("leave", bu.EMPTY_SIDES)
def test_gpu_inputs_planted_side_of_length_0(leave):
    import small_loop_reduce_instances as ri

    p = bu.empty_side_plant(leave)
    ref = ri.TracedSimplex(p.pl)
    assert ref.step()
    first = ref.log[0]
    assert first["deep"] > 3, "searched, not climbed"
    empty, full = ("res2", "res1") if leave == "first_side" else ("res1", "res2")
    assert len(first[empty]) == 0 and len(first[full]) >= 6, first


def test_gpu_inputs_limit_first_puts_one_past_the_narrow_limit_on_the_first_side():
    inst = bu.limit_first()
    assert ci.fits_lds(inst.n, inst.m)
    log = [r for r in bu.limit_first_log() if r["deep"] > 3]
    wide_first = [r for r in log if bu.LIMIT - 1 in r["res1"]]
    assert len(wide_first) >= 10, "searched pivots whose first side holds a residual of exactly 2^32 - 1"
