"""The even deal of the fused LDS loop's Dantzig register sweep (``csrc/mcf_core.h``: ``mcf_even_*``) on the host:
``csrc/mcf_small_cycle_regs_host.cpp`` runs the functions the device code calls round plain loops over the workgroup's lanes, in the
order of the device code, and the tests check the lane-to-arc map and the slot count: every arc is priced exactly once, by lane
``i % THREADS`` in slot ``i // THREADS``, the slot unpacks to the arc, and a sweep executes ``ceil(m / THREADS)`` slots rounded up
to one of the two compiled counts.  No GPU.

One test builds that file and a stand-alone program round it with the compiler's address and undefined-behaviour checks and runs
the program on the same cases."""

from __future__ import annotations

import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

# (THREADS, the two compiled slot counts): small_reg_arcs_few of the front kernels / small_reg_arcs of mcf_engine.hip at the two
# compiled widths; GENERAL: the one sweep of small_reg_arcs slots (few == reg), which no kernel runs under the even deal today
WIDTHS = ((256, 8, 10), (1024, 2, 3))
GENERAL = ((256, 10, 10), (1024, 3, 3))


def sizes(threads: int, reg: int):
    """The arc counts the map can go wrong at: one arc, one short of / exactly / one past a slot, the flagship's eight slots of 256
    lanes, one arc past the register slots (the LDS loop's first), sizes that are no multiple of the width, nothing at all."""
    return (0, 1, threads - 1, threads, threads + 1, 8 * threads, reg * threads + 1, 5 * threads + 37, 2048, 2047, reg * threads,
            12 * threads + 3)


CASES = [(base, m, t, few, reg) for t, few, reg in WIDTHS + GENERAL for m in sizes(t, reg) for base in (0, 7)]


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_small_cycle_regs_host()))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.mcf_small_even_deal_host.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.mcf_small_even_deal_host.restype = ctypes.c_int
    lib.mcf_small_even_slots_host.argtypes = [i32, i32]
    lib.mcf_small_even_slots_host.restype = i32
    return lib


def _deal(lib, base, m, threads, few, reg):
    times, lane, slot, lds = (np.full(max(m, 1), fill, np.int32) for fill in (0, -1, -1, -1))
    slots, masked = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = lib.mcf_small_even_deal_host(base, m, threads, few, reg, *(a.ctypes.data_as(ctypes.c_void_p) for a in (times, lane, slot, lds)),
                                      ctypes.byref(slots), ctypes.byref(masked))
    assert rc == 0, (rc, base, m, threads)
    return times[:m], lane[:m], slot[:m], lds[:m], slots.value, masked.value


def _want_slots(m, threads, few, reg):
    need = -(-m // threads)
    return few if need <= few else reg


@pytest.mark.parametrize("base, m, threads, few, reg", CASES)
def test_every_arc_is_priced_exactly_once(host, base, m, threads, few, reg):
    times, lane, slot, lds, slots, masked = _deal(host, base, m, threads, few, reg)
    i = np.arange(m)
    assert (times == 1).all()
    assert np.array_equal(lane, i % threads) and np.array_equal(slot, i // threads)
    assert np.array_equal(lds, (i // threads >= reg).astype(np.int32))          # the register slots first, the rest from LDS
    assert host.mcf_small_even_slots_host(m, threads) == -(-m // threads)
    assert slots == _want_slots(m, threads, few, reg)
    # executed register slots = the arcs they hold + the masked ones; a full last slot masks nothing beyond the compiled count
    in_regs = min(m, reg * threads)
    assert masked == slots * threads - min(in_regs, slots * threads)
    assert slot.max(initial=0) < 512                                              # the slot field of the info word: 9 bits


def test_cases_hold_the_edges():
    for threads, few, reg in WIDTHS:
        ms = set(sizes(threads, reg))
        assert {1, threads - 1, threads, threads + 1, 8 * threads, reg * threads + 1} <= ms
        assert any(m % threads and m > threads for m in ms)
        assert {_want_slots(m, threads, few, reg) for m in ms} == {few, reg}
        assert any(m > reg * threads for m in ms)
    # the flagship: 2 048 arcs are eight slots of 256 lanes -- the shorter compiled sweep -- and two of 1 024
    assert _want_slots(2048, 256, 8, 10) == 8 and _want_slots(2048, 1024, 2, 3) == 2


def test_constants_are_the_kernels():
    """WIDTHS restates small_reg_arcs and the front kernels' small_reg_arcs_few: a change there has to show up here."""
    text = (ge.CSRC / "mcf_engine.hip").read_text()
    assert "constexpr int small_reg_arcs(int threads) { return threads == 256 ? 10 : 3; }" in text
    assert ("constexpr int small_reg_arcs_few(int threads, bool front) "
            "{ return !front ? small_reg_arcs(threads) : (threads == 256 ? 8 : 2); }") in text
    assert 'static_assert(THREADS == 256 || THREADS == 1024, "the two widths the loop is tuned and instantiated for");' in text


def test_bad_arguments_are_refused(host):
    s, k = ctypes.c_int32(0), ctypes.c_int64(0)
    assert host.mcf_small_even_deal_host(0, 4, 0, 2, 3, None, None, None, None, ctypes.byref(s), ctypes.byref(k)) == -1
    assert host.mcf_small_even_deal_host(0, 4, 256, 4, 3, None, None, None, None, ctypes.byref(s), ctypes.byref(k)) == -1
    assert host.mcf_small_even_deal_host(0, 4, 256, 2, 3, None, None, None, None, ctypes.byref(s), ctypes.byref(k)) == -1


def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    """The same code, compiled together with a program of its own with -fsanitize=address,undefined, on the same cases."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "small_cycle_regs_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_small_cycle_regs_driver.cpp"), str(ge.CSRC / "mcf_small_cycle_regs_host.cpp")], check=True,
                   cwd=str(ge.CSRC))
    args, want = [], []
    for base, m, threads, few, reg in CASES:
        args += [str(x) for x in (base, m, threads, few, reg)]
        slots = _want_slots(m, threads, few, reg)
        in_regs = min(m, reg * threads)
        want.append(f"{slots} {slots * threads - min(in_regs, slots * threads)} {m - in_regs} {(m - 1) // threads if m else -1}")
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines() == want


# ------------------------------------------------------------------ the inputs of test_gpu_small_loop_regs.py
def test_gpu_inputs_fit_the_plan_and_hold_the_edges():
    import test_gpu_small_loop_regs as g

    g.test_inputs_fit_the_lds_plan_and_hold_the_edges()
    import small_loop_control_instances as ci
    for name in ("capped_transport", "wide_ties_31", "one_bucket", "lds_tail"):
        for rule in (0, 1, 2):
            assert ci.emul(g.INSTANCES[name](), rule)["status"] == "optimal", (name, rule)
