"""The selection arithmetic round the fused LDS loop's 32-bit wave reductions -- which ratio-test sides are narrow, the 32-bit key of
a residual, the winner out of the ballot, the two stages of the front kernel's arg-max (``csrc/mcf_core.h``: ``mcf_ratio_*``,
``mcf_argmax_*``) -- on the host: ``csrc/mcf_small_reduce_host.cpp`` runs the functions the device code calls round plain loops over
64 "lanes", and the tests hold the results against a direct 64-bit statement of the rule in Python ints.  No GPU.

One test builds that file and a stand-alone program round it with the compiler's address and undefined-behaviour checks and runs
the program on the same cases.  The last tests vet the inputs of ``test_gpu_small_loop_reduce.py``."""

from __future__ import annotations

import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import small_loop_control_instances as ci
import small_loop_instances as sl
import small_loop_reduce_instances as ri

INF = ri.MCF_INF
EDGES = (0, (1 << 32) - 3, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, INF - 1, INF, -5)
LENGTHS = (0, 1, 63, 64, 65, 128, 129)


# ------------------------------------------------------------------ the rule, stated directly
def rule_side(res, last: bool):
    d, k = INF, -1
    for i, r in enumerate(res):
        if (r <= d) if last else (r < d):
            d, k = r, i
    return d, k


def rule_narrow(res) -> bool:
    return all(r == INF or 0 <= r <= (1 << 32) - 2 for r in res)


def rule_argmax(packed):
    best = max(range(64), key=lambda l: packed[l])
    return (best, packed[best]) if packed[best] >> 32 else (0, 0)


def rule_stages(packed) -> int:
    top = max(p >> 32 for p in packed)
    return 2 if top and sum(1 for p in packed if p >> 32 == top) > 1 else 1


# ------------------------------------------------------------------ the cases
def ratio_cases():
    out = []
    rng = np.random.default_rng(20261)
    pools = {"narrow": (0, 1, 7, 1000, (1 << 31), (1 << 32) - 3, (1 << 32) - 2, INF),
             "limit": (5, (1 << 32) - 2, (1 << 32) - 1, INF),
             "wide": (0, 3, 1 << 32, (1 << 40) + 1, INF - 1, INF),
             "odd": (-5, 0, 9, INF, INF + 1)}
    for n in LENGTHS:
        for e in EDGES:                                     # the edge value alone among larger-or-equal ones, at every place
            for at in sorted({0, n // 2, n - 1} & set(range(n))):
                res = [INF] * n
                res[at] = e
                out.append(res)
        out.append([INF] * n)                               # nothing below MCF_INF
        for v in (0, 12345, (1 << 32) - 2, 1 << 33):        # ties: the minimum at the first, the middle and the last index
            for places in ((0, n - 1), (0, n // 2), (n // 2, n - 1), (0, n // 2, n - 1), tuple(range(n))):
                if n >= 2:
                    res = [v + 1 + int(x) for x in rng.integers(0, 50, n)]
                    for q in places:
                        res[q] = v
                    out.append(res)
        for name, pool in pools.items():                    # seeded mixes
            for _ in range(6):
                out.append([int(pool[j]) for j in rng.integers(0, len(pool), n)])
        for _ in range(6):                                  # one residual past the limit somewhere among narrow ones
            res = [int(x) for x in rng.integers(0, 1 << 20, n)]
            if n:
                res[int(rng.integers(0, n))] = (1 << 32) - 1 + int(rng.integers(0, 3))
            out.append(res)
    return out


def argmax_cases():
    out = []
    rng = np.random.default_rng(20262)
    none = 0xffffffff                                       # a lane with nothing eligible, as the sweep leaves it

    def packed(viols, ids):
        return [(int(v) << 32) | (~int(i) & 0xffffffff) if v else none for v, i in zip(viols, ids)]

    ids = rng.permutation(5000)[:64]
    out.append([none] * 64)                                                               # nothing eligible
    for lane in (0, 31, 63):
        v = np.zeros(64, np.int64)
        v[lane] = 17
        out.append(packed(v, ids))                                                        # one eligible lane
    for lane in (0, 63, 20):
        v = rng.integers(1, 1000, 64)
        v[lane] = 5000
        out.append(packed(v, ids))                                                        # a unique maximum in lane 0 / 63 / inside
    for lanes in ((0, 63), (0, 1), (62, 63), (5, 40, 41), tuple(range(64))):
        v = rng.integers(1, 1000, 64)
        v[list(lanes)] = 0x7fffffff
        out.append(packed(v, ids))                                                        # equal violations, different ids
        out.append(packed(v, np.sort(ids)))
        out.append(packed(v, np.sort(ids)[::-1]))
    for _ in range(40):
        out.append(packed(rng.integers(0, 4, 64), rng.permutation(200)[:64]))             # seeded, tie-rich
    for _ in range(20):
        out.append(packed(rng.integers(0, 1 << 31, 64), rng.permutation(1 << 20)[:64]))
    return out


RATIO = ratio_cases()
ARGMAX = argmax_cases()


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_small_reduce_host()))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.mcf_small_ratio_side_host.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.mcf_small_ratio_side_host.restype = ctypes.c_int
    lib.mcf_small_argmax_host.argtypes = [vp, i32, vp, vp, vp]
    lib.mcf_small_argmax_host.restype = ctypes.c_int
    return lib


def _side(lib, res, last, allow):
    a = np.array(res, np.int64)
    d, k, nar = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.mcf_small_ratio_side_host(a.ctypes.data_as(ctypes.c_void_p), len(res), int(last), int(allow), ctypes.byref(d), ctypes.byref(k),
                                       ctypes.byref(nar))
    assert rc == 0
    return d.value, k.value, nar.value


def _argmax(lib, packed, staged):
    a = np.array(packed, np.uint64)
    lane, stages, key = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_uint64(0)
    rc = lib.mcf_small_argmax_host(a.ctypes.data_as(ctypes.c_void_p), int(staged), ctypes.byref(lane), ctypes.byref(key), ctypes.byref(stages))
    assert rc == 0, "not exactly one lane writes the wave's slot"
    return lane.value, key.value, stages.value


@pytest.mark.parametrize("last", (False, True))
def test_ratio_side_returns_the_rules_winner_on_either_path(host, last):
    seen = {0: 0, 1: 0}
    for res in RATIO:
        want = rule_side(res, last)
        d, k, nar = _side(host, res, last, True)
        assert (d, k) == want and nar == int(rule_narrow(res)), (res, last, d, k, nar, want)
        d, k, nar = _side(host, res, last, False)
        assert (d, k) == want and nar == 0, (res, last, d, k, want)
        seen[int(rule_narrow(res))] += 1
    assert seen[0] > 100 and seen[1] > 100


def test_ratio_cases_hold_the_edges():
    assert {len(r) for r in RATIO} == set(LENGTHS)
    flat = {x for r in RATIO for x in r}
    assert set(EDGES) <= flat
    # an all-MCF_INF side: the first side returns nothing, the second its last index
    assert rule_side([INF] * 65, False) == (INF, -1) and rule_side([INF] * 65, True) == (INF, 64)
    # a narrow side whose winner lies in the second and in the third stride, and a wide residual there that decides the path
    assert any(len(r) > 128 and rule_narrow(r) and rule_side(r, True)[1] >= 128 for r in RATIO)
    assert any(len(r) > 64 and rule_narrow(r[:64]) and not rule_narrow(r) for r in RATIO)


def test_argmax_names_the_64_bit_maximum_in_either_form(host):
    stages_seen = set()
    for p in ARGMAX:
        want = rule_argmax(p)
        lane, key, stages = _argmax(host, p, True)
        assert (lane, key) == want and stages == rule_stages(p), (p, lane, key, stages, want)
        lane, key, stages = _argmax(host, p, False)
        assert (lane, key) == want and stages == 0, (p, lane, key, want)
        stages_seen.add(rule_stages(p))
    assert stages_seen == {1, 2}


def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    """The same code, compiled together with a program of its own with -fsanitize=address,undefined, on the same cases."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "small_reduce_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_small_reduce_driver.cpp"), str(ge.CSRC / "mcf_small_reduce_host.cpp")], check=True, cwd=str(ge.CSRC))
    path = tmp_path / "cases.bin"
    want = []
    with open(path, "wb") as f:
        for last in (0, 1):
            for res in RATIO:
                f.write(np.array([0, len(res), last], "<i8").tobytes() + np.array(res, "<i8").tobytes())
                d, k = rule_side(res, bool(last))
                want.append(f"r {d} {k} {int(rule_narrow(res))}")
        for p in ARGMAX:
            f.write(np.array([1, 64, 0], "<i8").tobytes() + np.array(p, "<u8").tobytes())
            lane, key = rule_argmax(p)
            want.append(f"a {lane} {key} {rule_stages(p)}")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines() == want


# ------------------------------------------------------------------ the inputs of test_gpu_small_loop_reduce.py
def _same_solve(inst):
    """The trace is of the pivots the engine makes: the emulation ends with the same count, status and flows."""
    tr, em = ri.trace(inst), ci.emul(inst, 0)
    assert em["status"] == tr["status"] == "optimal" and em["pivots"] == tr["pivots"], inst.name
    assert np.array_equal(em["flow"], tr["flow"]), inst.name
    return tr


@pytest.mark.parametrize("qmax, tie_rich", ri.WIDE_PARAMS, ids=ri.WIDE_IDS)
def test_gpu_inputs_wide_family_straddles_the_limit(qmax, tie_rich):
    inst = ri.wide(qmax, tie_rich)
    assert ci.fits_lds(inst.n, inst.m) and int(np.abs(inst.cost).max()) <= 1000
    tr = _same_solve(inst)
    assert tr["narrow_sides"] > 0 and tr["climb_then_search"] > 0 and tr["flip_then_swap"] > 0, inst.name
    if qmax >= 1 << 32:
        assert tr["wide_sides"] > 0, inst.name
    if qmax >= 1 << 33:                                     # ... and both kinds among the pivots made one launch each
        assert tr["first_steps"]["wide_sides"] > 0 and tr["first_steps"]["narrow_sides"] > 0, inst.name
    if qmax == 1 << 31 and not tie_rich:
        assert tr["first_steps"]["wide_sides"] == 0, inst.name
    if tie_rich:
        assert tr["ties_first"] > 0 and tr["ties_second"] > 0 and tr["shared_max"] >= 5, inst.name
        assert tr["first_steps"]["ties_first"] > 0 and tr["first_steps"]["ties_second"] > 0 and tr["first_steps"]["shared_max"] >= 5, inst.name


def test_gpu_inputs_open_ring_has_sides_of_nothing_but_infinity():
    inst = ri.open_ring()
    assert ci.fits_lds(inst.n, inst.m)
    tr = _same_solve(inst)
    assert tr["all_inf_sides"] > 0 and tr["wide_sides"] > 0 and tr["narrow_sides"] > 0


@pytest.mark.parametrize("n, m", ri.NODE_SHAPES)
def test_gpu_inputs_netgen_shapes(n, m):
    tr = _same_solve(sl.netgen(n, m))
    assert tr["narrow_sides"] > 0 and tr["wide_sides"] == 0
    assert tr["ties_first"] > 0 and tr["ties_second"] > 0 and tr["flip_then_swap"] > 0 and tr["climb_then_search"] > 0


def test_gpu_inputs_capped_transport_flips_and_shares_violations():
    tr = _same_solve(ci.capped_transport())
    assert tr["flip_then_swap"] > 0 and tr["first_steps"]["flip_then_swap"] > 0
    assert tr["shared_max"] >= 5 and tr["first_steps"]["shared_max"] >= 5
    assert tr["ties_first"] > 0 and tr["ties_second"] > 0 and tr["climb_then_search"] > 0


@pytest.mark.parametrize("n1, n2, ts", ri.SIDE_PARAMS, ids=ri.SIDE_IDS)
def test_gpu_inputs_planted_sides(n1, n2, ts):
    p = ri.side_plant(n1, n2, ts)
    assert ci.fits_lds(p.inst.n, p.inst.m) and p.inst.n + 1 <= 1024
    f = ri.side_first_pivot(n1, n2, ts)
    assert f["deep"] > 3 and sorted((len(f["res1"]), len(f["res2"]))) == sorted((n1, n2))
    assert 63 <= min(n1, n2) and max(n1, n2) <= 66
    s = f["summary"]
    assert s["narrow_sides"] == 2 and s["long_sides"] == (n1 > 64) + (n2 > 64)
    # the ties the case plants are ties the reductions see
    if "first" in ts:
        assert s["ties_first"] + s["ties_second"] >= 1
    if "first" in ts and "second" in ts:
        assert s["ties_first"] == 1 and s["ties_second"] == 1


def test_gpu_inputs_cover_a_long_side():
    assert sum(ri.side_first_pivot(*p)["summary"]["long_sides"] for p in ri.SIDE_PARAMS) >= 4
