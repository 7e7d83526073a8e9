"""mcf_fork / mcf_restore without a device: the ABI surface, the chunk arithmetic of the copy kernel (csrc/mcf_core.h:
mcf_fork_*) through its host restatement (csrc/mcf_fork_host.cpp) -- every byte of every segment reaches every destination
exactly once, nothing is written outside -- and the pure scenario mapping ``map_scenario``.  Every comparison is exact."""

from __future__ import annotations

import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from network_flow_solver_amd import build_problem, engine, generators
from network_flow_solver_amd.data import SoAProblem
from network_flow_solver_amd.exceptions import InvalidProblemError
from network_flow_solver_amd.simplex import flatten_problem, flatten_soa, map_cost_changes, map_rhs_changes, map_scenario


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_fork_host()))
    lib.mcf_fork_cover_host.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                        ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)]
    lib.mcf_fork_cover_host.restype = ctypes.c_int
    return lib


def segment_lists(chunk: int):
    node_arrays = [4 * (n + 1) for n in (64, 65, 66, 67)]
    return {
        "small lengths": [0, 1, 15, 16, 17],
        "node arrays": node_arrays,
        "mixed, empty segments first, inside and last": [0, 17] + node_arrays + [0, 0, 16, 1, 0],
        "one segment longer than a grid's stride": [15, 64 * chunk + 4 * 66 + 3, 0, 16],
        "whole chunks": [chunk, 2 * chunk, chunk - 1, chunk + 1],
    }


def cover(lib, lens, count, grid):
    lens = np.asarray(lens, np.int64)
    stride = int(lens.max()) + 16
    writes = np.zeros((count, len(lens), stride), np.uint8)
    reads = np.zeros((len(lens), stride), np.uint32)
    outside = ctypes.c_int64(-1)
    rc = lib.mcf_fork_cover_host(len(lens), lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count, grid, stride,
                                 writes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), reads.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                 ctypes.byref(outside))
    assert rc == 0
    return writes, reads, int(outside.value)


@pytest.mark.parametrize("grid", (1, 3, 8, 64, 2048))
@pytest.mark.parametrize("count", ("1", "2", "group + 1"))
def test_every_byte_reaches_every_destination_exactly_once(host, count, grid):
    chunk, group = host.mcf_fork_chunk_bytes_host(), host.mcf_fork_group_host()
    assert chunk % 16 == 0 and group >= 2
    count = group + 1 if count == "group + 1" else int(count)
    for name, lens in segment_lists(chunk).items():
        writes, reads, outside = cover(host, lens, count, grid)
        expect = (np.arange(writes.shape[2])[None, :] < np.asarray(lens)[:, None]).astype(np.uint8)
        assert outside == 0, name
        for d in range(count):
            assert np.array_equal(writes[d], expect), (name, d)
        # a chunk is loaded once per group of destinations, not once per destination
        groups = -(-count // group)
        assert np.array_equal(reads, expect.astype(np.uint32) * groups), name


def test_no_destination_no_work(host):
    writes, reads, outside = cover(host, [17, 4096], 0, 8)
    assert outside == 0 and not reads.any()


def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    """The same code, compiled together with a program of its own with -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "fork_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_fork_driver.cpp"), str(ge.CSRC / "mcf_fork_host.cpp")], check=True, cwd=str(ge.CSRC))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 12 and all(ln.endswith("wrong 0 outside 0") for ln in lines)


def test_abi_exports_fork_and_restore():
    assert {"mcf_fork", "mcf_restore"} <= set(ge.declared_symbols())
    lib = engine.load_library()
    assert hasattr(lib, "mcf_fork") and hasattr(lib, "mcf_restore")
    assert ctypes.sizeof(engine.McfForkReport) == 32
    # null arguments and a negative count are refused before anything is touched (no device needed)
    out = (ctypes.c_void_p * 1)()
    assert lib.mcf_fork(None, 1, out, None) == -1
    assert lib.mcf_restore(out, 1, None, None) == -1


# ------------------------------------------------------------------ scenario mapping

def _object_problem():
    nodes = [{"id": f"n{i}", "supply": s} for i, s in enumerate((6.0, 0.0, 0.0, -2.5, -3.5))]
    arcs = [{"tail": "n0", "head": "n1", "capacity": 10.0, "cost": 1.5}, {"tail": "n0", "head": "n2", "capacity": 4.0, "cost": 2.0},
            {"tail": "n1", "head": "n3", "capacity": 5.0, "cost": 1.0}, {"tail": "n2", "head": "n4", "capacity": 6.0, "cost": 0.5},
            {"tail": "n1", "head": "n4", "capacity": None, "cost": 3.0}, {"tail": "n2", "head": "n3", "capacity": 3.0, "cost": 2.5}]
    return build_problem(nodes, arcs, directed=True, tolerance=1e-6)


def _soa_problem():
    inst = generators.netgen_style(16, 64, seed=5)
    return SoAProblem(inst.n, tail=inst.tail, head=inst.head, cost=inst.cost, capacity=inst.cap, supply=inst.supply)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


def test_valid_scenarios_map_like_the_map_functions():
    tol = 1e-6
    flat = flatten_problem(_object_problem(), tol)
    sc = {"costs": {("n0", "n1"): 2.5, ("n2", "n3"): 0.0}, "supplies": {"n0": 7.0, "n3": -3.5}, "capacities": {("n1", "n4"): 2.0, ("n0", "n2"): None}}
    got = map_scenario(flat, sc, tol)
    _same(got["costs"], map_cost_changes(flat, sc["costs"], tol))
    _same(got["supplies"], map_rhs_changes(flat, sc["supplies"], None, tol))
    _same(got["capacities"], map_rhs_changes(flat, None, sc["capacities"], tol))
    assert map_scenario(flat, {}, tol) == {"costs": None, "supplies": None, "capacities": None}
    only = map_scenario(flat, {"capacities": sc["capacities"]}, tol)
    assert only["costs"] is None and only["supplies"] is None
    sflat = flatten_soa(_soa_problem(), tol)
    ssc = {"costs": (np.array([3, 9, 3]), np.array([5, 6, 7])), "capacities": (np.array([1]), np.array([-1]))}
    got = map_scenario(sflat, ssc, tol)
    _same(got["costs"], map_cost_changes(sflat, ssc["costs"], tol))
    _same(got["capacities"], map_rhs_changes(sflat, None, ssc["capacities"], tol))
    assert got["supplies"] is None


def test_unknown_key_and_invalid_edit_raise():
    tol = 1e-6
    flat = flatten_problem(_object_problem(), tol)
    with pytest.raises(InvalidProblemError, match="unknown key 'arcs'"):
        map_scenario(flat, {"costs": {("n0", "n1"): 2.0}, "arcs": []}, tol)
    with pytest.raises(InvalidProblemError):
        map_scenario(flat, {"costs": {("n0", "n4"): 2.0}}, tol)              # no such arc
    with pytest.raises(InvalidProblemError):
        map_scenario(flat, {"supplies": {"n0": 9.0}}, tol)                   # no longer balanced
    with pytest.raises(InvalidProblemError):
        map_scenario(flat, [("costs", {})], tol)                             # not a mapping


class _NoFork:
    """A stand-in solver that fails the test when anything but the mapping is reached."""

    def __init__(self, flat):
        self.flat, self.tolerance = flat, 1e-6

    def fork(self, count):
        raise AssertionError("a fork was made before every scenario was checked")


def test_solve_scenarios_checks_every_scenario_before_any_fork():
    from network_flow_solver_amd import solve_scenarios

    sv = _NoFork(flatten_problem(_object_problem(), 1e-6))
    good = {"costs": {("n0", "n1"): 2.5}}
    with pytest.raises(InvalidProblemError, match="unknown key"):
        solve_scenarios(sv, [good, {"cost": {}}])
    with pytest.raises(InvalidProblemError):
        solve_scenarios(sv, [good, good, {"capacities": {("n4", "n0"): 1.0}}])
    assert solve_scenarios(sv, []) == []
