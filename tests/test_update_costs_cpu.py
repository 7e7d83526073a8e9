"""Host side of re-optimising after a cost change (``mcf_update_costs``): the header declares the entry point and the
ctypes binding matches it, and the shim's mapping / validation of cost changes (``simplex.map_cost_changes``) -- a pure
function, so it needs no device."""

from __future__ import annotations

import copy
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT

import network_flow_solver_amd as nfs
from network_flow_solver_amd import engine
from network_flow_solver_amd.data import SoAProblem
from network_flow_solver_amd.exceptions import InvalidProblemError, SolverConfigurationError
from network_flow_solver_amd.simplex import flatten_problem, flatten_soa, map_cost_changes

_CTYPES = {
    "mcf_handle*": ctypes.c_void_p,
    "int64_t": ctypes.c_int64,
    "const int64_t*": ctypes.POINTER(ctypes.c_int64),
}


def _prototype(name: str):
    """(return type, [argument types]) of ``name`` as include/mcf.h declares it, comments stripped."""
    text = (ROOT / "include" / "mcf.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert found, f"{name} is not declared in include/mcf.h"
    args = []
    for a in found.group(2).split(","):
        a = " ".join(a.split())
        args.append(re.sub(r"\s*\w+$", "", a).replace(" *", "*"))   # drop the parameter name
    return found.group(1), args


def test_header_declares_update_costs_and_the_binding_matches():
    ret, args = _prototype("mcf_update_costs")
    assert ret == "int" and args == ["mcf_handle*", "int64_t", "const int64_t*", "const int64_t*"]
    assert "mcf_update_costs" in engine.ABI_SYMBOLS
    lib = engine.load_library()
    fn = lib.mcf_update_costs
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [_CTYPES[a] for a in args]
    assert callable(getattr(engine.McfEngine, "update_costs"))
    assert callable(getattr(nfs.NetworkSimplex, "update_costs"))
    assert lib.mcf_abi_version() == 3           # a new entry point, the same ABI version


def test_null_handle_is_a_bad_argument_without_a_device():
    lib = engine.load_library()
    assert lib.mcf_update_costs(None, 0, None, None) == -1


def _problem():
    nodes = [{"id": "a", "supply": 3.0}, {"id": "b", "supply": 0.0}, {"id": "c", "supply": -3.0}]
    arcs = [{"tail": "a", "head": "b", "capacity": 5.0, "cost": 1.25},
            {"tail": "b", "head": "c", "capacity": 5.0, "cost": 2.0},
            {"tail": "a", "head": "b", "capacity": 2.0, "cost": 0.5},      # parallel to the first
            {"tail": "a", "head": "c", "capacity": 4.0, "cost": 7.0}]
    return nfs.build_problem(nodes, arcs, True, 1e-6)


def test_mapping_scales_and_resolves_parallel_arcs_like_the_warm_start_key_map():
    p = _problem()
    f = flatten_problem(p)
    assert f.cost_scale == 100 and f.keys == [("a", "b"), ("a", "b"), ("a", "c"), ("b", "c")]
    idx, ci, cf = map_cost_changes(f, {("a", "b"): 0.75, ("b", "c"): 3}, 1e-6)
    # of the two (a, b) arcs the LAST index takes the change
    assert idx.tolist() == [1, 3] and ci.tolist() == [75, 300] and cf.tolist() == [0.75, 3.0]
    assert ci.dtype == np.int64 and idx.dtype == np.int64
    # an empty change set is fine
    idx, ci, cf = map_cost_changes(f, {}, 1e-6)
    assert idx.shape == ci.shape == cf.shape == (0,)


def test_mapping_refuses_unknown_keys_and_costs_off_the_scale_and_changes_nothing():
    p = _problem()
    before = copy.deepcopy(p)
    f = flatten_problem(p)
    cost0, orig0 = f.cost.copy(), f.orig_cost.copy()
    with pytest.raises(InvalidProblemError, match="not in the problem"):
        map_cost_changes(f, {("a", "b"): 1.0, ("c", "a"): 1.0}, 1e-6)
    with pytest.raises(InvalidProblemError, match="1/100"):
        map_cost_changes(f, {("a", "b"): 0.755}, 1e-6)          # needs a third decimal, the instance was scaled by 100
    with pytest.raises(InvalidProblemError):
        map_cost_changes(f, {("a", "b"): float("nan")}, 1e-6)
    with pytest.raises(SolverConfigurationError):
        map_cost_changes(f, {("a", "b"): 2.0 ** 31 / 100}, 1e-6)
    with pytest.raises(InvalidProblemError):
        map_cost_changes(f, [(("a", "b"), 1.0)], 1e-6)          # not a mapping
    # within the tolerance of a grid point is that grid point
    idx, ci, _ = map_cost_changes(f, {("a", "c"): 6.9999999999}, 1e-6)
    assert idx.tolist() == [2] and ci.tolist() == [700]
    assert np.array_equal(f.cost, cost0) and np.array_equal(f.orig_cost, orig0)
    assert p == before                                            # the caller's problem is untouched


def test_mapping_of_soa_changes_last_duplicate_wins():
    soa = SoAProblem(3, [0, 1, 0], [1, 2, 2], [4, 5, 6], [9, 9, 9], [2, 0, -2])
    f = flatten_soa(soa)
    cost0 = soa.cost.copy()
    idx, ci, cf = map_cost_changes(f, (np.array([2, 0, 2]), np.array([10, -3, 11])), 1e-6)
    assert dict(zip(idx.tolist(), ci.tolist())) == {0: -3, 2: 11}
    assert cf.tolist() == [float(c) for c in ci.tolist()]
    for bad in ((np.array([3]), np.array([1])), (np.array([-1]), np.array([1])), (np.array([0, 1]), np.array([1])),
                (np.array([0.5]), np.array([1]))):
        with pytest.raises(InvalidProblemError):
            map_cost_changes(f, bad, 1e-6)
    with pytest.raises(InvalidProblemError):
        map_cost_changes(f, (np.array([0]), np.array([1.5])), 1e-6)   # SoA costs are integers (scale 1)
    with pytest.raises(SolverConfigurationError):
        map_cost_changes(f, (np.array([0]), np.array([2 ** 31])), 1e-6)
    with pytest.raises(InvalidProblemError):
        map_cost_changes(f, {0: 1}, 1e-6)                             # a mapping is the object model's form
    assert np.array_equal(soa.cost, cost0) and f.cost is soa.cost
