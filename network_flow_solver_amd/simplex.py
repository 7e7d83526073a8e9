"""``NetworkSimplex`` facade: the reference's solver object, backed by the HIP engine.

Constructor / ``solve`` signature and the shape of everything that comes back
follow /root/reference/src/network_solver/simplex.py (``NetworkSimplex`` :62,
``__init__`` :99, ``solve`` :1446-1452).  What happens in between is different:

* the problem is flattened once into integer structure-of-arrays form
  (``flatten_problem``: the reference's node/arc ordering :149,:395, lower-bound
  shift :403-428, undirected expansion data.py:162-223, plus a decimal scaling
  step because the engine is integer);
* the pivot loop (:1109-1160, :1176-1425) runs on the MI355X through
  ``engine.McfEngine`` -- nothing in this module prices an arc or walks a tree;
* results are mapped back with the reference's post-processing (:1703-1765):
  flows summed per ``(tail, head)`` key, ``|f| <= tolerance`` dropped,
  ``round(., 12)``, objective over the original costs.

There is no CPU fallback here: without the HIP library or a GPU,
``NetworkSimplex(...)`` raises ``EngineUnavailableError``.
"""

from __future__ import annotations

import copy
import logging
import math
import time
from dataclasses import dataclass, replace

import numpy as np

from . import engine as _engine
from .data import (ArrayBasis, Basis, FlowResult, LazyDuals, LazyFlows, NetworkProblem, ProgressCallback, ProgressInfo,
                   SoAProblem, SolverOptions, SupplyRange)
from .exceptions import InvalidProblemError, SolverConfigurationError, UnboundedProblemError
from .specializations import analyze_network_structure, entering_rule_options

_MAX_DECIMALS = 9


@dataclass
class FlatProblem:
    """Integer SoA image of a NetworkProblem plus what is needed to map results back."""

    node_ids: list[str]            # index -> id, string-sorted like the reference
    keys: list[tuple[str, str]]    # per arc (tail id, head id), reference arc order
    tail: np.ndarray               # int32[m]
    head: np.ndarray               # int32[m]
    cost: np.ndarray               # int64[m]   cost * cost_scale
    cap: np.ndarray                # int64[m]   (capacity - lower) * flow_scale, -1 = unlimited
    supply: np.ndarray             # int64[n]   (supply shifted by lower bounds) * flow_scale
    lower: np.ndarray              # float64[m] original lower bounds (the shift)
    orig_cost: np.ndarray          # float64[m]
    flow_scale: int
    cost_scale: int
    soa: bool = False              # built from an SoAProblem: ids / keys are virtual sequences, results stay flat


class _IdSeq:
    """node index -> DIMACS id string, without holding n strings."""

    def __init__(self, n: int):
        self._n = n

    def __len__(self) -> int:
        return self._n

    def __getitem__(self, i: int) -> str:
        if not 0 <= i < self._n:
            raise IndexError(i)
        return str(i + 1)

    def __iter__(self):
        return (str(i + 1) for i in range(self._n))


class _KeySeq:
    """arc index -> (tail id, head id)."""

    def __init__(self, tail: np.ndarray, head: np.ndarray):
        self._tail, self._head = tail, head

    def __len__(self) -> int:
        return int(self._tail.shape[0])

    def __getitem__(self, i: int) -> tuple[str, str]:
        return (str(int(self._tail[i]) + 1), str(int(self._head[i]) + 1))


def flatten_soa(problem: SoAProblem, tolerance: float | None = None) -> FlatProblem:
    """SoAProblem -> the engine's arrays: the lower-bound shift of simplex.py:413-428 and the checks of :381-412,
    vectorised; no per-arc Python object.  Arcs and nodes keep the file's order (the reference's string sort of ids,
    :149 and :395, only decides among alternative optima and the order of pivots)."""
    tol = problem.tolerance if tolerance is None else tolerance
    m = problem.m
    lower = problem.lower
    finite = problem.capacity >= 0
    cap = np.full(m, -1, dtype=np.int64)
    width = problem.capacity - lower
    if (finite & (width < 0)).any():
        i = int(np.nonzero(finite & (width < 0))[0][0])
        raise InvalidProblemError(
            f"Arc capacity ({problem.capacity[i]}) is less than lower bound ({lower[i]}) for arc "
            f"{int(problem.tail[i]) + 1} -> {int(problem.head[i]) + 1}. Capacity must be >= lower bound.")
    cap[finite] = width[finite]
    supply = problem.supply.copy()
    if lower.any():
        np.subtract.at(supply, problem.tail, lower)
        np.add.at(supply, problem.head, lower)
    if abs(int(supply.sum())) > tol:
        raise InvalidProblemError(
            f"Supplies do not balance after lower-bound adjustment: total supply {float(supply.sum()):.6f} "
            f"exceeds tolerance {tol}.")
    if m and (np.abs(problem.cost).max() >= 2 ** 31 or cap.max() >= 2 ** 60):
        raise SolverConfigurationError("costs must fit int32 and capacities int60")
    return FlatProblem(_IdSeq(problem.n), _KeySeq(problem.tail, problem.head), problem.tail, problem.head, problem.cost,
                       cap, supply, lower.astype(np.float64), problem.cost.astype(np.float64), 1, 1, soa=True)


def _decimal_scale(values: np.ndarray, what: str) -> int:
    """Smallest power of ten that makes every value an integer (exactly, up to 1e-9 relative)."""
    if values.size == 0:
        return 1
    if not np.all(np.isfinite(values)):
        raise InvalidProblemError(f"{what} must be finite numbers")
    for k in range(_MAX_DECIMALS + 1):
        scaled = values * (10.0 ** k)
        if np.all(np.abs(scaled - np.round(scaled)) <= 1e-9 * np.maximum(1.0, np.abs(scaled))):
            return 10 ** k
    raise SolverConfigurationError(
        f"{what} need more than {_MAX_DECIMALS} decimal digits; the integer MI355X engine cannot "
        f"represent them exactly")


def flatten_problem(problem: NetworkProblem, tolerance: float | None = None) -> FlatProblem:
    """NetworkProblem -> integer SoA, in the reference's internal order.  ``tolerance`` is the solver's
    (``SolverOptions.tolerance``, simplex.py:154): the balance and bound checks below are the solver's own
    (:381-412), not the problem's build-time ones."""
    node_ids = sorted(problem.nodes.keys())                       # simplex.py:149
    index = {nid: i for i, nid in enumerate(node_ids)}
    arcs = sorted(problem.undirected_expansion(), key=lambda a: (a.tail, a.head))  # simplex.py:394-395
    m = len(arcs)
    tol = problem.tolerance if tolerance is None else tolerance
    supply = np.array([problem.nodes[nid].supply for nid in node_ids], dtype=np.float64)
    if abs(float(supply.sum())) > tol:                            # simplex.py:381-390
        raise InvalidProblemError(
            f"Supplies do not balance after lower-bound adjustment: total supply {supply.sum():.6f} "
            f"exceeds tolerance {tol}.")
    tail = np.fromiter((index[a.tail] for a in arcs), dtype=np.int32, count=m)
    head = np.fromiter((index[a.head] for a in arcs), dtype=np.int32, count=m)
    cost = np.fromiter((a.cost for a in arcs), dtype=np.float64, count=m)
    lower = np.fromiter((a.lower for a in arcs), dtype=np.float64, count=m)
    upper = np.empty(m, dtype=np.float64)
    for i, a in enumerate(arcs):                                  # simplex.py:399-412
        if a.capacity is None:
            upper[i] = math.inf
        else:
            u = float(a.capacity) - a.lower
            if u < -tol:
                raise InvalidProblemError(
                    f"Arc capacity ({a.capacity}) is less than lower bound ({a.lower}) for arc "
                    f"{a.tail} -> {a.head}. Capacity must be >= lower bound.")
            upper[i] = max(0.0, u)
    np.subtract.at(supply, tail, lower)                           # simplex.py:413-415
    np.add.at(supply, head, lower)
    finite = np.isfinite(upper)
    flow_scale = _decimal_scale(np.concatenate((supply, upper[finite], lower)), "supplies / capacities / lower bounds")
    cost_scale = _decimal_scale(cost, "costs")
    cap_i = np.full(m, -1, dtype=np.int64)
    cap_i[finite] = np.round(upper[finite] * flow_scale).astype(np.int64)
    supply_i = np.round(supply * flow_scale).astype(np.int64)
    residual = int(supply_i.sum())
    if residual != 0:
        # the reference tolerates |sum| <= tolerance (checked above); the integer engine needs an exact balance:
        # the sub-tolerance remainder goes onto the largest node -- never more than the tolerance allows
        if abs(residual) > tol * flow_scale + 1:
            raise InvalidProblemError(
                f"Supplies do not balance after lower-bound adjustment: total supply {residual / flow_scale:.6f} "
                f"exceeds tolerance {tol}.")
        supply_i[int(np.argmax(np.abs(supply_i)))] -= residual
    cost_i = np.round(cost * cost_scale).astype(np.int64)
    if m and (np.abs(cost_i).max() >= 2 ** 31 or (cap_i.max() >= 2 ** 60)):
        raise SolverConfigurationError("scaled costs must fit int32 and scaled capacities int60")
    return FlatProblem(node_ids, [(a.tail, a.head) for a in arcs], tail, head, cost_i, cap_i, supply_i, lower,
                       cost, flow_scale, cost_scale)


def map_cost_changes(flat: FlatProblem, changes, tolerance: float) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Cost changes in the caller's terms -> ``(arc indices, integer engine costs, costs in caller units)`` in ``flat``'s arc
    order, one entry per changed arc.  Pure: neither ``flat`` nor ``changes`` is modified.

    * object-model problems: ``changes`` maps ``(tail id, head id)`` to the new cost.  Of parallel arcs with one key the
      LAST index takes it, like the key -> index map of a warm start (``_apply_warm_start_basis``); a key the problem does
      not have is an ``InvalidProblemError``.
    * ``SoAProblem``: ``changes`` is a pair ``(indices, costs)`` of arrays in the problem's arc order; of duplicate indices
      the last entry wins.

    Every new cost has to be an integer at ``flat.cost_scale`` (the decimal scaling chosen when the problem was flattened)
    to within ``tolerance`` in the caller's units -- the engine is integer and the scale of the resident instance is fixed --
    and fit int32 after scaling; otherwise ``InvalidProblemError`` / ``SolverConfigurationError``, and nothing is returned."""
    m = len(flat.keys)
    if flat.soa:
        try:
            if hasattr(changes, "items"):
                raise TypeError
            idx_in, cost_in = changes
        except (TypeError, ValueError):
            raise InvalidProblemError("cost changes of an SoAProblem are a pair (indices, costs) of arrays") from None
        idx = np.asarray(idx_in).reshape(-1)
        values = np.asarray(cost_in, dtype=np.float64).reshape(-1)
        if idx.shape[0] != values.shape[0]:
            raise InvalidProblemError("cost changes: indices and costs differ in length")
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise InvalidProblemError("cost changes: arc indices must be integers")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= m):
            raise InvalidProblemError(f"cost changes: arc index outside [0, {m})")
        # the last entry of every index wins
        _, first_rev = np.unique(idx[::-1], return_index=True)
        keep = np.sort(idx.shape[0] - 1 - first_rev)
        idx, values = idx[keep], values[keep]
    else:
        if not hasattr(changes, "items"):
            raise InvalidProblemError("cost changes are a mapping {(tail, head): cost}")
        last: dict[tuple[str, str], int] = {}
        for i, key in enumerate(flat.keys):
            last[key] = i
        picked: dict[int, float] = {}
        for key, value in changes.items():
            i = last.get(tuple(key))
            if i is None:
                raise InvalidProblemError(f"cost change names arc {tuple(key)} which is not in the problem")
            picked[i] = float(value)
        idx = np.fromiter(picked.keys(), dtype=np.int64, count=len(picked))
        values = np.fromiter(picked.values(), dtype=np.float64, count=len(picked))
    if values.size and not np.all(np.isfinite(values)):
        raise InvalidProblemError("costs must be finite numbers")
    scaled = values * float(flat.cost_scale)
    rounded = np.round(scaled)
    off = np.abs(scaled - rounded) > tolerance * flat.cost_scale
    if off.any():
        i = int(np.nonzero(off)[0][0])
        raise InvalidProblemError(
            f"new cost {values[i]} of arc {flat.keys[int(idx[i])]} is not a multiple of 1/{flat.cost_scale}, the cost "
            f"resolution this solver was built with; build a new solver for finer costs")
    if rounded.size and np.abs(rounded).max() >= 2 ** 31:
        raise SolverConfigurationError("scaled costs must fit int32")
    return idx, rounded.astype(np.int64), values


def map_rhs_changes(flat: FlatProblem, supplies, capacities, tolerance: float):
    """Supply and capacity changes in the caller's terms -> ``(node indices, integer engine supplies, supplies in caller
    units, arc indices, integer engine capacities (-1: none), capacities in caller units (nan: none))`` in ``flat``'s
    orders.  Pure: neither ``flat`` nor the changes are modified.  Either argument may be ``None``.

    * object-model problems: ``supplies`` maps node id to the new supply, ``capacities`` maps ``(tail id, head id)`` to the
      new capacity or ``None`` (of parallel arcs the LAST index takes it, as in ``map_cost_changes``).
    * ``SoAProblem``: pairs ``(indices, values)`` of arrays; a negative capacity means none; of duplicates the last wins.

    The resident instance keeps its ``flow_scale`` and its lower-bound shift (simplex.py:403-428): the engine's supply of a
    node is ``(supply + shift) * flow_scale`` with the node's shift unchanged, the engine's capacity ``(capacity - lower) *
    flow_scale``.  A value that is not an integer at that scale (to within ``tolerance``), a capacity below the arc's lower
    bound or a supply vector that no longer balances is an ``InvalidProblemError`` with the reference's wording, and nothing
    is returned."""
    n, m = len(flat.node_ids), len(flat.keys)
    scale = float(flat.flow_scale)

    def pairs(changes, what, count):
        try:
            if hasattr(changes, "items"):
                raise TypeError
            idx_in, val_in = changes
        except (TypeError, ValueError):
            raise InvalidProblemError(f"{what} changes of an SoAProblem are a pair (indices, values) of arrays") from None
        idx = np.asarray(idx_in).reshape(-1)
        values = np.asarray(val_in, dtype=np.float64).reshape(-1)
        if idx.shape[0] != values.shape[0]:
            raise InvalidProblemError(f"{what} changes: indices and values differ in length")
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise InvalidProblemError(f"{what} changes: indices must be integers")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= count):
            raise InvalidProblemError(f"{what} changes: index outside [0, {count})")
        _, first_rev = np.unique(idx[::-1], return_index=True)      # the last entry of every index wins
        keep = np.sort(idx.shape[0] - 1 - first_rev)
        return idx[keep], values[keep]

    def to_int(values, what, names):
        if values.size and not np.all(np.isfinite(values)):
            raise InvalidProblemError(f"{what} must be finite numbers")
        scaled = values * scale
        rounded = np.round(scaled)
        off = np.abs(scaled - rounded) > tolerance * scale
        if off.any():
            i = int(np.nonzero(off)[0][0])
            raise InvalidProblemError(
                f"new {what} of {names(i)} is not a multiple of 1/{flat.flow_scale}, the flow resolution this solver was "
                f"built with; build a new solver for finer values")
        if rounded.size and np.abs(rounded).max() >= 2 ** 60:
            raise SolverConfigurationError("scaled supplies / capacities must stay below 2^60")
        return rounded.astype(np.int64)

    empty_i, empty_f = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
    # ---- supplies
    if supplies is None:
        s_idx, s_val = empty_i, empty_f
    elif flat.soa:
        s_idx, s_val = pairs(supplies, "supply", n)
    else:
        if not hasattr(supplies, "items"):
            raise InvalidProblemError("supply changes are a mapping {node id: supply}")
        index = {nid: i for i, nid in enumerate(flat.node_ids)}
        for nid in supplies:
            if nid not in index:
                raise InvalidProblemError(f"supply change names node {nid!r} which is not in the problem")
        s_idx = np.fromiter((index[nid] for nid in supplies), dtype=np.int64, count=len(supplies))
        s_val = np.fromiter((float(v) for v in supplies.values()), dtype=np.float64, count=len(supplies))
    shift = np.zeros(n, dtype=np.float64)                           # simplex.py:413-415, per node
    if m and flat.lower.any():
        np.subtract.at(shift, flat.tail, flat.lower)
        np.add.at(shift, flat.head, flat.lower)
    s_int = to_int(s_val + shift[s_idx], "supply", lambda i: f"node {flat.node_ids[int(s_idx[i])]}")
    if s_idx.size:
        new_supply = flat.supply.copy()
        new_supply[s_idx] = s_int
        residual = sum(int(x) for x in new_supply.tolist())
        if residual != 0:
            raise InvalidProblemError(
                f"Supplies do not balance after lower-bound adjustment: total supply {residual / flat.flow_scale:.6f} "
                f"exceeds tolerance {tolerance}.")
    # ---- capacities
    if capacities is None:
        c_idx, c_val = empty_i, empty_f
    elif flat.soa:
        c_idx, c_val = pairs(capacities, "capacity", m)
        c_val = np.where(c_val < 0, np.nan, c_val)
    else:
        if not hasattr(capacities, "items"):
            raise InvalidProblemError("capacity changes are a mapping {(tail, head): capacity or None}")
        last: dict[tuple[str, str], int] = {}
        for i, key in enumerate(flat.keys):
            last[key] = i
        picked: dict[int, float] = {}
        for key, value in capacities.items():
            i = last.get(tuple(key))
            if i is None:
                raise InvalidProblemError(f"capacity change names arc {tuple(key)} which is not in the problem")
            picked[i] = math.nan if value is None else float(value)
        c_idx = np.fromiter(picked.keys(), dtype=np.int64, count=len(picked))
        c_val = np.fromiter(picked.values(), dtype=np.float64, count=len(picked))
    none = np.isnan(c_val)
    if np.isinf(c_val).any():
        raise InvalidProblemError("capacities must be finite numbers or None")
    width = np.where(none, 0.0, c_val - flat.lower[c_idx])
    low = width < -tolerance
    if low.any():
        i = int(np.nonzero(low)[0][0])
        t, h = flat.keys[int(c_idx[i])]
        raise InvalidProblemError(
            f"Arc capacity ({c_val[i]:g}) is less than lower bound ({flat.lower[int(c_idx[i])]:g}) for arc "
            f"{t} -> {h}. Capacity must be >= lower bound.")
    c_int = to_int(np.maximum(width, 0.0), "capacity", lambda i: f"arc {flat.keys[int(c_idx[i])]}")
    c_int[none] = -1
    return s_idx, s_int, s_val, c_idx, c_int, c_val


SCENARIO_KEYS = ("costs", "supplies", "capacities")


def map_scenario(flat: FlatProblem, scenario, tolerance: float) -> dict:
    """One what-if scenario -> the integer edit arrays of its parts.  ``scenario`` is a mapping with any of ``costs``,
    ``supplies``, ``capacities``, each in the format of the matching ``NetworkSimplex.update_*`` method (``map_cost_changes``,
    ``map_rhs_changes``); an empty scenario is an empty cost change.  Returns ``{"costs": map_cost_changes(...) or None,
    "supplies": map_rhs_changes(flat, supplies, None, ...) or None, "capacities": map_rhs_changes(flat, None, capacities, ...)
    or None}``.  Pure, no device: an unknown key or an invalid edit raises ``InvalidProblemError`` and nothing is returned."""
    if not hasattr(scenario, "keys"):
        raise InvalidProblemError("a scenario is a mapping with any of 'costs', 'supplies', 'capacities'")
    unknown = [k for k in scenario.keys() if k not in SCENARIO_KEYS]
    if unknown:
        raise InvalidProblemError(f"scenario has unknown key {unknown[0]!r}; known: {', '.join(SCENARIO_KEYS)}")
    out = {"costs": None, "supplies": None, "capacities": None}
    if scenario.get("costs") is not None:
        out["costs"] = map_cost_changes(flat, scenario["costs"], tolerance)
    if scenario.get("supplies") is not None:
        out["supplies"] = map_rhs_changes(flat, scenario["supplies"], None, tolerance)
    if scenario.get("capacities") is not None:
        out["capacities"] = map_rhs_changes(flat, None, scenario["capacities"], tolerance)
    return out


def map_arc_additions(flat: FlatProblem, arcs, tolerance: float, directed: bool = True) -> dict:
    """New arcs in the caller's terms -> the engine's arrays, by flatten's own per-arc transformation: cost and flow scales of
    the resident instance, the lower-bound shift (simplex.py:403-428), the undirected expansion (data.py:162-223).  Pure:
    neither ``flat`` nor ``arcs`` is modified.

    * object-model problems: ``arcs`` is an iterable of the dicts ``build_problem`` takes (``tail``, ``head``, ``capacity``,
      ``cost``, ``lower``); with ``directed=False`` every one is an undirected edge.
    * ``SoAProblem``: ``arcs`` is ``(tail, head, cost, capacity[, lower])`` of integer arrays, 0-based nodes, a negative
      capacity meaning none.

    Returns ``tail`` / ``head`` (int32 node indices), ``cost`` / ``cap`` (int64, engine units; cap -1 = none), ``lower`` and
    ``orig_cost`` (caller units), ``keys`` (tail id, head id) and ``supply_nodes`` / ``supply_values``: the nodes whose engine
    supply the new lower bounds shift, with their new engine supplies.  Refusals carry the reference's wording where it has
    one (capacity below lower bound, unknown node, self-loop), and the "not a multiple of 1/..." message of the other update
    calls for a value off the instance's scale; nothing is returned then."""
    n = len(flat.node_ids)
    if flat.soa:
        try:
            if hasattr(arcs, "items") or not 4 <= len(arcs) <= 5:
                raise TypeError
            parts = [np.asarray(a).reshape(-1) for a in arcs]
        except TypeError:
            raise InvalidProblemError("new arcs of an SoAProblem are (tail, head, cost, capacity[, lower]) arrays") from None
        k = parts[0].shape[0]
        if any(a.shape[0] != k for a in parts):
            raise InvalidProblemError("Arc arrays differ in length.")
        if k and not all(np.issubdtype(a.dtype, np.integer) for a in parts):
            raise InvalidProblemError("new arcs of an SoAProblem are integer arrays")
        tail, head, cost, capacity = (a.astype(np.int64) for a in parts[:4])
        lower = parts[4].astype(np.int64) if len(parts) == 5 else np.zeros(k, dtype=np.int64)
        bad = (tail < 0) | (tail >= n) | (head < 0) | (head >= n)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise InvalidProblemError(f"Arc tail '{int(tail[i]) + 1}' or head '{int(head[i]) + 1}' not found in node set. "
                                      f"All arc endpoints must reference existing nodes.")
        if (tail == head).any():
            i = int(np.nonzero(tail == head)[0][0])
            raise InvalidProblemError(f"Self-loop detected on node '{int(tail[i]) + 1}'. Self-loops are not supported in network simplex.")
        finite = capacity >= 0
        width = capacity - lower
        if (finite & (width < 0)).any():
            i = int(np.nonzero(finite & (width < 0))[0][0])
            raise InvalidProblemError(f"Arc capacity ({capacity[i]}) is less than lower bound ({lower[i]}) for arc "
                                      f"{int(tail[i]) + 1} -> {int(head[i]) + 1}. Capacity must be >= lower bound.")
        if k and (np.abs(cost).max() >= 2 ** 31 or width[finite].max(initial=0) >= 2 ** 60):
            raise SolverConfigurationError("costs must fit int32 and capacities int60")
        cap_i = np.where(finite, width, -1).astype(np.int64)
        cost_i, lower_f, cost_f, shift_i = cost, lower.astype(np.float64), cost.astype(np.float64), lower
        keys = [(str(int(t) + 1), str(int(h) + 1)) for t, h in zip(tail.tolist(), head.tolist())]
    else:
        from .data import Arc
        index = {nid: i for i, nid in enumerate(flat.node_ids)}
        made = []
        for a in arcs:
            cap = a.get("capacity")
            arc = Arc(tail=str(a["tail"]), head=str(a["head"]), capacity=None if cap is None else float(cap),
                      cost=float(a.get("cost", 0.0)), lower=float(a.get("lower", 0.0)))       # (refuses self-loops and capacity < lower)
            for end, label in ((arc.tail, "tail"), (arc.head, "head")):
                if end not in index:
                    raise InvalidProblemError(f"Arc {label} '{end}' not found in node set. All arc endpoints must reference "
                                              f"existing nodes.")
            if not directed:                                           # data.py:162-223
                if arc.capacity is None:
                    raise InvalidProblemError(f"Undirected edge {arc.tail} -- {arc.head} has infinite capacity. Undirected graphs "
                                              f"require finite capacity on all edges.")
                c = float(arc.capacity)
                if abs(arc.lower) > 1e-12 and not math.isclose(arc.lower, -c, rel_tol=0.0, abs_tol=1e-12):
                    raise InvalidProblemError(f"Undirected edge {arc.tail} -- {arc.head} has custom lower bound ({arc.lower}). "
                                              f"Undirected edges do not support custom lower bounds.")
                arc = Arc(tail=arc.tail, head=arc.head, capacity=c, cost=arc.cost, lower=-c)
            made.append(arc)
        k = len(made)
        keys = [(a.tail, a.head) for a in made]
        tail = np.fromiter((index[a.tail] for a in made), dtype=np.int64, count=k)
        head = np.fromiter((index[a.head] for a in made), dtype=np.int64, count=k)
        cost_f = np.fromiter((a.cost for a in made), dtype=np.float64, count=k)
        lower_f = np.fromiter((a.lower for a in made), dtype=np.float64, count=k)
        upper = np.full(k, math.inf)
        for i, a in enumerate(made):                                   # simplex.py:399-412
            if a.capacity is not None:
                u = float(a.capacity) - a.lower
                if u < -tolerance:
                    raise InvalidProblemError(f"Arc capacity ({a.capacity}) is less than lower bound ({a.lower}) for arc "
                                              f"{a.tail} -> {a.head}. Capacity must be >= lower bound.")
                upper[i] = max(0.0, u)
        if not (np.all(np.isfinite(cost_f)) and np.all(np.isfinite(lower_f)) and not np.isnan(upper).any()):
            raise InvalidProblemError("costs, capacities and lower bounds must be finite numbers")

        def to_int(values, scale, what, unit):
            scaled = values * float(scale)
            rounded = np.round(scaled)
            off = np.abs(scaled - rounded) > tolerance * scale
            if off.any():
                i = int(np.nonzero(off)[0][0])
                raise InvalidProblemError(f"new {what} {values[i]} of arc {keys[i]} is not a multiple of 1/{scale}, the {unit} "
                                          f"resolution this solver was built with; build a new solver for finer {what}s")
            return rounded.astype(np.int64)

        cost_i = to_int(cost_f, flat.cost_scale, "cost", "cost")
        finite = np.isfinite(upper)
        cap_i = np.full(k, -1, dtype=np.int64)
        cap_i[finite] = to_int(upper[finite], flat.flow_scale, "capacity", "flow") if finite.any() else 0
        shift_i = to_int(lower_f, flat.flow_scale, "lower bound", "flow")
        if k and (np.abs(cost_i).max() >= 2 ** 31 or cap_i.max() >= 2 ** 60):
            raise SolverConfigurationError("scaled costs must fit int32 and scaled capacities int60")
    # the lower-bound shift of the supplies (simplex.py:413-415), per node
    delta = np.zeros(n, dtype=np.int64)
    if k and shift_i.any():
        np.subtract.at(delta, tail, shift_i)
        np.add.at(delta, head, shift_i)
    nodes = np.nonzero(delta)[0].astype(np.int64)
    return {"tail": tail.astype(np.int32), "head": head.astype(np.int32), "cost": cost_i.astype(np.int64), "cap": cap_i,
            "lower": lower_f, "orig_cost": cost_f, "keys": keys, "supply_nodes": nodes,
            "supply_values": (flat.supply[nodes] + delta[nodes]).astype(np.int64)}


@dataclass
class Certificate:
    """What ``NetworkSimplex.certify()`` returns; ``raw`` holds every field of ``mcf_certificate``."""

    verdict: str                     # "optimal" / "infeasible" / "not_proven": what the evidence proves (see certify() on "infeasible")
    status: str                      # the handle's solve status ("running" before a solve)
    proves_status: bool
    primal_objective: int            # exact, in flow_scale x cost_scale units
    big_m_term: int
    dual_objective: int
    gap: int
    artificial_flow: int
    flow_scale: int
    cost_scale: int
    bound_violations: int
    worst_bound_arc: tuple[str, str] | None
    imbalanced_nodes: int
    worst_imbalance_node: str | None
    dual_violations: int
    worst_dual_arc: tuple[str, str] | None
    basis_inconsistencies: int
    raw: dict


class NetworkSimplex:
    """Network simplex solver for minimum-cost flow, pivoting on an MI355X.

    Same construction and ``solve`` contract as the reference class
    (simplex.py:62-265, :1446-1765).  ``SolverOptions.pricing_strategy``:
    ``"dantzig"`` selects the full-scan pricing kernel, ``"devex"`` the block-search Devex
    kernel, ``"candidate_list"`` and ``"adaptive"`` (which the reference starts as a candidate
    list, simplex_pricing.py:545-587) the candidate-list rule: a full sweep keeps one candidate
    per pricing workgroup and the following pivots re-price only that list.  All rules reach the
    same optimum.
    """

    ROOT_NODE = "__network_simplex_root__"

    def __init__(self, problem: NetworkProblem, options: SolverOptions | None = None, *, device: int = -1,
                 batch_pivots: int = 64, use_graph: bool = True, engine_options: dict | None = None):
        self.options = options if options is not None else SolverOptions()
        self.logger = logging.getLogger(__name__)
        self.problem = problem
        self.tolerance = self.options.tolerance
        self.flat = (flatten_soa(problem, self.tolerance) if isinstance(problem, SoAProblem)
                     else flatten_problem(problem, self.tolerance))
        self.node_ids = [self.ROOT_NODE] + self.flat.node_ids if not self.flat.soa else self.flat.node_ids
        self.actual_arc_count = len(self.flat.keys)
        self.degenerate_pivots = 0
        strategy = self._select_pricing_strategy()
        self.pricing_rule = {"dantzig": _engine.RULE_DANTZIG, "devex": _engine.RULE_DEVEX_BLOCK}.get(
            strategy, _engine.RULE_CANDIDATE_LIST)  # candidate_list and adaptive (which starts as one)
        # simplex.py:133-137, 259-261 + specialized_pivots.py:452-527: structured instances get the reference's
        # specialised entering rule, as a variant of the same sweep kernel
        self.network_structure = analyze_network_structure(problem)
        special = entering_rule_options(self.network_structure, self.flat.node_ids, self.flat.tail, self.flat.head, self.flat.supply,
                                        unit=self.flat.flow_scale)
        if special is not None:
            # the reference tries the specialised scan first and falls back to the configured strategy when it finds nothing
            # (simplex.py:1060-1064); here the specialised rule IS a key variant of one sweep, so it replaces the strategy
            # for the whole solve -- status and objective are the same, iteration counts need not be
            if self.options.explicit_pricing_strategy and strategy != "dantzig":
                self.logger.info(f"pricing_strategy={strategy!r} is overridden by the specialised rule of this network class")
            self.pricing_rule = special.pop("rule")
            self.logger.info(f"Using specialized pivot strategy for {self.network_structure.network_type.value}")
        bs = self.options.block_size
        block_size = 0 if bs is None or isinstance(bs, str) else int(bs)
        self._engine_kwargs = dict(rule=self.pricing_rule, block_size=block_size, batch_pivots=batch_pivots, use_graph=use_graph,
                                   device=device, **(special or {}), **(engine_options or {}))
        self._arc_order_map = None   # flat arc j -> index into problem.arcs, once add_arcs has appended arcs (None: flatten's sort)
        self.engine = _engine.McfEngine(
            len(self.flat.node_ids), self.flat.tail, self.flat.head, self.flat.cost, self.flat.cap,
            self.flat.supply, **self._engine_kwargs)
        self.stats: dict = {}
        self._pivots_seen = 0   # the engine's cumulative pivot count when the last solve() returned

    # simplex.py:314-374: the reference's grid-on-torus heuristic switches to Dantzig unless the
    # caller pinned a strategy
    def _select_pricing_strategy(self) -> str:
        if self.options.explicit_pricing_strategy:
            return self.options.pricing_strategy
        m = self.actual_arc_count
        if self.flat.soa:
            n = len(self.flat.node_ids)
            non_transship = int(np.count_nonzero(self.problem.supply))
        else:
            nodes = self.problem.nodes
            n = len(nodes)
            non_transship = sum(1 for nd in nodes.values() if abs(nd.supply) > self.tolerance)
        if n == 0:
            return self.options.pricing_strategy
        if (non_transship <= 4 and (n - non_transship) / n > 0.98 and (2 * m) / n >= 8 and 6 <= m / n <= 12):
            self.logger.info("Auto-detected grid-on-torus structure, switching to Dantzig pricing")
            return "dantzig"
        return self.options.pricing_strategy

    def _apply_warm_start_basis(self, basis: Basis) -> bool:
        """simplex.py:740-903: map the basis' (tail, head) keys onto arcs and hand them to the engine
        (``mcf_set_basis``), which adds one artificial arc per uncovered component and recomputes the tree
        flows from conservation (:905-1010).  False -> the engine is at the cold start (the reference's
        fall-back).  ``Basis.arc_flows`` entries of arcs OUTSIDE ``tree_arcs`` (this build's results carry the
        non-basic arcs that sit at capacity there; the reference ignores such keys) tell the engine which
        non-basic arcs start at their upper bound."""
        f = self.flat
        if isinstance(basis, ArrayBasis):                          # flat arrays in this problem's arc order
            if basis.in_tree.shape[0] != len(f.keys):
                self.logger.warning("Warm-start basis does not match the problem's arc count. Falling back to cold start.")
                return False
            if not basis.in_tree.any():
                self.logger.warning("Warm-start basis is empty. Falling back to cold start.")
                return False
            self._pivots_seen = 0                                  # (mcf_set_basis resets the engine's counters either way)
            if self.engine.set_basis(basis.in_tree, basis.at_upper):
                self.logger.info(f"Successfully applied warm-start basis with {int(basis.in_tree.sum())} basis arcs")
                return True
            self.logger.warning(f"{self.engine.last_error()}. Falling back to cold start.")
            return False
        if len(basis.tree_arcs) == 0:
            self.logger.warning("Warm-start basis is empty. Falling back to cold start.")
            return False
        by_key: dict[tuple[str, str], list[int]] = {}
        for i, key in enumerate(f.keys):
            by_key.setdefault(key, []).append(i)
        in_tree = np.zeros(len(f.keys), dtype=np.int8)
        for key in basis.tree_arcs:
            idxs = by_key.get(tuple(key))
            if not idxs:
                self.logger.warning(f"Warm-start basis contains arc {key} not in current problem. "
                                    "Falling back to cold start.")
                return False
            in_tree[idxs[-1]] = 1                                  # like the reference's key -> index dict (:763-766)
        at_upper = np.zeros(len(f.keys), dtype=np.int8)
        for key, value in basis.arc_flows.items():
            idxs = by_key.get(tuple(key))
            if not idxs or tuple(key) in basis.tree_arcs:
                continue
            i = idxs[-1]
            if f.cap[i] > 0 and round(float(value) * f.flow_scale) >= f.cap[i]:
                at_upper[i] = 1
        self._pivots_seen = 0
        if self.engine.set_basis(in_tree, at_upper):
            self.logger.info(f"Successfully applied warm-start basis with {int(in_tree.sum())} basis arcs")
            return True
        self.logger.warning(f"{self.engine.last_error()}. Falling back to cold start.")
        return False

    def fork(self, count: int = 1) -> list["NetworkSimplex"]:
        """``count`` solvers on forked engines (``mcf_fork``): each holds a complete copy of this solver's resident state, made on
        the device, and goes on exactly as this one would -- edit and re-solve it without touching this one.  ``flat``,
        ``problem`` and the maps are shared by reference (the update methods replace them, they never mutate them); the next
        ``solve()`` of a fork reports the pivots of that call.  Close a fork's engine when done (``fork.engine.close()``)."""
        out = []
        for eng in self.engine.fork(count):
            sv = copy.copy(self)
            sv.engine = eng
            sv.stats = dict(self.stats)
            sv._engine_kwargs = dict(self._engine_kwargs)
            out.append(sv)
        return out

    def update_costs(self, changes) -> int:
        """Change arc costs and keep the solved state: the basis that is resident on the device stays, its potentials and
        reduced costs are brought in line with the new costs there (``mcf_update_costs``), and the next ``solve()`` goes on
        pivoting from it -- no new solver, no upload, no warm-start hand-over.  ``changes``: ``{(tail, head): cost}`` for
        an object-model problem, ``(indices, costs)`` for an ``SoAProblem`` (see ``map_cost_changes``; on an invalid
        change nothing is changed).  The caller's problem object is left alone: ``self.problem`` becomes an updated copy.
        Returns the number of arcs whose cost was set."""
        f = self.flat
        idx, cost_i, cost_f = map_cost_changes(f, changes, self.tolerance)
        self.engine.update_costs(idx, cost_i)
        new_cost = f.cost.copy()
        new_cost[idx] = cost_i
        if f.soa:
            problem = copy.copy(self.problem)
            problem.cost = new_cost
            problem._arcs = None
            self.problem = problem
            self.flat = replace(f, cost=new_cost, orig_cost=new_cost.astype(np.float64))
        else:
            orig_cost = f.orig_cost.copy()
            orig_cost[idx] = cost_f
            arcs = list(self.problem.arcs)
            order = self._arc_order()
            for j, c in zip(idx.tolist(), cost_f.tolist()):
                arcs[order[j]] = replace(arcs[order[j]], cost=c)
            self.problem = replace(self.problem, nodes=dict(self.problem.nodes), arcs=arcs)
            self.flat = replace(f, cost=new_cost, orig_cost=orig_cost)
        return int(idx.shape[0])

    def cost_ranges(self, keys=None):
        """Cost ranging on the basis resident on the device (``mcf_cost_ranges``): for every arc, the interval its cost may move
        in -- this arc alone, all others as they are -- without the basis ceasing to be optimal, so that ``update_costs`` with
        a cost inside it followed by ``solve()`` makes no pivot.  Computed for all arcs at once on the device; nothing is
        re-solved.  Meaningful after a ``solve()`` that ended "optimal"; on any other state the intervals describe that
        state's basis and may be empty (``lowest > highest``).  The intervals hold as long as the new cost does not raise the
        engine's big-M (a cost far above every cost of the problem does).

        * object-model problems: ``keys`` = ``(tail, head)`` keys (default: all; of parallel arcs the LAST one, as in
          ``update_costs``); returns ``{(tail, head): (lowest_cost, highest_cost)}`` in the caller's cost units, ``None`` for an
          unbounded end.
        * ``SoAProblem``: ``keys`` = arc indices (default: all, duplicates allowed); returns ``(lowest, highest)`` arrays in the
          order asked.  An unscaled instance -- an ``SoAProblem`` always is -- gets the exact integers, int64, with
          ``-engine.RANGE_INF`` / ``engine.RANGE_INF`` for an unbounded end; a scaled one floats with -inf / +inf."""
        f = self.flat
        m = len(f.keys)
        if f.soa:
            idx = None
            if keys is not None:
                idx = np.asarray(keys).reshape(-1)
                if idx.size and not np.issubdtype(idx.dtype, np.integer):
                    raise InvalidProblemError("cost ranges: arc indices must be integers")
                idx = idx.astype(np.int64)
                if idx.size and (idx.min() < 0 or idx.max() >= m):
                    raise InvalidProblemError(f"cost ranges: arc index outside [0, {m})")
        else:
            last: dict[tuple[str, str], int] = {}
            for i, key in enumerate(f.keys):
                last[key] = i
            wanted = list(last) if keys is None else [tuple(k) for k in keys]
            missing = [k for k in wanted if k not in last]
            if missing:
                raise InvalidProblemError(f"cost range asked for arc {missing[0]} which is not in the problem")
            idx = np.fromiter((last[k] for k in wanted), dtype=np.int64, count=len(wanted))
        down, up, _ = self.engine.cost_ranges(idx)
        cost = f.cost if idx is None else f.cost[idx]
        inf = _engine.RANGE_INF
        if f.soa:
            lowest = np.where(down == inf, -inf, cost - np.where(down == inf, 0, down))
            highest = np.where(up == inf, inf, cost + np.where(up == inf, 0, up))
            if f.cost_scale == 1:
                return lowest, highest
            return (np.where(down == inf, -np.inf, lowest / f.cost_scale), np.where(up == inf, np.inf, highest / f.cost_scale))
        scale = f.cost_scale
        out = {}
        for k, c, d, u in zip(wanted, cost.tolist(), down.tolist(), up.tolist()):
            out[k] = (None if d == inf else (c - d) / scale, None if u == inf else (c + u) / scale)
        return out

    def _arc_name(self, index: int):
        """A caller's arc index of the engine as the caller names it: a key, ``("artificial", node id)``, ``None`` for -1."""
        f = self.flat
        if index < 0:
            return None
        m = len(f.keys)
        return f.keys[index] if index < m else ("artificial", f.node_ids[index - m])

    def supply_ranges(self, pairs):
        """Supply ranging on the basis resident on the device (``mcf_supply_ranges``): for every pair ``(a, b)``, how far the
        shift ``supply[a] += d, supply[b] -= d`` can go -- this shift alone -- before a tree flow reaches a bound, and what
        the objective does until then.  ``update_supplies`` with a shift below the limit keeps the basis, and the ``solve()``
        after it makes no pivot; the objective moves by exactly ``rate * d``.  All pairs are answered at once on the device;
        nothing is re-solved.  Meaningful after a ``solve()`` that ended "optimal".

        * object-model problems: ``pairs`` = ``(from id, to id)`` tuples; returns a list of ``SupplyRange`` in the caller's
          flow and cost units.
        * ``SoAProblem``: ``pairs`` = ``(from indices, to indices)``; returns ``(limit, rate, limit_arc,
          creates_artificial_flow)`` arrays: exact int64, ``engine.RANGE_INF`` for no limit, ``limit_arc`` an arc index,
          ``m + v`` for the artificial arc of node ``v``, -1 for none."""
        f = self.flat
        n = len(f.node_ids)
        if f.soa:
            try:
                src, dst = pairs
            except (TypeError, ValueError):
                raise InvalidProblemError("supply ranges of an SoAProblem take a pair (from indices, to indices) of arrays") from None
            src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
            if src.shape != dst.shape:
                raise InvalidProblemError("supply ranges: from and to differ in length")
            for idx in (src, dst):
                if idx.size and not np.issubdtype(idx.dtype, np.integer):
                    raise InvalidProblemError("supply ranges: node indices must be integers")
                if idx.size and (idx.min() < 0 or idx.max() >= n):
                    raise InvalidProblemError(f"supply ranges: node index outside [0, {n})")
            limit, arc, rate, rising, _ = self.engine.supply_ranges(src, dst)
            return limit, rate, arc, rising > 0
        index = {nid: i for i, nid in enumerate(f.node_ids)}
        pairs = [tuple(p) for p in pairs]
        for p in pairs:
            for nid in p:
                if nid not in index:
                    raise InvalidProblemError(f"supply range names node {nid!r} which is not in the problem")
        src = np.fromiter((index[a] for a, _ in pairs), dtype=np.int32, count=len(pairs))
        dst = np.fromiter((index[b] for _, b in pairs), dtype=np.int32, count=len(pairs))
        limit, arc, rate, rising, _ = self.engine.supply_ranges(src, dst)
        inf = _engine.RANGE_INF
        return [SupplyRange(None if lim == inf else lim / f.flow_scale, r / f.cost_scale, self._arc_name(a), k > 0)
                for lim, a, r, k in zip(limit.tolist(), arc.tolist(), rate.tolist(), rising.tolist())]

    def capacity_ranges(self, keys=None):
        """Capacity ranging on the basis resident on the device (``mcf_capacity_ranges``): for every arc, the interval its
        capacity may move in -- this arc alone -- without a tree flow leaving its bounds, so that ``update_capacities`` inside
        it keeps the basis and the ``solve()`` after it makes no pivot.  ``rate`` is the objective change per unit of capacity
        added: the reduced cost of an arc that sits at its capacity, 0 for every other arc.  All arcs are answered at once on
        the device.  Meaningful after a ``solve()`` that ended "optimal".

        * object-model problems: ``keys`` = ``(tail, head)`` keys (default: all; of parallel arcs the LAST one, as in
          ``update_capacities``); returns ``{(tail, head): (lowest_capacity, highest_capacity, rate, limiting_arc_down,
          limiting_arc_up)}`` in the caller's units, lower bounds included; ``None`` for an unbounded end -- both ends of an
          uncapacitated arc -- and for no limiting arc.
        * ``SoAProblem``: ``keys`` = arc indices (default: all, duplicates allowed); returns ``(lowest, highest, rate,
          limiting_arc_down, limiting_arc_up)`` arrays in the order asked: exact int64, ``engine.RANGE_INF`` for an unbounded
          highest, -1 for the lowest of an uncapacitated arc and for no limiting arc."""
        f = self.flat
        m = len(f.keys)
        if f.soa:
            idx = None
            if keys is not None:
                idx = np.asarray(keys).reshape(-1)
                if idx.size and not np.issubdtype(idx.dtype, np.integer):
                    raise InvalidProblemError("capacity ranges: arc indices must be integers")
                idx = idx.astype(np.int64)
                if idx.size and (idx.min() < 0 or idx.max() >= m):
                    raise InvalidProblemError(f"capacity ranges: arc index outside [0, {m})")
        else:
            last: dict[tuple[str, str], int] = {}
            for i, key in enumerate(f.keys):
                last[key] = i
            wanted = list(last) if keys is None else [tuple(k) for k in keys]
            missing = [k for k in wanted if k not in last]
            if missing:
                raise InvalidProblemError(f"capacity range asked for arc {missing[0]} which is not in the problem")
            idx = np.fromiter((last[k] for k in wanted), dtype=np.int64, count=len(wanted))
        down, up, down_arc, up_arc, rate, _ = self.engine.capacity_ranges(idx)
        cap = f.cap if idx is None else f.cap[idx]
        lower = f.lower if idx is None else f.lower[idx]
        inf = _engine.RANGE_INF
        if f.soa:
            shift = lower.astype(np.int64)
            lowest = np.where(down == inf, -1, cap - np.where(down == inf, 0, down) + shift)
            highest = np.where(up == inf, inf, cap + np.where(up == inf, 0, up) + shift)
            return lowest, highest, rate, down_arc, up_arc
        out = {}
        for k, c, lo, d, u, da, ua, r in zip(wanted, cap.tolist(), lower.tolist(), down.tolist(), up.tolist(), down_arc.tolist(), up_arc.tolist(), rate.tolist()):
            out[k] = (None if d == inf else (c - d) / f.flow_scale + lo, None if u == inf else (c + u) / f.flow_scale + lo,
                      r / f.cost_scale, self._arc_name(da), self._arc_name(ua))
        return out

    def _update_rhs(self, supplies, capacities, dual: bool = False) -> dict:
        f = self.flat
        s_idx, s_int, s_val, c_idx, c_int, c_val = map_rhs_changes(f, supplies, capacities, self.tolerance)
        if dual:
            report, dual_report, _ = self.engine.update_rhs_dual(s_idx, s_int, c_idx, c_int)
            report["dual"] = dual_report
        else:
            report = self.engine.update_rhs(s_idx, s_int, c_idx, c_int)
        new_supply, new_cap = f.supply.copy(), f.cap.copy()
        new_supply[s_idx] = s_int
        new_cap[c_idx] = c_int
        if f.soa:
            problem = copy.copy(self.problem)
            if s_idx.size:
                problem.supply = self.problem.supply.copy()
                problem.supply[s_idx] = s_val.astype(self.problem.supply.dtype)
            if c_idx.size:
                problem.capacity = self.problem.capacity.copy()
                problem.capacity[c_idx] = np.where(np.isnan(c_val), -1, c_val).astype(self.problem.capacity.dtype)
            problem._arcs = None
            self.problem = problem
        else:
            nodes = dict(self.problem.nodes)
            for i, v in zip(s_idx.tolist(), s_val.tolist()):
                nid = f.node_ids[i]
                nodes[nid] = replace(nodes[nid], supply=v)
            arcs = list(self.problem.arcs)
            if c_idx.size:
                order = self._arc_order()
                for j, c in zip(c_idx.tolist(), c_val.tolist()):
                    arcs[order[j]] = replace(arcs[order[j]], capacity=None if math.isnan(c) else c)
            self.problem = replace(self.problem, nodes=nodes, arcs=arcs)
        self.flat = replace(f, supply=new_supply, cap=new_cap)
        return report

    def update_supplies(self, changes, dual: bool = False) -> dict:
        """Change supplies / demands and keep the solved state (``mcf_update_rhs``): the tree flows of the resident basis
        are recomputed on the device; where they respect the bounds the basis stays (a solved instance is optimal again in
        zero pivots), otherwise it is repaired and the next ``solve()`` pivots on from it.  ``changes``: ``{node id:
        supply}`` for an object-model problem, ``(indices, supplies)`` for an ``SoAProblem`` (``map_rhs_changes``; on an
        invalid change nothing is changed).  The caller's problem object is left alone: ``self.problem`` becomes an updated
        copy.  Returns the engine's report (``path`` 0 = basis kept, 1 = repaired, 2 = cold start).  ``dual=True``: dual simplex
        pivots on the device drive violated tree flows back inside their bounds before any repair (``mcf_update_rhs_dual``);
        the report then carries the fields of ``mcf_dual_report`` under ``"dual"``."""
        return self._update_rhs(changes, None, dual)

    def update_capacities(self, changes, dual: bool = False) -> dict:
        """Change arc capacities and keep the solved state, as ``update_supplies`` does.  ``changes``: ``{(tail, head):
        capacity or None}`` for an object-model problem, ``(indices, capacities)`` (negative: none) for an ``SoAProblem``."""
        return self._update_rhs(None, changes, dual)

    def _arc_order(self) -> list[int]:
        """flat arc j is arc order[j] of the problem: flatten_problem's stable sort by key, then the arcs ``add_arcs`` appended."""
        if self._arc_order_map is not None:
            return self._arc_order_map
        arcs = self.problem.arcs
        return sorted(range(len(arcs)), key=lambda i: (arcs[i].tail, arcs[i].head))

    def add_arcs(self, arcs) -> dict:
        """Add arcs and keep the solved state (``mcf_add_arcs``): the new arcs enter non-basic at their lower bound, the basis
        that is resident on the device stays, and the next ``solve()`` goes on pivoting from it.  ``arcs``: the dicts
        ``build_problem`` takes for an object-model problem, ``(tail, head, cost, capacity[, lower])`` arrays for an
        ``SoAProblem`` (``map_arc_additions``; on an invalid arc nothing is changed).  New arcs with a lower bound send their
        supply shift through ``mcf_update_rhs`` in the same call.  The flat problem and ``self.problem`` (an extended copy:
        the caller's object is left alone) grow by the new arcs, appended in the given order, so that results, ``certify()``
        and later keyed updates see them.  Returns ``path`` (0 = resident re-layout; 2 = a new handle on the extended
        instance warm-started from the resident basis, taken when the handle's engine path cannot hold the grown instance),
        ``first_index``, ``count``, ``eligible`` and ``device_ms``."""
        f = self.flat
        add = map_arc_additions(f, arcs, self.tolerance, directed=bool(self.problem.directed))
        k = int(add["tail"].shape[0])
        first = len(f.keys)
        tail, head = np.concatenate([f.tail, add["tail"]]).astype(np.int32), np.concatenate([f.head, add["head"]]).astype(np.int32)
        cost, cap = np.concatenate([f.cost, add["cost"]]).astype(np.int64), np.concatenate([f.cap, add["cap"]]).astype(np.int64)
        report = {"path": 0, "first_index": first, "count": k, "eligible": 0, "device_ms": 0.0}
        try:
            rep = self.engine.add_arcs(add["tail"], add["head"], add["cost"], add["cap"])
            report["eligible"], report["device_ms"] = int(rep["eligible"]), float(rep["device_ms"])
        except _engine.EngineError as exc:
            if exc.code != -6:
                raise
            # the handle's engine path cannot hold the grown instance: a new handle, warm-started from the resident basis
            self.logger.info(f"{exc}; building a new handle on the extended instance")
            res = self.engine.result()
            rc_new = add["cost"] + res.potential[add["tail"]] - res.potential[add["head"]]
            kwargs = dict(self._engine_kwargs)
            if kwargs.get("arc_priority") is not None:
                kwargs["arc_priority"] = np.concatenate([np.asarray(kwargs["arc_priority"], np.int8), np.zeros(k, np.int8)])
            new_engine = _engine.McfEngine(len(f.node_ids), tail, head, cost, cap, f.supply, **kwargs)
            in_tree = np.concatenate([res.in_tree, np.zeros(k, bool)])
            at_upper = np.concatenate([~res.in_tree & (f.cap > 0) & (res.flow == f.cap), np.zeros(k, bool)])
            if in_tree.any():
                new_engine.set_basis(in_tree, at_upper)
            self.engine.close()
            self.engine = new_engine
            self._engine_kwargs = kwargs
            self._pivots_seen = 0
            report["path"], report["eligible"] = 2, int((rc_new < 0).sum())
        # the engine holds the arcs from here on: the flat problem and the problem follow at once, the supply shift of new lower
        # bounds after them -- should the engine refuse it, indices and keys still agree with what the engine holds
        supply = f.supply
        lower, orig_cost = np.concatenate([f.lower, add["lower"]]), np.concatenate([f.orig_cost, add["orig_cost"]])
        if f.soa:
            problem = copy.copy(self.problem)
            p = self.problem
            problem.tail, problem.head = tail, head
            problem.cost = np.concatenate([p.cost, add["orig_cost"].astype(p.cost.dtype)])
            problem.capacity = np.concatenate([p.capacity, np.where(add["cap"] < 0, -1, add["cap"] + add["lower"].astype(np.int64)).astype(p.capacity.dtype)])
            problem.lower = np.concatenate([p.lower, add["lower"].astype(p.lower.dtype)])
            problem._arcs = None
            self.problem = problem
            self.flat = replace(f, keys=_KeySeq(tail, head), tail=tail, head=head, cost=cost, cap=cap, supply=supply, lower=lower,
                                orig_cost=orig_cost)
        else:
            from .data import Arc
            old = list(self.problem.arcs)
            self._arc_order_map = self._arc_order() + list(range(len(old), len(old) + k))
            scale = float(f.flow_scale)
            new = [Arc(tail=t, head=h, capacity=None if cp < 0 else cp / scale + lo, cost=c, lower=lo)
                   for (t, h), cp, c, lo in zip(add["keys"], add["cap"].tolist(), add["orig_cost"].tolist(), add["lower"].tolist())]
            if not self.problem.directed:      # an undirected edge is stored with its capacity alone, as the caller wrote it
                new = [replace(a, lower=0.0) for a in new]
            self.problem = replace(self.problem, nodes=dict(self.problem.nodes), arcs=old + new)
            self.flat = replace(f, keys=list(f.keys) + list(add["keys"]), tail=tail, head=head, cost=cost, cap=cap, supply=supply,
                                lower=lower, orig_cost=orig_cost)
        self.actual_arc_count = len(self.flat.keys)
        if add["supply_nodes"].size:
            self.engine.update_rhs(add["supply_nodes"], add["supply_values"])
            supply = f.supply.copy()
            supply[add["supply_nodes"]] = add["supply_values"]
            self.flat = replace(self.flat, supply=supply)
        return report

    def close_arcs(self, keys) -> dict:
        """Close arcs and keep the solved state: capacity 0 through ``update_capacities`` (``mcf_update_rhs``); the arcs stay in
        the problem and every index stays what it was.  ``keys``: ``(tail, head)`` keys for an object-model problem (of
        parallel arcs the last one, as for every keyed update), arc indices for an ``SoAProblem``.  An arc with a positive
        lower bound cannot be closed: ``InvalidProblemError``.  Nor can an edge of an undirected problem: it lives in the resident
        instance as one arc with the bounds [-C, C] shifted to [0, 2C], and that shift (the lower bound -C) is fixed when the
        arc is created, so no capacity of the shifted arc means "no flow either way"; it is refused the same way."""
        f = self.flat
        if f.soa:
            idx = np.asarray(keys, dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= len(f.keys)):
                raise InvalidProblemError(f"capacity changes: index outside [0, {len(f.keys)})")
            changes = (idx, np.zeros(idx.shape[0], dtype=np.int64))
        else:
            last = {key: i for i, key in enumerate(f.keys)}
            idx = []
            for key in keys:
                if tuple(key) not in last:
                    raise InvalidProblemError(f"capacity change names arc {tuple(key)} which is not in the problem")
                idx.append(last[tuple(key)])
            idx = np.asarray(idx, dtype=np.int64)
            changes = {tuple(key): 0.0 for key in keys}
        bound = idx[f.lower[idx] != 0] if idx.size else idx
        if bound.size:
            t, h = f.keys[int(bound[0])]
            lo = float(f.lower[int(bound[0])])
            what = f"has the lower bound {lo:g}" if lo > 0 else f"is an undirected edge (bounds shifted by {-lo:g})"
            raise InvalidProblemError(f"arc {t} -> {h} {what} and cannot be closed")
        return self.update_capacities(changes)

    def certify(self) -> "Certificate":
        """Certify the state resident on the device -- conservation, bounds, complementary slackness, exact objectives,
        consistency of the basis -- without downloading it (``mcf_certify``).  Objectives are exact Python ints in the
        engine's integer units (flow scale x cost scale, lower bounds shifted out); offenders are mapped back to
        ``(tail, head)`` keys and node ids.

        The verdict "infeasible" is weaker than "optimal": the dual groups cover the real arcs only, so it says that the
        state is optimal for the big-M problem restricted to the artificial arcs still in the basis (those carrying the
        remaining flow); the reduced costs of artificial arcs that have left the basis are not examined."""
        f = self.flat
        c = self.engine.certify()
        arc = lambda i: f.keys[i] if 0 <= i < len(f.keys) else None
        return Certificate(
            verdict=c["verdict"], status=c["status"], proves_status=c["proves_status"],
            primal_objective=c["primal"], big_m_term=c["bigm_term"], dual_objective=c["dual"], gap=c["gap"],
            artificial_flow=c["artificial_flow"], flow_scale=f.flow_scale, cost_scale=f.cost_scale,
            bound_violations=c["negative_flow_count"] + c["over_capacity_count"], worst_bound_arc=arc(c["bounds_worst_arc"]),
            imbalanced_nodes=c["imbalance_count"],
            worst_imbalance_node=f.node_ids[c["imbalance_worst_node"]] if 0 <= c["imbalance_worst_node"] < len(f.node_ids) else None,
            dual_violations=c["dual_lower_count"] + c["dual_upper_count"],
            worst_dual_arc=arc(c["dual_lower_arc"] if c["dual_lower_worst"] >= c["dual_upper_worst"] else c["dual_upper_arc"]),
            basis_inconsistencies=sum(c[k] for k in ("basic_count_mismatch", "tree_rc_count", "state_flow_count", "tree_shape_count",
                                                     "strong_count", "rc_mismatch_count", "key_mismatch_count")),
            raw=c)

    def unbounded_ray(self, arc=None):
        """The witness of an unbounded problem, evaluated on the device (``mcf_certify_ray``): the cycle the entering arc
        closes with the resident tree.  Usable after ``solve()`` raised ``UnboundedProblemError`` -- this object still holds
        the handle.  ``arc``: ``None`` = the arc of that verdict, else a ``(tail, head)`` key (of parallel arcs the last; an
        arc index for an ``SoAProblem``) of any non-basic arc.  Returns an ``UnboundedRay``."""
        from .utils import UnboundedRay

        f = self.flat
        m = len(f.keys)
        if arc is None:
            index = -1
        elif f.soa:
            index = int(arc)
        else:
            hits = [i for i, key in enumerate(f.keys) if key == tuple(arc)]
            if not hits:
                raise InvalidProblemError(f"arc {tuple(arc)} is not in the problem")
            index = hits[-1]
        r = self.engine.certify_ray(index)
        if f.soa:
            arcs = [int(a) for a in r["arcs"]]
        else:
            arcs = [f.keys[a] if a < m else (f.node_ids[a - m], self.ROOT_NODE) for a in r["arcs"].tolist()]
        raw = {k: v for k, v in r.items() if k != "arcs"}
        return UnboundedRay(arcs=arcs, cost=r["cost"] / f.cost_scale, reduced_cost=r["reduced_cost"] / f.cost_scale,
                            length=int(r["length"]), proven=bool(r["proven"]), raw=raw)

    def infeasibility_cut(self, nodes=None):
        """The witness of an infeasible problem (``mcf_certify_cut``): a node set S whose net supply exceeds what the arcs
        leaving it can carry.  ``nodes=None``: S is searched on the device from the state the last ``solve()`` left (the
        nodes the stranded supply can still reach); ``nodes`` = an iterable of node ids (node indices for an
        ``SoAProblem``): that set is evaluated against the instance alone, solved or not.  Capacity and supply come back in
        the caller's units with the lower-bound shift of the flattening undone.  Returns an ``InfeasibleCut``."""
        from .utils import InfeasibleCut

        f = self.flat
        n = len(f.node_ids)
        in_S = None
        if nodes is not None:
            in_S = np.zeros(n, dtype=bool)
            if f.soa:
                idx = np.fromiter((int(v) for v in nodes), dtype=np.int64)
                if idx.size and (idx.min() < 0 or idx.max() >= n):
                    raise InvalidProblemError(f"node index outside [0, {n})")
            else:
                index = {nid: i for i, nid in enumerate(f.node_ids)}
                missing = [v for v in nodes if v not in index]
                if missing:
                    raise InvalidProblemError(f"node {missing[0]!r} is not in the problem")
                idx = np.fromiter((index[v] for v in nodes), dtype=np.int64)
            in_S[idx] = True
        c = self.engine.certify_cut(in_S)
        S = c.pop("S")
        leaving = np.flatnonzero(S[f.tail] & ~S[f.head])
        entering = S[f.head] & ~S[f.tail]
        capped = leaving[(f.cap[leaving] >= 0) & (f.cap[leaving] < 2 ** 60)]   # the engine's predicate: the capacity sums the capped arcs only
        lower_leaving, lower_entering = float(f.lower[leaving].sum()), float(f.lower[entering].sum())
        scale = f.flow_scale
        return InfeasibleCut(
            nodes=np.flatnonzero(S).tolist() if f.soa else [f.node_ids[i] for i in np.flatnonzero(S)],
            leaving_arcs=leaving.tolist() if f.soa else [f.keys[i] for i in leaving],
            capacity=c["capacity"] / scale + float(f.lower[capped].sum()),
            supply=c["supply"] / scale + lower_leaving - lower_entering,
            entering_lower=lower_entering, excess=c["excess"] / scale, proven=bool(c["proven"]), raw=c)

    def _objective_estimate(self, flow: np.ndarray) -> float:
        f = self.flat
        return float(np.dot(flow / f.flow_scale + f.lower, f.orig_cost))

    def solve(self, max_iterations: int | None = None, progress_callback: ProgressCallback | None = None,
              progress_interval: int = 100, warm_start_basis: Basis | None = None) -> FlowResult:
        """Solve; returns a FlowResult, raises UnboundedProblemError (simplex.py:1446-1765)."""
        max_iterations = self.default_budget(max_iterations)    # simplex.py:1470 (len(arcs) incl. artificial)
        if warm_start_basis is not None:
            self.logger.info("Attempting to apply warm-start basis")      # simplex.py:1496
            if not self._apply_warm_start_basis(warm_start_basis):
                self.logger.info("Warm-start failed, performing cold start")  # simplex.py:1528
        start = time.time()

        progress = None
        raised: list[BaseException] = []
        if progress_callback is not None:
            def progress(pivots: int, cap: int, elapsed: float):
                res = self.engine.result()
                phase = 1 if res.stats["artificial_flow"] > 0 else 2
                try:
                    progress_callback(ProgressInfo(iteration=pivots, max_iterations=max_iterations, phase=phase,
                                                   phase_iterations=pivots,
                                                   objective_estimate=self._objective_estimate(res.flow),
                                                   elapsed_time=time.time() - start))
                except BaseException as exc:  # an exception cannot cross the C boundary: stop the solve, re-raise after
                    raised.append(exc)
                    return True
                return False

        self.engine.solve(max_iterations, progress, progress_interval)
        if raised:
            raise raised[0]
        return self._collect()

    def default_budget(self, max_iterations: int | None = None) -> int:
        """The pivot budget ``solve`` would use (simplex.py:1470)."""
        if max_iterations is None:
            max_iterations = self.options.max_iterations
        if max_iterations is None:
            max_iterations = max(100, 20 * (self.actual_arc_count + len(self.flat.node_ids)))
        return int(max_iterations)

    def _collect(self) -> FlowResult:
        """The engine's final state as the reference's FlowResult (simplex.py:1573-1765); raises UnboundedProblemError."""
        f = self.flat
        m = self.actual_arc_count
        res = self.engine.result()
        self.stats = res.stats
        # the engine counts pivots cumulatively over successive solves of one handle: report this call's
        iterations = int(res.stats["pivots"]) - self._pivots_seen
        self._pivots_seen = int(res.stats["pivots"])
        self.degenerate_pivots = int(res.stats["degenerate"])

        if res.status == "unbounded":                             # simplex.py:1231-1246
            arc = int(res.stats["unbounded_arc"])
            raise UnboundedProblemError(
                "Unbounded problem detected: entering arc can increase indefinitely without hitting any "
                "capacity constraint. This indicates a negative-cost cycle with infinite capacity.",
                entering_arc=f.keys[arc] if 0 <= arc < m else None,
                reduced_cost=res.stats["unbounded_rc"] / f.cost_scale)
        if res.status == "infeasible" or (res.status == "iteration_limit" and res.stats["artificial_flow"] > 0):
            # simplex.py:1600-1624: no feasible flow (or none found within the budget)
            return FlowResult(objective=0.0, flows={}, status=res.status, iterations=iterations, duals={})

        if f.soa:
            # flat result: nothing per arc is boxed unless the caller looks at the dict views (simplex.py:1703-1765)
            flow_total = res.flow + self.problem.lower                       # flow + shift, exact integers
            objective = res.objective + int(np.dot(self.problem.lower.astype(object), self.problem.cost.astype(object))
                                            if self.problem.lower.any() else 0)
            at_upper = ~res.in_tree & (f.cap > 0) & (res.flow == f.cap)
            return FlowResult(objective=float(round(float(objective), 12)),
                              flows=LazyFlows(f.tail, f.head, flow_total, self.tolerance), status=res.status,
                              iterations=iterations, duals=LazyDuals(res.potential.astype(np.float64)),
                              basis=ArrayBasis(f.tail, f.head, res.in_tree, at_upper, res.flow))
        flow_value = res.flow.astype(np.float64) / f.flow_scale + f.lower   # flow + shift
        flows: dict[tuple[str, str], float] = {}
        objective = 0.0
        for i, key in enumerate(f.keys):                          # simplex.py:1703-1714
            fv = float(flow_value[i])
            flows[key] = flows.get(key, 0.0) + fv
            objective += fv * float(f.orig_cost[i])
        for key, value in list(flows.items()):                    # simplex.py:1716-1721
            if abs(value) <= self.tolerance:
                flows.pop(key)
            else:
                flows[key] = float(round(value, 12))
        duals = {nid: float(round(int(res.potential[i]) / f.cost_scale, 12)) for i, nid in enumerate(f.node_ids)}
        # simplex.py:1029-1039 (tree arcs with their flows), plus -- outside tree_arcs, where the reference
        # never looks -- the non-basic arcs sitting at capacity, so that a warm start can restore them
        tree_idx = np.nonzero(res.in_tree)[0]
        full_idx = np.nonzero(~res.in_tree & (f.cap > 0) & (res.flow == f.cap))[0]
        arc_flows = {f.keys[i]: float(res.flow[i]) / f.flow_scale for i in tree_idx}
        for i in full_idx:
            arc_flows.setdefault(f.keys[i], float(res.flow[i]) / f.flow_scale)
        basis = Basis(tree_arcs={f.keys[i] for i in tree_idx}, arc_flows=arc_flows)
        return FlowResult(objective=float(round(objective, 12)), flows=flows, status=res.status,
                          iterations=iterations, duals=duals, basis=basis)
