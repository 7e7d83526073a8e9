"""Solution analysis with the reference's surface (``network_solver/utils.py:169-312``): ``validate_flow`` and
``compute_bottleneck_arcs``, decided on the device by ``mcf_certify`` / ``mcf_bottlenecks``.

The flows of ``result`` are scaled to integers (as ``flatten_problem`` scales a problem), one engine arc per flow entry is
built with the bounds the problem gives that ``(tail, head)`` key, and the device pass says whether anything is violated
and which arcs are bottlenecks.  Only when it reports a violation does the host walk the arrays to NAME the offenders (the
reference's lists and messages).  ``extract_path`` of the reference is a breadth-first search over a result dict with no
device part; it is not provided.  No CPU fallback: without a device these raise ``EngineUnavailableError``.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import engine as _engine
from .data import FlowResult, NetworkProblem
from .exceptions import SolverConfigurationError
from .simplex import _decimal_scale

__all__ = ["ValidationResult", "BottleneckArc", "UnboundedRay", "InfeasibleCut", "validate_flow", "compute_bottleneck_arcs"]


@dataclass
class ValidationResult:
    """Results from validating a flow solution (field names of the reference)."""

    is_valid: bool
    errors: list[str]
    flow_balance: dict[str, float]
    capacity_violations: list[tuple[str, str]]
    lower_bound_violations: list[tuple[str, str]]


@dataclass
class BottleneckArc:
    """An arc at or near capacity (field names of the reference)."""

    tail: str
    head: str
    flow: float
    capacity: float | None
    utilization: float | None
    cost: float
    slack: float


@dataclass
class UnboundedRay:
    """What ``NetworkSimplex.unbounded_ray()`` returns: the cycle an entering arc closes with the resident tree, evaluated on
    the device (``mcf_certify_ray``).  ``proven``: every arc is a real arc followed in its own direction and has no capacity,
    and the cycle's cost is negative -- flow can be pushed round it for ever."""

    arcs: list                       # push order: (tail id, head id) keys (arc indices for an SoAProblem); the artificial arc of a
    #                                  node shows as (node id, NetworkSimplex.ROOT_NODE) (as m + node index for an SoAProblem)
    cost: float                      # signed sum of the arcs' costs, in the caller's units
    reduced_cost: float              # the entering arc's reduced cost in the push direction
    length: int
    proven: bool
    raw: dict                        # every field of mcf_ray, integer units


@dataclass
class InfeasibleCut:
    """What ``NetworkSimplex.infeasibility_cut()`` returns: a node set S and what leaves it (``mcf_certify_cut``), in the
    caller's units with the lower-bound shift undone.  ``proven``: no uncapacitated arc leaves S and
    ``excess = supply + entering_lower - capacity > 0``: S has to send out more than its leaving arcs can carry."""

    nodes: list                      # node ids of S (node indices for an SoAProblem)
    leaving_arcs: list               # (tail id, head id) keys of the arcs from S to the rest (arc indices for an SoAProblem)
    capacity: float                  # sum of their capacities
    supply: float                    # net supply of S
    entering_lower: float            # sum of the lower bounds of the arcs into S: flow S cannot refuse
    excess: float
    proven: bool
    raw: dict                        # every field of mcf_cut, integer units


class _Image:
    """One engine arc per entry of ``result.flows``, with the bounds of the problem's arc of that key (of parallel arcs the
    last, as the reference's key -> arc map keeps it); integer-scaled, lower bounds shifted out."""

    def __init__(self, problem, result: FlowResult):
        arc_map = {(a.tail, a.head): a for a in problem.undirected_expansion()}
        self.keys = list(result.flows.keys())
        self.flow = np.array([float(result.flows[k]) for k in self.keys], dtype=np.float64)
        self.node_ids = list(problem.nodes.keys())
        index = {nid: i for i, nid in enumerate(self.node_ids)}
        for t, h in self.keys:                       # nodes the problem does not know: balance only, as in the reference
            for nid in (t, h):
                if nid not in index:
                    index[nid] = len(self.node_ids)
                    self.node_ids.append(nid)
        m = len(self.keys)
        self.known = np.array([k in arc_map for k in self.keys], dtype=bool)
        self.capacity = [arc_map[k].capacity if k in arc_map else None for k in self.keys]
        self.lower = np.array([arc_map[k].lower if k in arc_map else -math.inf for k in self.keys], dtype=np.float64)
        self.cost = [arc_map[k].cost if k in arc_map else 0.0 for k in self.keys]
        self.tail = np.fromiter((index[t] for t, _ in self.keys), dtype=np.int32, count=m)
        self.head = np.fromiter((index[h] for _, h in self.keys), dtype=np.int32, count=m)
        self.supply = np.array([problem.nodes[nid].supply if nid in problem.nodes else 0.0 for nid in self.node_ids], dtype=np.float64)
        self.self_loop = self.tail == self.head      # the engine has no self-loops: they cancel in the balance and are checked on the host

    def engine(self, tolerance: float):
        """(engine, integer flows, scale): lower bounds shifted out; an arc the problem does not know is free in both
        directions (cap unlimited, shifted by its own flow so that it never reports a bound)."""
        finite_cap = np.array([c is not None for c in self.capacity], dtype=bool)
        cap = np.array([c if c is not None else 0.0 for c in self.capacity], dtype=np.float64)
        shift = np.where(np.isfinite(self.lower), self.lower, np.minimum(self.flow, 0.0))
        scale = _decimal_scale(np.concatenate((self.supply, cap[finite_cap], shift, self.flow)), "flows / supplies / capacities")
        tol_i = int(math.floor(tolerance * scale))
        flow_i = np.round((self.flow - shift) * scale).astype(np.int64)
        cap_i = np.full(len(self.keys), -1, dtype=np.int64)
        cap_i[finite_cap] = np.round((cap[finite_cap] - shift[finite_cap]) * scale).astype(np.int64)
        if (cap_i[finite_cap] < 0).any() or (cap_i >= 1 << 60).any():
            raise SolverConfigurationError("capacities below the lower bound or beyond 2^60 after scaling")
        supply = self.supply.copy()
        np.subtract.at(supply, self.tail, shift)
        np.add.at(supply, self.head, shift)
        supply_i = np.round(supply * scale).astype(np.int64)
        keep = ~self.self_loop
        # the engine wants balanced supplies; what is missing goes to an extra node nothing touches (its own balance is dropped)
        supply_i = np.concatenate((supply_i, [-int(supply_i.sum())]))
        eng = _engine.McfEngine(len(supply_i), self.tail[keep], self.head[keep], np.zeros(int(keep.sum()), np.int64), cap_i[keep], supply_i)
        return eng, flow_i, cap_i, keep, scale, tol_i

    def bottleneck_engine(self):
        """(engine, integer flows, engine arc -> entry, entries the host decides alone): flows and capacities scaled but NOT
        shifted, because the reference's utilisation is ``flow / capacity`` in the caller's terms whatever the lower bound is
        (an undirected edge has ``lower = -capacity``).  Supplies play no part in the comparison and are zero.  Self-loops
        (the engine has none) and capacities below zero (outside its domain) are left to the host's comparison."""
        finite_cap = np.array([c is not None for c in self.capacity], dtype=bool)
        cap = np.array([c if c is not None else 0.0 for c in self.capacity], dtype=np.float64)
        scale = _decimal_scale(np.concatenate((cap[finite_cap], self.flow)), "flows / capacities")
        flow_i = np.round(self.flow * scale).astype(np.int64)
        cap_i = np.full(len(self.keys), -1, dtype=np.int64)
        cap_i[finite_cap] = np.round(cap[finite_cap] * scale).astype(np.int64)
        if (cap_i >= 1 << 60).any():
            raise SolverConfigurationError("capacities beyond 2^60 after scaling")
        host_only = self.self_loop | (finite_cap & (cap_i < 0))
        kept = np.flatnonzero(~host_only)
        eng = _engine.McfEngine(len(self.node_ids), self.tail[kept], self.head[kept], np.zeros(kept.size, np.int64), cap_i[kept],
                                np.zeros(len(self.node_ids), np.int64))
        return eng, flow_i[kept], kept, np.flatnonzero(host_only)


class _ClosingHandle:
    """Context manager around the tuple an ``_Image`` method returns: its first entry, the engine handle, is closed on exit."""

    def __init__(self, parts):
        self.parts = parts

    def __enter__(self):
        return self.parts

    def __exit__(self, *exc):
        self.parts[0].close()


def validate_flow(problem: NetworkProblem, result: FlowResult, tolerance: float = 1e-6) -> ValidationResult:
    """Flow conservation at each node, capacity and lower-bound constraints of every arc in ``result.flows`` -- the
    reference's checks and result, decided on the device.

    Two differences from the reference, both from deciding on exact integers.  (1) Flows, supplies and bounds are scaled to
    integers as ``flatten_problem`` scales a problem, so values with more decimals than that scaling admits (a float
    result of some other solver, say) raise ``SolverConfigurationError`` where the reference validates any floats.
    (2) When the device reports nothing beyond ``tolerance``, ``flow_balance`` is exactly 0.0 for every node; the
    reference returns the float residuals it computed (below ``tolerance`` in that case).  With a violation anywhere the
    balances are the reference's float sums."""
    im = _Image(problem, result)
    with _ClosingHandle(im.engine(tolerance)) as (eng, flow_i, cap_i, keep, scale, tol_i):
        cert = eng.certify(flow_i[keep], np.zeros(eng.n, np.int64), _engine.CERT_BOUNDS | _engine.CERT_CONSERVATION)
    # (the padding node carries what the supplies lack to balance: non-zero only when some real node is out of balance too)
    clean = cert["bounds_worst"] <= tol_i and cert["imbalance_worst"] <= tol_i and not im.self_loop.any()
    balance = {nid: 0.0 for nid in im.node_ids}
    errors: list[str] = []
    cap_v: list[tuple[str, str]] = []
    low_v: list[tuple[str, str]] = []
    if not clean:                                    # name the offenders (host walk, violations only)
        bal = im.supply.copy()
        np.subtract.at(bal, im.tail, im.flow)
        np.add.at(bal, im.head, im.flow)
        for i, (t, h) in enumerate(im.keys):
            f = float(im.flow[i])
            if not im.known[i]:
                continue
            c = im.capacity[i]
            if c is not None and f > c + tolerance:
                cap_v.append((t, h))
                errors.append(f"Arc ({t}, {h}): flow {f:.6f} exceeds capacity {c:.6f}")
            if f < im.lower[i] - tolerance:
                low_v.append((t, h))
                errors.append(f"Arc ({t}, {h}): flow {f:.6f} below lower bound {im.lower[i]:.6f}")
        for nid, b in zip(im.node_ids, bal.tolist()):
            balance[nid] = b
            if abs(b) > tolerance:
                errors.append(f"Node {nid}: flow imbalance {b:.6f} (should be zero)")
    return ValidationResult(is_valid=not errors, errors=errors, flow_balance=balance, capacity_violations=cap_v,
                            lower_bound_violations=low_v)


def compute_bottleneck_arcs(problem: NetworkProblem, result: FlowResult, threshold: float = 0.95,
                            tolerance: float = 1e-6) -> list[BottleneckArc]:
    """Arcs of ``result.flows`` with finite capacity whose utilisation ``flow / capacity`` is at least ``threshold``, sorted by
    utilisation (descending) and slack, as in the reference.  The candidates come from the device (``mcf_bottlenecks`` on the
    unshifted integer flows and capacities -- lower bounds play no part in the reference's utilisation -- with
    ``threshold`` as an exact fraction, one step below it so that rounding cannot lose an arc); the host then applies the
    reference's float comparison to those few.  Values with more decimals than the integer scaling admits raise
    ``SolverConfigurationError``."""
    im = _Image(problem, result)
    if not im.keys:
        return []
    num, den = (max(0.0, threshold) * (1 - 1e-9)).as_integer_ratio()
    while den > 1 << 61 or num > 1 << 61:
        num, den = num >> 1, den >> 1
    with _ClosingHandle(im.bottleneck_engine()) as (eng, flow_i, kept, host_only):
        idx, _ = eng.bottlenecks(num, max(den, 1), flow=flow_i)
    candidates = np.sort(np.concatenate((kept[idx], host_only)))   # in the order of result.flows, as the reference walks them
    out: list[BottleneckArc] = []
    for i in candidates.tolist():
        f, c = float(im.flow[i]), im.capacity[i]
        if f < tolerance or not im.known[i] or c is None:
            continue
        u = f / c if c > 0 else 0.0
        if u >= threshold:
            out.append(BottleneckArc(tail=im.keys[i][0], head=im.keys[i][1], flow=f, capacity=c, utilization=u, cost=im.cost[i], slack=c - f))
    out.sort(key=lambda x: (-(x.utilization or 0.0), x.slack))
    return out
