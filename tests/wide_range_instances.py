"""Seeded instances at the edges of the engine's numeric domain (include/mcf.h, "Numeric domain"), plus the exact
yardsticks the numeric-range tests compare against.  A plain helper like ``random_instances.py``.

The family (``make``) is feasible and bounded BY CONSTRUCTION, so no seed ever has to be skipped:

* ``m`` random arcs ``tail != head`` and a ring ``v -> v + 1 mod n``;
* random-arc cost: a magnitude class per arc out of {1, 10, 10^3, 10^6, cmax}, the value uniform in [-mag, mag],
  10 % forced to exactly 0; ``cmax`` = INT32_MAX where big-M = (max|c| + 1)(n + 2) stays below 2^44, else the largest
  value for which it does;
* random-arc capacity uniform in [1, qmax), 10 % exactly 0; EVERY random arc is capped, so a negative cycle is bounded;
* ring arcs: cost +cmax, capacity 8 qmax -- the feasibility skeleton (the total supply is below 3 qmax);
* three sources and three sinks (six distinct nodes), source i sending q_i in [1, qmax) to sink i.

``tie_rich=True``: costs only out of {-cmax, -1, 0, 1, cmax}, capacities out of {0, 1, qmax}.
``nonneg=True`` (an extra, not part of the family proper): the same arcs with costs max(|cost|, cmax / 8) -- no negative cycle and no cheap
arc, so the optimum is the transport alone, POSITIVE and beyond 2^63 (the family's own optimum is negative: its capped negative cycles dominate).

Nothing here goes through ``float``: costs, capacities and supplies are int64 arrays, every yardstick works on Python
ints (objectives run to ~2^90).
"""

from __future__ import annotations

import numpy as np

from network_flow_solver_amd.generators import ArcSoA

INT32_MAX = (1 << 31) - 1
BIG_M_LIMIT = 1 << 44          # mcf_build_image: big-M must stay below this
MCF_INF = 1 << 60              # csrc/mcf_core.h: "uncapacitated" and the ratio test's infinity
VKEY_SAT = 0x7fffffff          # csrc/mcf_core.h: MCF_VKEY_SAT

# (nodes, random arcs): the LDS path, past the LDS path, the mid loop, and -- see edge_instance -- n = 8 189
SIZES = {"small": (60, 500), "medium": (1024, 8192), "large": (4096, 32768)}
EDGE_N = 8189                  # the largest n for which a cost of INT32_MAX is admissible: 2^31 * 8191 < 2^44


def big_m_of(n: int, max_abs_cost: int) -> int:
    return (int(max_abs_cost) + 1) * (int(n) + 2)


def cmax_for(n: int) -> int:
    """Largest admissible |cost| on n nodes: INT32_MAX, or less where big-M would reach 2^44."""
    return min(INT32_MAX, (BIG_M_LIMIT - 1) // (n + 2) - 1)


def make(seed: int, n: int = 60, m: int = 500, qmax: int = 1 << 40, tie_rich: bool = False, cmax: int | None = None,
         nonneg: bool = False) -> ArcSoA:
    assert n >= 8 and m >= 0 and 2 <= qmax <= 1 << 56
    cmax = cmax_for(n) if cmax is None else int(cmax)
    assert big_m_of(n, cmax) < BIG_M_LIMIT
    rng = np.random.default_rng([20240, seed, n, m, int(qmax).bit_length(), int(tie_rich)])
    tail = rng.integers(0, n, m).astype(np.int32)
    head = ((tail + 1 + rng.integers(0, n - 1, m)) % n).astype(np.int32)
    if tie_rich:
        cost = rng.choice(np.array([-cmax, -1, 0, 1, cmax], np.int64), m)
        cap = rng.choice(np.array([0, 1, qmax], np.int64), m)
    else:
        mags = np.array([1, 10, 10 ** 3, 10 ** 6, cmax], np.int64)
        mag = np.minimum(mags[rng.integers(0, len(mags), m)], cmax)
        cost = rng.integers(-mag, mag + 1, dtype=np.int64)
        cost[rng.random(m) < 0.10] = 0
        cap = rng.integers(1, qmax, m, dtype=np.int64)
        cap[rng.random(m) < 0.10] = 0
    if nonneg:
        cost = np.maximum(np.abs(cost), cmax >> 3)
    ring = np.arange(n, dtype=np.int32)
    tail = np.concatenate((tail, ring))
    head = np.concatenate((head, ((ring + 1) % n).astype(np.int32)))
    cost = np.concatenate((cost, np.full(n, cmax, np.int64)))
    cap = np.concatenate((cap, np.full(n, 8 * qmax, np.int64)))
    supply = np.zeros(n, np.int64)
    ends = rng.choice(n, 6, replace=False)
    q = rng.integers(1, qmax, 3, dtype=np.int64)
    supply[ends[:3]] = q
    supply[ends[3:]] = -q
    name = f"wide_{'ties_' if tie_rich else ''}{'nonneg_' if nonneg else ''}{n}_{m}_q{int(qmax).bit_length() - 1}_s{seed}"
    return ArcSoA(n, tail, head, cost.astype(np.int64), cap.astype(np.int64), supply, name)


def edge_instance(seed: int = 0, m: int = 16384, qmax: int = 1 << 40) -> ArcSoA:
    """The admissibility edge: n = 8 189 with exactly ONE arc at INT32_MAX (big-M = 2^31 * 8 191, just under 2^44);
    everything else as in the family, with the other costs bounded by 10^6."""
    n = EDGE_N
    inst = make(seed, n, m, qmax, cmax=10 ** 6)
    cost = inst.cost.copy()
    cost[m] = INT32_MAX                                   # the ring arc 0 -> 1
    assert big_m_of(n, int(np.abs(cost).max())) < BIG_M_LIMIT <= big_m_of(n + 1, INT32_MAX)
    return ArcSoA(n, inst.tail, inst.head, cost, inst.cap, inst.supply, f"wide_edge_{n}_{m}_s{seed}")


# ------------------------------------------------------------------ exact yardsticks (Python ints only)
def exact_objective(inst, flow) -> int:
    return sum(int(f) * int(c) for f, c in zip(np.asarray(flow).tolist(), inst.cost.tolist()))


def exact_certificate(inst, flow, potential) -> int:
    """Conservation, bounds and complementary slackness in Python-int arithmetic (cap < 0 or >= 2^60: uncapacitated);
    returns the objective recomputed as an exact int.  An optimality proof that needs no other solver."""
    flow = [int(f) for f in np.asarray(flow).tolist()]
    pi = [int(p) for p in np.asarray(potential).tolist()]
    bal = [int(s) for s in inst.supply.tolist()]
    objective = 0
    for i, (t, h, c, cp) in enumerate(zip(inst.tail.tolist(), inst.head.tolist(), inst.cost.tolist(), inst.cap.tolist())):
        f = flow[i]
        capped = 0 <= cp < MCF_INF
        assert f >= 0 and (not capped or f <= cp), f"arc {i}: flow {f} outside [0, {cp}]"
        bal[t] -= f
        bal[h] += f
        rc = c + pi[t] - pi[h]
        if f > 0 and (not capped or f < cp):
            assert rc == 0, f"arc {i}: interior flow with reduced cost {rc}"
        elif f == 0 and (not capped or cp > 0):
            assert rc >= 0, f"arc {i}: at its lower bound with reduced cost {rc}"
        elif capped and cp > 0:
            assert rc <= 0, f"arc {i}: at its capacity with reduced cost {rc}"
        objective += f * c
    assert not any(bal), "flow conservation violated"
    return objective


def networkx_objective(inst) -> int:
    """Independent exact optimum: networkx.network_simplex on Python ints."""
    import networkx as nx

    g = nx.MultiDiGraph()
    for v, s in enumerate(inst.supply.tolist()):
        g.add_node(v, demand=-int(s))
    for t, h, c, cp in zip(inst.tail.tolist(), inst.head.tolist(), inst.cost.tolist(), inst.cap.tolist()):
        if 0 <= cp < MCF_INF:
            g.add_edge(t, h, weight=int(c), capacity=int(cp))
        else:
            g.add_edge(t, h, weight=int(c))
    value, _ = nx.network_simplex(g)
    assert isinstance(value, int)
    return value


# ------------------------------------------------------------------ compressed Dantzig keys (csrc/mcf_core.h: mcf_vkey)
def _vkey_code(viol: np.ndarray, bigm: int, half: int) -> np.ndarray:
    """csrc/mcf_core.h:mcf_vkey in numpy: the compressed Dantzig key of a violation."""
    SAT = VKEY_SAT
    viol = viol.astype(np.int64)
    if bigm < (1 << 29) and half >= (1 << 28):
        return np.where(viol <= 0, 0, np.where(viol < SAT, viol, SAT)).astype(np.int32)
    j = np.where(2 * viol < bigm, 0, np.where(2 * viol < 3 * bigm, 1, np.where(2 * viol < 5 * bigm, 2, 3)))
    d = viol - j * bigm
    ok = (j < 3) & (d < half) & (d > -half)
    code = (j.astype(np.int64) << 29) + d + (1 << 28)
    return np.where(viol <= 0, 0, np.where(ok, code, SAT)).astype(np.int32)


def vkey_int(viol: int, bigm: int, half: int) -> int:
    """The same scheme on Python ints, written from its description (nearest level out of 0 / big-M / 2 big-M, offset
    strictly inside (-half, half), level 0 holding [1, half)) rather than from the C text."""
    if viol <= 0:
        return 0
    if bigm < (1 << 29) and half >= (1 << 28):
        return min(viol, VKEY_SAT)
    j = (2 * viol + bigm) // (2 * bigm)                    # round(viol / big-M), halves up
    d = viol - j * bigm
    if j > 2 or abs(d) >= half:
        return VKEY_SAT
    return (j << 29) + d + (1 << 28)


def vkey_decode_int(code: int, bigm: int, half: int) -> int:
    if bigm < (1 << 29) and half >= (1 << 28):
        return code
    return (code >> 29) * bigm + (code & ((1 << 29) - 1)) - (1 << 28)


KEY_CLASSES = ("zero", "level0", "level1", "level2", "sat_between", "sat_above")


def key_classes(viol: np.ndarray, bigm: int, half: int) -> dict:
    """Arcs per code class of a level-coded handle (big-M >= 2^29 or a narrow half width): zero (ineligible), the three
    levels, saturated BETWEEN two levels (exact compare against coded neighbours on both sides) and saturated ABOVE
    the range of level 2."""
    viol = np.asarray(viol, np.int64)
    code = _vkey_code(viol, bigm, half).astype(np.int64)
    sat = code == VKEY_SAT
    lvl = code >> 29
    above = sat & (viol >= 2 * bigm + half)
    return {"zero": int((code == 0).sum()), "level0": int(((code > 0) & ~sat & (lvl == 0)).sum()),
            "level1": int((~sat & (lvl == 1)).sum()), "level2": int((~sat & (lvl == 2)).sum()),
            "sat_between": int((sat & ~above).sum()), "sat_above": int(above.sum())}


def chain_instance(n: int = 48, chain_cost: int = 8 * 10 ** 7, qmax: int = 1 << 40) -> ArcSoA:
    """Violations NEAR big-M (code level 1) do not occur in the seeded family: a potential is +-big-M plus the cost of a
    tree path, so it takes a path of ~n maximal-cost arcs to get there.  This instance is one: a chain 0 -> 1 -> ... -> n-1
    of arcs of cost C that carries the only supply from node 0 to node n-1.  From the cold start the chain becomes basic
    from its far end, one arc per pivot whatever the rule (only one arc is ever eligible): after p pivots the arc
    (n-2-p) -> (n-1-p) has the violation 2 big-M - (p + 1) C, which walks from level 2 through the gap down to
    big-M + 3 C + n + 2 on the last arc -- level 1, since 3 C + n + 2 < 2^28.  n = 48: that is the state after
    1 + 5 + 40 pivots, one of the stages the budget ladder of the tests stops at."""
    C = int(chain_cost)
    assert 3 * C + n + 2 < (1 << 28)          # (C = 1 000 puts it inside a level of half width 2^12 as well)
    tail = np.arange(n - 1, dtype=np.int32)
    head = (tail + 1).astype(np.int32)
    cost = np.full(n - 1, C, np.int64)
    cap = np.full(n - 1, 8 * qmax, np.int64)
    supply = np.zeros(n, np.int64)
    supply[0], supply[n - 1] = qmax - 1, -(qmax - 1)
    return ArcSoA(n, tail, head, cost, cap, supply, f"wide_chain_{n}")
