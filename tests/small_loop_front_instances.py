"""Inputs of ``test_gpu_small_loop_front.py`` (``test_small_loop_front_cpu.py`` vets them without a GPU): the front of a pivot in
the fused LDS loop -- 32-bit pricing keys where the instance's range allows them (``mcf_small_narrow_ok``), an arg-max that hands
the winner's record to ``begin``.  A plain helper like ``small_loop_instances.py``: seeded, no fixtures, every result computed once."""

from __future__ import annotations

import functools

import numpy as np

import small_loop_control_instances as ci
import small_loop_instances as sl
from network_flow_solver_amd.generators import ArcSoA

SHAPES = ((64, 512), (256, 2048))      # netgen shapes of the narrow-against-wide runs
STEPS = 40                             # solve(1) launches compared one by one
INT32_MAX = 2 ** 31 - 1


def big_m(n: int, max_abs_cost: int) -> int:
    """mcf_build_image's big-M."""
    return (max_abs_cost + 1) * (n + 2)


def rc_bound(bigm: int, max_abs_cost: int) -> int:
    """csrc/mcf_host.h, mcf_small_rc_bound, restated."""
    return 4 * bigm - 5 * max_abs_cost - 1


def edge_cost(n: int) -> int:
    """The largest max|cost| of an n-node instance whose reduced costs provably fit int32:
    4 (n + 2)(C + 1) - 5 C - 1 <= 2^31 - 1."""
    return (2 ** 31 - 4 * (n + 2)) // (4 * (n + 2) - 5)


@functools.lru_cache(maxsize=None)
def edge(above: int) -> ArcSoA:
    """``sl.netgen(64, 512)`` with costs scaled so that max|cost| is ``edge_cost(64) + above``; every third capped arc costs
    the negative of its scaled cost (capped: no negative cycle is unbounded)."""
    b = sl.netgen(64, 512)
    c_max = edge_cost(b.n) + above
    top = int(np.abs(b.cost).max())
    cost = b.cost.astype(object) * c_max // top
    cost = np.array(cost, dtype=np.int64)
    capped = np.flatnonzero(b.cap > 0)
    cost[capped[::3]] *= -1
    assert int(np.abs(cost).max()) == c_max
    return ArcSoA(b.n, b.tail, b.head, cost, b.cap, b.supply, f"netgen_64_512_edge_plus_{above}")


@functools.lru_cache(maxsize=None)
def unit_grid() -> ArcSoA:
    """8 x 8 grid, arcs both ways between neighbours, every cost 1, every capacity 3; the first row supplies one unit per node,
    the last row takes one: eligible arcs tie within a lane, a half-wave, a wave and across waves at every sweep."""
    k = 8
    tail, head = [], []
    for r in range(k):
        for c in range(k):
            v = r * k + c
            if c + 1 < k:
                tail += [v, v + 1]; head += [v + 1, v]
            if r + 1 < k:
                tail += [v, v + k]; head += [v + k, v]
    m = len(tail)
    supply = np.zeros(k * k, np.int64)
    supply[:k] = 1
    supply[-k:] = -1
    return ArcSoA(k * k, np.array(tail, np.int32), np.array(head, np.int32), np.ones(m, np.int64), np.full(m, 3, np.int64), supply, "grid_8x8_unit_costs")


def emul_bounds(inst, rule: int, pivots: int) -> tuple[int, int]:
    """(max |cost + pi[tail] - pi[head]| over the real arcs and the artificial ones of either direction, max |pi|) of the CPU
    emulation's state after ``pivots`` pivots.  The root's potential is 0; artificial arc of node v: cost big-M, v <-> root."""
    em = ci.emul(inst, rule, pivots)
    pi = em["potential"].astype(object)
    rc = inst.cost.astype(object) + pi[inst.tail] - pi[inst.head]
    bm = big_m(inst.n, int(np.abs(inst.cost).max()))
    worst_real = max(abs(int(x)) for x in rc) if len(rc) else 0
    worst_art = max(bm + abs(int(x)) for x in pi)
    return max(worst_real, worst_art), max(abs(int(x)) for x in pi)
