"""Inputs of ``test_gpu_small_loop_budget.py`` (``test_small_loop_budget_cpu.py`` vets them without a GPU): the 256-lane front
kernel of the fused LDS loop names the arrays of a side or a buffer by arithmetic, takes its ballots straight from their compares
and files a wave's two counts as one word.  A plain helper like ``small_loop_back_instances.py``: seeded, no fixtures, every result
computed once.

* trees of 3, 65 and 257 nodes: ``tiny`` (two real nodes: both distances are rounded up), ``netgen(64, 512)``, ``netgen(256, 1024)``;
* ``limit``: the wide-range family at 60 nodes with every capacity from 2^31 on set to 2^32 - 2 or 2^32 - 1 -- the two sides of the
  narrow limit of the ratio tests (``mcf_ratio_narrow_ok``), met by searched pivots among the first ``STEPS``; ``limit_first``:
  the same with 2^32, which puts 2^32 - 1 on the FIRST side (a gaining arc that carries 1);
* the planted sides of 63 .. 65 arcs and the tie instances come from ``small_loop_instances.py`` / ``small_loop_slots_instances.py``."""

from __future__ import annotations

import functools

import numpy as np

import planted_pivots as pp
import small_loop_instances as sl
import small_loop_reduce_instances as ri
import wide_range_instances as wr
from network_flow_solver_amd.generators import ArcSoA

STEPS = 80                               # pivots made one launch each: either side has left from either buffer by then
LIMIT = 1 << 32
TREE_SHAPES = ((64, 512), (256, 1024))   # 65 and 257 tree nodes
SIDES = ((63, 65), (64, 64), (65, 63))   # planted cycle sides round one stride of the ratio tests (65: their wide path)
TREES = (2, 3, 5, 64, 65, 257, 1370)     # tree nodes of the address arithmetic's cases
COUNTS = (0, 1, 63, 64, 65, 1370)
FOLD_BUDGETS = (297, 129, -1)            # one long launch, then resumed twice (the last to the end): the counters across launches


@functools.lru_cache(maxsize=None)
def tiny() -> ArcSoA:
    """Two real nodes, three tree nodes: parallel arcs either way, capacities that force bound flips and swaps."""
    tail = np.array([0, 0, 0, 1, 1], np.int32)
    head = np.array([1, 1, 1, 0, 0], np.int32)
    return ArcSoA(2, tail, head, np.array([5, 2, 9, -1, 3], np.int64), np.array([2, 1, 4, 1, 2], np.int64), np.array([4, -4], np.int64), "budget_tiny")


@functools.lru_cache(maxsize=None)
def limit() -> ArcSoA:
    i = wr.make(1, n=60, m=500, cmax=1000, qmax=1 << 33, tie_rich=True)
    cap = i.cap.copy()
    idx = np.flatnonzero((cap >= (1 << 31)) & (cap < wr.MCF_INF))
    cap[idx] = np.where(np.arange(len(idx)) % 2 == 0, LIMIT - 2, LIMIT - 1)
    return ArcSoA(i.n, i.tail, i.head, i.cost, cap, i.supply, "budget_limit_s1")


@functools.lru_cache(maxsize=None)
def limit_first() -> ArcSoA:
    """``limit`` with those capacities at 2^32: a first-side arc that gains flow and carries 1 has the residual 2^32 - 1, one past
    the narrow limit -- the first side's wide detection and its fall back to the 64-bit reduction."""
    i = limit()
    cap = i.cap.copy()
    cap[cap >= LIMIT - 2] = np.where(cap[cap >= LIMIT - 2] < wr.MCF_INF, LIMIT, cap[cap >= LIMIT - 2])
    return ArcSoA(i.n, i.tail, i.head, i.cost, cap, i.supply, "budget_limit_first_s1")


@functools.lru_cache(maxsize=None)
def limit_first_log():
    ref = ri.TracedSimplex(pp.cold_plant(limit_first()))
    while len(ref.log) < STEPS and ref.step():
        pass
    return ref.log


@functools.lru_cache(maxsize=None)
def limit_log():
    """What the ratio tests of the first ``STEPS`` pivots see (``small_loop_reduce_instances.TracedSimplex``)."""
    ref = ri.TracedSimplex(pp.cold_plant(limit()))
    while len(ref.log) < STEPS and ref.step():
        pass
    return ref.log


@functools.lru_cache(maxsize=None)
def fold_instance() -> ArcSoA:
    """The bench instance: some 560 pivots under rule 0."""
    from network_flow_solver_amd import generators

    return generators.named_instance("netgen_8_08a")


EMPTY_SIDES = ("first_side", "second_side")   # the leaving arc's side; the OTHER side of the planted cycle has no arc


@functools.lru_cache(maxsize=None)
def empty_side_plant(leave: str) -> pp.PivotPlant:
    """A searched pivot one of whose end points is the join itself: the side opposite the leaving arc has length 0."""
    return pp.pivot_plant(stem=5, t2=9, other=0, above=2, leave=leave, direction="after" if leave == "second_side" else "before", seed=31)


@functools.lru_cache(maxsize=None)
def empty_side_trajectory(leave: str):
    ref = pp.RefSimplex(empty_side_plant(leave))
    snaps = []
    while len(snaps) < pp.K_PIVOTS and ref.step():
        snaps.append(ref.snapshot())
    obj = ref.run()
    return snaps, obj, ref.status, ref.pivots


def netgen(n: int, m: int) -> ArcSoA:
    return sl.netgen(n, m)
