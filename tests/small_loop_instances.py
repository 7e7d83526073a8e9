"""Inputs of the fused LDS loop's tests (``test_gpu_small_loop.py``; ``test_small_loop_cpu.py`` checks them without a GPU).  A plain
helper like ``planted_pivots.py``: seeded, no fixtures, every result computed once and never changed.

* node counts around the workgroup's width: the node-parallel cycle search takes nodes ``x, x + THREADS, ...``, so 255 .. 258 and
  511 .. 514 tree nodes are one, two and three passes of a 256-lane workgroup;
* arc counts around a step of ``m_pad`` (1 024): padded entries must never be priced;
* a transportation instance whose heads all fall in the FIRST head bucket (nodes 0 .. 31 of 256): the lanes of that bucket price
  far more arcs than they keep in registers (``small_reg_arcs``: 320 per bucket at 256 lanes, 384 at 1 024), the others none;
* netgen-style instances whose first bucket holds 319 .. 321 and 383 .. 385 arcs: the last register slot of a lane is the
  bucket's last arc, one short of it, and one arc goes to the LDS loop;
* planted pivots whose two cycle sides are 63 .. 65 and 127 .. 129 arcs long -- one and two strides of the 64-lane ratio test --
  with every set of tying arcs."""

from __future__ import annotations

import functools

import numpy as np

import planted_pivots as pp
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

WIDTHS = (256, 1024)                     # every compiled width of k_solve_small
NODE_COUNT_SHAPES = ((254, 1016), (255, 1020), (256, 1024), (257, 1028), (510, 1020), (511, 1022), (512, 1024), (513, 1026))
PADDING_SHAPES = ((256, 1023), (256, 1025), (256, 2048))
# per-bucket register capacity of the lane maps -- 320 and 384 arcs -- minus 1, at it and plus 1 all lie below the smallest
# feasible instance of this shape, 1 024 arcs, which therefore stands for them; then a second and a third step of m_pad
TRANSPORT_ARCS = (1024, 2048, 2049)
# ... and a head bucket AT the register capacity: netgen-style arcs plus extra ones into the first bucket until it holds exactly
# this many -- one less, just as many and one more than 32 lanes x 10 slots and 128 lanes x 3 slots
BUCKET_ARCS = (319, 320, 321, 383, 384, 385)
SIDE_LENGTHS = ((63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127))


@functools.lru_cache(maxsize=None)
def netgen(n: int, m: int) -> ArcSoA:
    return generators.netgen_style(n, m, seed=5)


@functools.lru_cache(maxsize=None)
def transport(m: int) -> ArcSoA:
    """224 unit sources (nodes 32 .. 255), 32 sinks of 7 (nodes 0 .. 31); one arc from each source first, the rest from random
    sources; heads random among the sinks; costs 1 .. 100, every capacity 256."""
    n = 256
    rng = np.random.default_rng([256, m])
    supply = np.ones(n, np.int64)
    supply[:32] = -7
    tail = np.concatenate((np.arange(32, n), rng.integers(32, n, m - (n - 32))))
    head = rng.integers(0, 32, m)
    return ArcSoA(n, tail.astype(np.int32), head.astype(np.int32), rng.integers(1, 101, m).astype(np.int64), np.full(m, 256, np.int64),
                  supply, f"transport_first_bucket_{m}")


@functools.lru_cache(maxsize=None)
def bucket_at(k: int) -> ArcSoA:
    """netgen_style(256, 1024, seed=5) with further arcs into nodes 0 .. 31 -- the first head bucket -- so that exactly k arcs
    end there.  Added arcs keep the instance feasible; their costs lie in the range of the others so that they take part."""
    base = netgen(256, 1024)
    have = int((base.head < 32).sum())
    extra = k - have
    assert extra > 0
    rng = np.random.default_rng([320, k])
    head = rng.integers(0, 32, extra)
    tail = rng.integers(32, 256, extra)
    lo, hi = int(base.cost.min()), int(base.cost.max())
    cost = rng.integers(lo, hi + 1, extra)
    cap = rng.integers(1, max(int(base.cap[base.cap > 0].max()), 2) + 1, extra)
    return ArcSoA(base.n, np.concatenate((base.tail, tail)).astype(np.int32), np.concatenate((base.head, head)).astype(np.int32),
                  np.concatenate((base.cost, cost)).astype(np.int64), np.concatenate((base.cap, cap)).astype(np.int64), base.supply.copy(),
                  f"first_bucket_of_{k}")


@functools.lru_cache(maxsize=None)
def side_plant(n1: int, n2: int, ts: tuple) -> pp.PivotPlant:
    """A cycle of n1 + n2 + 1 arcs: n1 tree arcs on the side of the re-hung subtree, n2 on the other."""
    return pp.pivot_plant(stem=n1 - 3, t2=n1 + 3, other=n2, above=2, leave=pp._tie_winner(ts), ties=ts, seed=21)


@functools.lru_cache(maxsize=None)
def side_trajectory(n1: int, n2: int, ts: tuple):
    """As ``planted_pivots.trajectory``: (snapshots after pivots 1 .. K, final objective, final status, pivots in all)."""
    ref = pp.RefSimplex(side_plant(n1, n2, ts))
    snaps = []
    while len(snaps) < pp.K_PIVOTS and ref.step():
        snaps.append(ref.snapshot())
    obj = ref.run()
    return snaps, obj, ref.status, ref.pivots


SIDE_PARAMS = [(n1, n2, ts) for n1, n2 in SIDE_LENGTHS for ts in pp.TIE_SETS]
SIDE_IDS = [f"{n1}_{n2}-" + "_".join(ts) for n1, n2, ts in SIDE_PARAMS]
