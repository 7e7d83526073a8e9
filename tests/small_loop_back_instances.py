"""Inputs of ``test_gpu_small_loop_back.py`` (``test_apply_paths_cpu.py`` vets them without a GPU): the fused LDS loop runs the
finish pass in its LAST wave while the other waves already apply, and the last wave then takes the apply positions from
``lo + THREADS - 64`` on.  A plain helper like ``small_loop_instances.py``: seeded, no fixtures, every result computed once.

* planted pivots that move 191 .. 193 and 255 .. 257 positions: at 256 lanes the finishing wave has no apply work, one
  position, two, its whole share, and a second trip of the whole workgroup;
* planted pivots whose leaving arc has stem index 0, 1, 63, 64, 65 on cycle sides of 63 .. 66 arcs (a side is at least one arc
  longer than the stem index): the 64-lane finish pass takes one and two strides over the flows and over the stem;
* netgen-style shapes of 255 .. 257 and 511 .. 513 real nodes: the node-parallel search passes over the real nodes only -- one,
  one and two passes of 256 lanes, then two, two and three."""

from __future__ import annotations

import functools

import planted_pivots as pp

MOVED_RANGES = (191, 192, 193, 255, 256, 257)
# (stem index of the leaving arc, tree arcs between its node and the join, arcs of the other side)
STEM_SIDES = ((0, 63, 64), (1, 62, 65), (63, 0, 63), (64, 0, 64), (65, 0, 65))
NODE_SHAPES = ((255, 1020), (256, 1024), (257, 1028), (511, 1022), (512, 1024), (513, 1026))
STEPS = 40                               # pivots made one launch each


@functools.lru_cache(maxsize=None)
def range_plant(r: int, leave: str = "first_side") -> pp.PivotPlant:
    """T2 (r - 1 nodes) goes directly behind the leaf ``w``, which lies one node in front of it: [lo, hi) is r positions."""
    return pp.pivot_plant(stem=2, t2=r - 1, other=3, above=1, leave=leave, seed=41)


@functools.lru_cache(maxsize=None)
def stem_plant(stem: int, above: int, other: int, leave: str = "first_side") -> pp.PivotPlant:
    return pp.pivot_plant(stem=stem, t2=stem + 6, other=other, above=above, leave=leave, direction="after" if leave == "second_side" else "before",
                          seed=42)


def _trajectory(p: pp.PivotPlant):
    """As ``planted_pivots.trajectory``: (snapshots after pivots 1 .. K, final objective, final status, pivots in all)."""
    ref = pp.RefSimplex(p)
    snaps = []
    while len(snaps) < pp.K_PIVOTS and ref.step():
        snaps.append(ref.snapshot())
    obj = ref.run()
    return snaps, obj, ref.status, ref.pivots


@functools.lru_cache(maxsize=None)
def range_trajectory(r: int, leave: str = "first_side"):
    return _trajectory(range_plant(r, leave))


@functools.lru_cache(maxsize=None)
def stem_trajectory(stem: int, above: int, other: int, leave: str = "first_side"):
    return _trajectory(stem_plant(stem, above, other, leave))
