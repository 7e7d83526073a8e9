"""Inputs of ``test_gpu_small_loop_decide.py`` (``test_small_loop_decide_cpu.py`` vets them without a GPU): the fused LDS loop's
256-lane front kernel decides a pivot with ``mcf_pivot_decide_flat`` -- selects where ``mcf_pivot_decide`` returns -- so every
exit of the decision and every select of the swap is planted here on trees of at most about 70 nodes.  A plain helper like
``small_loop_back_instances.py``: seeded, no fixtures, every result computed once.

* a bound flip as the first pivot of a launch; a bound flip directly behind a swap inside ONE launch;
* the ties of the three-way comparison: both sides and the entering arc at the same residual (the second side leaves), the
  entering arc's capacity equal to the first side's residual below the second's (a flip); a degenerate step on the first side
  (``planted_pivots`` cannot plant one on the second: a strongly feasible tree has its empty blocking arc on the first);
* a re-hung subtree of one node on the first side and on the second; a stem of 1 and of 3 nodes;
* the insertion point directly behind ``v_in`` (a leaf: both candidates coincide), at the end of its block, and the two at the
  same cost (the tie goes to the point behind ``v_in``);
* an unbounded cycle met after at least one swap of the same launch: the uncapacitated instances of the verdict tests;
* netgen-style instances of 64 / 512 and 40 / 160 (seed 3), stepped one launch per pivot."""

from __future__ import annotations

import functools

import numpy as np

import planted_pivots as pp
import small_loop_control_instances as ci
from network_flow_solver_amd import generators

STEPS = 40
STEPPED_SHAPES = ((64, 512), (40, 160))
UNBOUNDED = ("unbounded_5", "deep_unbounded")

_BASE = dict(stem=2, t2=6, other=3, above=1, seed=61)
# name -> (arguments of pivot_plant, what the first pivot is: "flip" / "first" / "second", its step is degenerate)
PLANTS = {
    "flip_first_pivot": (dict(_BASE, leave="entering"), "flip", False),
    "all_three_tie_second_leaves": (dict(_BASE, leave="second_side", ties=("first", "entering", "second")), "second", False),
    "capacity_ties_first_side_flip": (dict(_BASE, leave="entering", ties=("first", "entering")), "flip", False),
    "degenerate_first_side": (dict(_BASE, leave="first_side", theta0=True), "first", True),
    "one_node_first_side": (dict(stem=0, t2=1, other=4, above=3, leave="first_side", seed=62), "first", False),
    "one_node_second_side": (dict(stem=0, t2=1, other=4, above=3, leave="second_side", seed=62), "second", False),
    "stem_1": (dict(stem=1, t2=4, other=3, above=2, leave="first_side", seed=63), "first", False),
    "stem_3": (dict(stem=3, t2=9, other=3, above=1, leave="second_side", seed=63), "second", False),
    # (this seed's second pivot is a bound flip, both pivots by the parallel search: one launch of two pivots holds the pair)
    "flip_behind_a_swap": (dict(stem=2, t2=6, other=3, above=1, leave="second_side", seed=63), "second", False),
    "insert_behind_a_leaf": (dict(stem=2, t2=5, other=3, above=2, leave="first_side", seed=64), "first", False),
    "insert_at_the_end_of_the_block": (dict(stem=2, t2=5, other=0, above=2, leave="first_side", seed=64), "first", False),
    "insert_tie_goes_behind_v_in": (dict(stem=2, t2=5, other=0, above=0, leave="first_side", seed=64), "first", False),
}
# name -> the insertion point mcf_pivot_swap has to choose: "same" (tA == tB), "tB" (strictly cheaper), "tie" (tA != tB, same cost)
INSERTIONS = {"insert_behind_a_leaf": "same", "insert_at_the_end_of_the_block": "tB", "insert_tie_goes_behind_v_in": "tie"}


@functools.lru_cache(maxsize=None)
def plant(name: str) -> pp.PivotPlant:
    return pp.pivot_plant(**PLANTS[name][0])


@functools.lru_cache(maxsize=None)
def trajectory(name: str):
    """As ``planted_pivots.trajectory``: (snapshots after pivots 1 .. K, final objective, final status, pivots in all)."""
    ref = pp.RefSimplex(plant(name))
    snaps = []
    while len(snaps) < pp.K_PIVOTS and ref.step():
        snaps.append(ref.snapshot())
    obj = ref.run()
    return snaps, obj, ref.status, ref.pivots


def insertion(name: str):
    """(tA, tB, costA, costB) of the planted pivot as mcf_pivot_swap computes them, from the planted tree: positions are labels + 1
    (the root at 0), ``v_in`` is ``w``, T2 is the subtree of ``a``."""
    p = plant(name)
    n = p.inst.n
    parent = np.asarray(p.pl.parent)
    size = np.ones(n + 1, np.int64)
    for x in range(n - 1, -1, -1):          # labels are preorder numbers: children come behind their parents
        size[parent[x]] += size[x]
    pos = lambda x: 0 if x == n else x + 1
    a0, s = pos(p.a), int(size[p.a])
    assert s == p.t2
    t_a, t_b = pos(p.w) + 1, pos(p.w) + int(size[p.w])
    cost = lambda t: a0 - t if t <= a0 else t - (a0 + s)
    return t_a, t_b, cost(t_a), cost(t_b)


@functools.lru_cache(maxsize=None)
def stepped(n: int, m: int):
    return generators.netgen_style(n, m, seed=3)



def unbounded(name: str):
    return ci.verdict_cases()[name][0]
