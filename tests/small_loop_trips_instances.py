"""Inputs of ``test_gpu_small_loop_trips.py`` (``test_small_loop_trips_cpu.py`` vets them without a GPU): what the fused LDS loop does
behind its search barrier with its loads issued together.  A plain helper like ``small_loop_reduce_instances.py``: seeded, no
fixtures, every result computed once.

* ``side_plant``: planted cycles whose sides have (first, second) = (0, 1), (1, 0), (1, 1), (63, 64), (64, 64), (64, 65), (65, 1)
  tree arcs, under a join that hangs ``LIFT`` arcs deeper than ``planted_pivots`` hangs it, so that even a side of no arc at all
  has end points below depth 3 and goes through the node-parallel search, not the two-lane climb;
* ``mixed_plant``: one side narrow, the other holding a residual of 2^32 - 1 or more (the both-sides-at-once reduction must fall
  back to one reduction per side), both ways round; ``inf_plant``: one side of nothing but ``MCF_INF``;
* ``range_trace``: the positions of the preorder array that each pivot of an emulated solve moves, and how the ranges of
  consecutive swaps lie to each other -- what the apply pass's catch-up range gets to see."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import planted_pivots as pp
import small_loop_back_instances as bi
import small_loop_control_instances as ci
import small_loop_reduce_instances as ri
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

MCF_INF = ri.MCF_INF
NARROW_LIMIT = ri.NARROW_LIMIT
LIFT = 3                                 # tree arcs put between the top of the component and the join
SIDES = ((0, 1), (1, 0), (1, 1), (63, 64), (64, 64), (64, 65), (65, 1))
# (who ties with the leaving arc, the side that leaves by the documented rule)
TIES = (((), "first_side"), ((), "second_side"), (("first",), "first_side"), (("second",), "second_side"), (("first", "second"), "second_side"))
MIXED = (("first", 5, 7), ("second", 5, 7), ("first", 64, 64), ("second", 64, 64))   # (the wide side, arcs of the first side, of the second)
RANGE_STEPS = 40
RANGE_KINDS = ("disjoint", "nested", "overlap", "identical")


def _lifted_tree(orig, lift):
    """``planted_pivots._tree`` with a chain of `lift` nodes between the component's top and the join: labels stay preorder numbers."""
    def tree(*args):
        parent, role = orig(*args)
        n, j = len(parent), role["join"]
        assert 0 < j < n, "a join inside one component"
        top = int(parent[j])
        sh = lambda x: x + lift if x >= j else x
        par = np.full(n + lift, -1, np.int64)
        for x in range(n):
            par[sh(x)] = -1 if parent[x] < 0 else sh(int(parent[x]))
        for q in range(lift):
            par[j + q] = top if q == 0 else j + q - 1
        par[j + lift] = j + lift - 1
        out = {k: ([sh(x) for x in v] if isinstance(v, list) else (sh(v) if v >= 0 else v)) for k, v in role.items()}
        return par, out
    return tree


def deep_plant(**kw) -> pp.PivotPlant:
    """``pp.pivot_plant`` with the join ``LIFT`` arcs deeper (the generator's tree builder is wrapped for the call)."""
    orig = pp._tree
    pp._tree = _lifted_tree(orig, LIFT)
    try:
        return pp.pivot_plant(**kw)
    finally:
        pp._tree = orig


def _possible(n1, n2, ts, leave):
    mine, other = (n1, n2) if leave == "first_side" else (n2, n1)
    if mine < 1:
        return False                                         # the re-hung subtree's side holds the leaving arc
    me, oth = ("first", "second") if leave == "first_side" else ("second", "first")
    if me in ts and mine < 2:
        return False                                         # a further arc on that side that loses the tie
    return not (oth in ts and other < 1)


SIDE_CASES = [(n1, n2, ts, leave) for n1, n2 in SIDES for ts, leave in TIES if _possible(n1, n2, ts, leave)]
SIDE_IDS = [f"{n1}_{n2}-{leave}" + ("-ties_" + "_".join(ts) if ts else "") for n1, n2, ts, leave in SIDE_CASES]


@functools.lru_cache(maxsize=None)
def side_plant(n1: int, n2: int, ts: tuple, leave: str) -> pp.PivotPlant:
    """The re-hung subtree's side has stem + above + 1 tree arcs, the other side `other`."""
    mine, other = (n1, n2) if leave == "first_side" else (n2, n1)
    first = leave == "first_side"
    # a first-side arc that loses the tie lies above `a`, a second-side one below it
    above = min(2, mine - 1) if first else max(0, min(2, mine - 2))
    stem = mine - 1 - above
    return deep_plant(stem=stem, t2=stem + 6, other=other, above=above, leave=leave, ties=ts,
                      direction="after" if leave == "second_side" and other else "before", seed=23)


def trajectory(p: pp.PivotPlant):
    return bi._trajectory(p)


@functools.lru_cache(maxsize=None)
def side_trajectory(n1: int, n2: int, ts: tuple, leave: str):
    return trajectory(side_plant(n1, n2, ts, leave))


def first_pivot(p: pp.PivotPlant) -> dict:
    """What the ratio tests see at the planted pivot (``ri.TracedSimplex``): res1 / res2 by path index, deep, flip."""
    ref = ri.TracedSimplex(p.pl)
    assert ref.step()
    return ref.log[0]


def _with_residual(p: pp.PivotPlant, side: str, value: int, everywhere: bool, tag: str) -> pp.PivotPlant:
    """`p` with the spare capacity of tree arcs of `side` that GAIN flow at the planted pivot set to `value` (one arc, or every
    arc of the side, which then must all gain): flows, supplies and the leaving arc stay what they were."""
    ref = pp.RefSimplex(p)
    end = p.first if side == "first" else p.second
    nodes, x = [], end
    while x != p.join and x != ref.n:
        nodes.append(x)
        x = int(ref.parent[x])
    inst, pl = p.inst, p.pl
    cap = np.asarray(inst.cap, np.int64).copy()
    done = 0
    for x in nodes:
        e = int(pl.tree_arc[x])
        gains = (int(inst.tail[e]) == x) == (side == "second")          # second side: an up arc gains; first side: a down arc
        if e == p.leaving or not gains:
            assert not everywhere or e != p.leaving, "the leaving arc's side cannot be all MCF_INF"
            if everywhere:
                return None
            continue
        cap[e] = value if value >= MCF_INF else int(pl.flow[e]) + value
        done += 1
        if not everywhere:
            break
    if not done:
        return None
    ninst = ArcSoA(inst.n, inst.tail, inst.head, inst.cost, cap, inst.supply, inst.name + tag)
    return dataclasses.replace(p, pl=dataclasses.replace(pl, inst=ninst))


@functools.lru_cache(maxsize=None)
def mixed_plant(wide_side: str, n1: int, n2: int) -> pp.PivotPlant:
    """The planted swap leaves on the NARROW side; the other side holds one residual of 2^32 + 5."""
    leave = "second_side" if wide_side == "first" else "first_side"
    for seed in range(60, 90):
        mine, other = (n1, n2) if leave == "first_side" else (n2, n1)
        base = deep_plant(stem=mine - 3, t2=mine + 3, other=other, above=2, leave=leave,
                          direction="after" if leave == "second_side" else "before", seed=seed)
        p = _with_residual(base, wide_side, (1 << 32) + 5, False, f"_wide_{wide_side}")
        if p is not None:
            return p
    raise AssertionError("no arc of that side gains flow")


@functools.lru_cache(maxsize=None)
def inf_plant(inf_side: str) -> pp.PivotPlant:
    """Every arc of one side uncapacitated and gaining flow: a side of nothing but ``MCF_INF``; the swap leaves on the other."""
    leave = "second_side" if inf_side == "first" else "first_side"
    for seed in range(60, 400):
        base = deep_plant(stem=2, t2=8, other=3, above=2, leave=leave, direction="after" if leave == "second_side" else "before", seed=seed)
        p = _with_residual(base, inf_side, MCF_INF, True, f"_inf_{inf_side}")
        if p is not None:
            return p
    raise AssertionError("no seed whose side gains flow on every arc")


# ------------------------------------------------------------------ moved ranges of consecutive swaps
@functools.lru_cache(maxsize=None)
def range_instance(which: str) -> ArcSoA:
    """netgen_513: moved ranges beyond 192 and 256 positions in front of further swaps; netgen_41: two consecutive swaps that move
    the identical range (pivots 37 and 38)."""
    return {"netgen_513": lambda: generators.netgen_style(513, 1026, seed=5), "netgen_41": lambda: generators.netgen_style(40, 160, seed=3)}[which]()


def relation(a, b) -> str:
    if a == b:
        return "identical"
    if a[1] <= b[0] or b[1] <= a[0]:
        return "disjoint"
    if (a[0] <= b[0] and b[1] <= a[1]) or (b[0] <= a[0] and a[1] <= b[1]):
        return "nested"
    return "overlap"


@functools.lru_cache(maxsize=None)
def range_trace(which: str, steps: int = RANGE_STEPS):
    """[(pivot, previous range, this range, relation)] over the first `steps` pivots of the emulated Dantzig solve: a range is
    [first, last + 1) of the preorder positions whose node the pivot changed (a bound flip changes none and is passed over -- the
    catch-up range survives it)."""
    inst = range_instance(which)
    out, prev_order, last = [], None, None
    for k in range(steps + 1):
        order = np.asarray(ci.emul(inst, 0, k)["order"])
        if prev_order is not None:
            d = np.flatnonzero(order != prev_order)
            if len(d):
                cur = (int(d[0]), int(d[-1]) + 1)
                if last is not None:
                    out.append((k, last, cur, relation(last, cur)))
                last = cur
        prev_order = order
    return out
