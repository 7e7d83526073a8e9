"""Inputs of ``test_gpu_small_loop_slots.py`` (``test_small_loop_slots_cpu.py`` vets them without a GPU): what the front kernel of the
fused LDS loop does differently once it is budgeted in issue slots -- a register sweep whose violation needs no compare, dealt over
two accumulators per lane, and a pick that reads the waves' slots whole.  A plain helper like ``small_loop_trips_instances.py``:
seeded, no fixtures, every result computed once.

All instances here are circulations -- no supplies, so every one is feasible and the start basis has every potential equal: at the
first sweep an arc's reduced cost IS its cost, every real arc is at zero flow (state +1), and an arc is eligible exactly when its cost
is negative.  That makes the first pivot plantable by costs alone.

* ``arc_count(m)``: m arcs over 48 nodes, m around the lane count (1, 255 .. 257), around the switch from the 8-slot to the 10-slot
  sweep (2 047 .. 2 049) and one past the register slots (2 561: the first arc priced from LDS);
* ``tie(kind, order)``: 2 048 arcs in engine order, two of them tied on the largest violation -- in two slots of one accumulator of
  a lane, in its two accumulators, in two lanes of a wave, in waves 0 and 3, in waves 1 and 2 -- with the caller's ids of the two
  ascending or descending along the engine order (the lower id wins either way);
* ``last_slot()``: the only eligible arc in the last slot of the last lane of wave 3; ``nothing()``: no eligible arc at all;
* ``states()``: capacities 1 .. 2 and many negative cycles, so that arcs sit at capacity: both states with either sign of the
  reduced cost in the sweeps, and arcs of either state entering, within the 100 pivots compared;
* ``limit()``: ``small_loop_front_instances.edge(0)``, the instance whose reduced-cost bound is the narrow limit 2^31 - 1;
* ``counter_run(which)``: netgen-style 64 / 512 and 40 / 160 (seed 3) and the verdict tests' ``deep_unbounded``, solved in resumed
  launches: between them bound flips, degenerate pivots and an unbounded verdict."""

from __future__ import annotations

import functools

import numpy as np

import planted_pivots as pp
import rule_reference as rr
import small_loop_decide_instances as di
import small_loop_front_instances as fi
from network_flow_solver_amd.generators import ArcSoA

LANES = 256                              # the width the changed code is compiled for (small_price_flat, small_pick_one_trip)
REG_FEW, REG = 8, 10                     # small_reg_arcs_few / small_reg_arcs at that width
CHAINS = 2                               # small_price_chains
ARC_COUNTS = (1, 255, 256, 257, REG_FEW * LANES - 1, REG_FEW * LANES, REG_FEW * LANES + 1, REG * LANES + 1)
COUNT_NODES = 48
COUNT_STEPS = 6
TIE_NODES, TIE_ARCS = 64, REG_FEW * LANES
# engine positions (e1 < e2) of the two tied arcs; lane = e % 256, slot = e // 256, wave = lane // 64, accumulator = slot % 2
TIES = {
    "slots_of_one_accumulator": (17, 17 + 2 * LANES),
    "accumulators_of_one_lane": (17, 17 + LANES),
    "lanes_of_one_wave": (5 + LANES, 40 + LANES),
    "waves_0_and_3": (200, 3 + 3 * LANES),
    "waves_1_and_2": (70, 130 + 4 * LANES),
}
ORDERS = ("ascending", "descending")
TIE_STEPS = 3
STATES_STEPS = 100                       # entering arcs at capacity from the 74th pivot on (118 in all)
LIMIT_STEPS = 8
COUNTER_CAPS = (1, 2, 7)                 # pivots per launch of the resumed solves
# name -> (how the solve ends, holds bound flips, holds degenerate pivots): the stepped netgen-style instances of the decide tests and
# the verdict tests' unbounded instance whose cycle is met behind 46 degenerate swaps
COUNTER_RUNS = {"netgen_64_512": ("optimal", True, True), "netgen_40_160": ("optimal", True, True), "deep_unbounded": ("unbounded", False, True)}


def _arcs(n, m, rng):
    tail = rng.integers(0, n, m)
    head = (tail + rng.integers(1, n, m)) % n
    return tail.astype(np.int32), head.astype(np.int32)


@functools.lru_cache(maxsize=None)
def arc_count(m: int) -> ArcSoA:
    """Costs -20 .. 20, capacities 1 .. 3; arc 0 costs -21: at least one pivot, whatever m."""
    rng = np.random.default_rng([48, m])
    tail, head = _arcs(COUNT_NODES, m, rng)
    cost = rng.integers(-20, 21, m).astype(np.int64)
    cost[0] = -21
    return ArcSoA(COUNT_NODES, tail, head, cost, rng.integers(1, 4, m).astype(np.int64), np.zeros(COUNT_NODES, np.int64), f"circulation_48_{m}")


def _sorted_arcs(seed):
    """TIE_ARCS arcs over TIE_NODES nodes already in engine order: the caller's index of an arc is its engine index."""
    rng = np.random.default_rng(seed)
    tail, head = _arcs(TIE_NODES, TIE_ARCS, rng)
    per = (TIE_NODES + rr.NUM_BUCKETS - 1) // rr.NUM_BUCKETS
    by = np.lexsort((tail, head // per))
    return tail[by], head[by], rng.integers(0, 10, TIE_ARCS).astype(np.int64)


def _planted(name, eligible: dict, swap=None) -> ArcSoA:
    tail, head, cost = _sorted_arcs(81)
    for e, c in eligible.items():
        cost[e] = c
    if swap is not None:
        # the two arcs' ids descend along the engine order: their whole groups of equal sort key (head bucket, tail) change places
        # in the CALLER's order -- inside a group the engine keeps the caller's order, so every engine position stays what it was
        a, b = swap
        per = (TIE_NODES + rr.NUM_BUCKETS - 1) // rr.NUM_BUCKETS
        key = (head // per).astype(np.int64) * TIE_NODES + tail
        ga, gb = np.flatnonzero(key == key[a]), np.flatnonzero(key == key[b])
        assert a < b and key[a] != key[b] and ga[-1] < gb[0]
        caller = np.concatenate((np.arange(ga[0]), gb, np.arange(ga[-1] + 1, gb[0]), ga, np.arange(gb[-1] + 1, TIE_ARCS)))
        tail, head, cost = tail[caller], head[caller], cost[caller]
    return ArcSoA(TIE_NODES, tail, head, cost, np.full(TIE_ARCS, 3, np.int64), np.zeros(TIE_NODES, np.int64), name)


@functools.lru_cache(maxsize=None)
def tie(kind: str, order: str) -> ArcSoA:
    e1, e2 = TIES[kind]
    return _planted(f"tie_{kind}_{order}", {e1: -7, e2: -7}, swap=(e1, e2) if order == "descending" else None)


@functools.lru_cache(maxsize=None)
def last_slot() -> ArcSoA:
    return _planted("only_arc_in_the_last_slot", {TIE_ARCS - 1: -7})


@functools.lru_cache(maxsize=None)
def nothing() -> ArcSoA:
    return _planted("nothing_eligible", {})


@functools.lru_cache(maxsize=None)
def states() -> ArcSoA:
    rng = np.random.default_rng(29)
    n, m = 24, 160
    tail, head = _arcs(n, m, rng)
    return ArcSoA(n, tail, head, rng.integers(-20, 21, m).astype(np.int64), rng.integers(1, 3, m).astype(np.int64), np.zeros(n, np.int64),
                  "circulation_24_160_caps_1_2")


def limit() -> ArcSoA:
    return fi.edge(0)


def counter_run(which: str) -> ArcSoA:
    return {"netgen_64_512": lambda: di.stepped(64, 512), "netgen_40_160": lambda: di.stepped(40, 160),
            "deep_unbounded": lambda: di.unbounded("deep_unbounded")}[which]()


# ------------------------------------------------------------------ what the CPU file checks them with
def engine_slot(inst, arc: int) -> dict:
    """Where the even deal of the 256-lane front kernel puts the caller's arc: engine index, lane, slot, wave, accumulator."""
    perm, off = rr.engine_order(inst)
    e = int(np.flatnonzero(perm == arc)[0]) - off[0]
    lane, slot = e % LANES, e // LANES
    return dict(engine=e, lane=lane, slot=slot, wave=lane // 64, chain=slot % CHAINS)


@functools.lru_cache(maxsize=None)
def sweeps(name_key, steps: int):
    """[(violations by caller's arc, states, reduced costs, entering arc)] of the first `steps` sweeps of the independent reference
    from the start basis (``planted_pivots.RefSimplex``: Dantzig, the lowest id among the largest violations)."""
    inst = _BY_NAME[name_key]
    ref = pp.RefSimplex(pp.cold_plant(inst))
    out = []
    for _ in range(steps):
        rc, st = ref.reduced_costs().copy(), ref.state.copy()
        e = ref.select()
        out.append((-st * rc, st, rc, e))
        if e < 0 or not ref.pivot(e):
            break
    return out


_BY_NAME: dict = {}


def trace(inst, steps: int):
    _BY_NAME.setdefault(inst.name, inst)
    return sweeps(inst.name, steps)
