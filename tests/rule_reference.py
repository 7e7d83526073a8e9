"""The state of the Devex and candidate-list pricing rules, restated in plain Python from the written rule (``DESIGN.md`` section 4,
"State of the pricing rules"; ``include/mcf.h``, "Pricing rules").  A plain helper like ``planted_pivots.py``: numpy and Python
ints, no fixtures; it imports neither ``oracle`` nor the engine, loads no shared library and shares no code with
``csrc/mcf_core.h``.  The pivot itself -- cycle, ratio test, leaving arc, tree -- is ``RefSimplex.pivot``; what is added here is
everything that decides WHICH arc enters next, and the counters a caller can read back (``arcs_priced``, ``minor_pivots``,
``major_sweeps``, the Devex weights).

Every quantity is an integer except the Devex merit, which is ``viol * viol / w`` in IEEE double on operands that are exact in
that format (violations below 2^46, weights small integers held in float32): the comparisons are exact, no tolerance exists."""

from __future__ import annotations

import numpy as np

from planted_pivots import RefSimplex

NUM_BUCKETS = 8            # head buckets
GRANULES = 64              # granules per bucket
WLIST_CAP = 1024           # weights that may differ from 1 between two resets
RESET_SWAPS = 64           # basis swaps between two resets
TUNER_MAX_ARCS = 16384     # the tuner grows a block to at most this many arcs (never below the start size)
TUNER_PERIOD = 50


def engine_order(inst):
    """(perm, bucket_off): engine arc e is the caller's arc perm[e]; bucket x holds the engine arcs bucket_off[x] .. bucket_off[x + 1].
    Arcs are bucketed by head // ceil(n / 8) and ordered by tail inside a bucket, equal tails in the caller's order."""
    per = (inst.n + NUM_BUCKETS - 1) // NUM_BUCKETS
    bucket = np.asarray(inst.head, np.int64) // per
    perm = np.lexsort((np.asarray(inst.tail, np.int64), bucket))          # stable: last key first, then tail, then index
    off = np.searchsorted(bucket[perm], np.arange(NUM_BUCKETS + 1))
    return perm.astype(np.int64), [int(x) for x in off]


def granule_table(bucket_off):
    """gran[x][g]: the engine arc at which granule g of bucket x starts, g = 0 .. 64 (granule g = the g-th 64th of every bucket)."""
    return [[bucket_off[x] + (bucket_off[x + 1] - bucket_off[x]) * g // GRANULES for g in range(GRANULES + 1)] for x in range(NUM_BUCKETS)]


def auto_block_size(m: int) -> int:
    return max(m // 4 if m < 1000 else (m // 8 if m < 10000 else m // 16), 1)


def granules_for(block_size: int, m: int) -> int:
    return min(max((block_size * GRANULES + m // 2) // m, 1), GRANULES) if m > 0 else GRANULES


class DevexRef(RefSimplex):
    """Block search with merit viol^2 / w.  ``block_size`` <= 0: automatic; ``tuner``: 0 on exactly when the block size is
    automatic, 1 on, -1 off; ``stay``: keep to a block until it holds no eligible arc (else the next block after every pivot).
    ``events``: (pivot number, what) for every reset ("reset" / "early_reset"), tuner step ("tuner"), wrap of the block index
    by a tuner step ("wrap") and tie between the directions ("direction_tie"); ``pass_log``: (block, granules, arcs, found) of every pricing pass; ``direction_ties``: the pivots
    whose largest merit a forward and a backward arc shared."""

    def __init__(self, pp_or_pl, block_size: int = 0, tuner: int = 0, stay: bool = False):
        super().__init__(pp_or_pl)
        inst = getattr(pp_or_pl, "pl", pp_or_pl).inst
        m = self.m
        self.perm, self.bucket_off = engine_order(inst)
        self.gran = granule_table(self.bucket_off)
        self.auto_tune = tuner > 0 or (tuner == 0 and block_size <= 0)
        self.stay = bool(stay)
        self.block_granules = granules_for(block_size if block_size > 0 else auto_block_size(m), m)
        self.num_blocks = -(-GRANULES // self.block_granules)
        self.max_granules = max(self.block_granules, min(GRANULES, TUNER_MAX_ARCS * GRANULES // m if m > 0 else GRANULES))
        self.block_index = 0
        self.empty_blocks = 0
        self.weights = np.ones(m, np.float32)                     # caller's order
        self.touched = 0                                          # weights set since the last reset (an arc counts every time)
        self.swaps = 0
        self.tn_total = self.tn_degenerate = self.tn_last = 0
        self.arcs_priced = 0
        self.events, self.pass_log, self.direction_ties = [], [], []
        self.just_reset = False

    def block_arcs(self, k: int):
        """Caller's indices of the arcs of block k."""
        g0 = k * self.block_granules
        g1 = min(g0 + self.block_granules, GRANULES)
        return np.concatenate([self.perm[self.gran[x][g0]:self.gran[x][g1]] for x in range(NUM_BUCKETS)])

    def select(self) -> int:
        while True:
            arcs = self.block_arcs(self.block_index)
            self.arcs_priced += len(arcs)
            viol = (-self.state * self.reduced_costs())[arcs]
            ok = viol > 0
            self.pass_log.append((self.block_index, self.block_granules, len(arcs), bool(ok.any())))
            if not ok.any():
                self.empty_blocks += 1
                self.block_index = (self.block_index + 1) % self.num_blocks
                if self.empty_blocks >= self.num_blocks:
                    return -1
                continue
            cand, v = arcs[ok], viol[ok].astype(np.float64)
            merit = v * v / self.weights[cand].astype(np.float64)
            ties = cand[merit == merit.max()]
            backward = ties[self.state[ties] < 0]                  # forward wins only when strictly greater
            if 0 < len(backward) < len(ties):
                self.direction_ties.append(self.pivots + 1)
                self.events.append((self.pivots + 1, "direction_tie"))
            e = int(backward.min()) if len(backward) else int(ties.min())
            self.empty_blocks = 0
            if not self.stay:
                self.block_index = (self.block_index + 1) % self.num_blocks
            return e

    def pivot(self, e: int) -> bool:
        super().pivot(e)
        reset = False
        if not self.flip:                                          # a bound flip is no basis swap
            if self.swaps >= RESET_SWAPS:
                reset, self.swaps = True, 0
                self.events.append((self.pivots, "reset"))
            else:
                self.swaps += 1
        if not reset:
            if self.touched >= WLIST_CAP:
                reset = True
                self.events.append((self.pivots, "early_reset"))
            else:
                self.weights[e] = np.float32(max(self.cycle_len - 1, 1))   # tree arcs on the cycle
                self.touched += 1
        self.just_reset = reset
        if reset:
            self.weights[:] = 1
            self.touched = 0
            self.block_index = 0
        self.tn_total += 1
        if self.theta == 0 or self.flip:
            self.tn_degenerate += 1
        if self.auto_tune and self.pivots - self.tn_last >= TUNER_PERIOD and self.tn_total >= 10:
            bg = self.block_granules
            if 10 * self.tn_degenerate > 3 * self.tn_total:
                bg = max(bg, min(max(bg * 3 // 2, bg + 1), self.max_granules))
            elif 10 * self.tn_degenerate < self.tn_total:
                bg = max(bg * 3 // 4, 1)
            if bg != self.block_granules:
                self.block_granules = bg
                self.num_blocks = -(-GRANULES // bg)
                self.events.append((self.pivots, "tuner"))
                if self.block_index >= self.num_blocks:
                    self.block_index = 0
                    self.events.append((self.pivots, "wrap"))
            self.tn_total = self.tn_degenerate = 0
            self.tn_last = self.pivots
        return True


def list_geometry(price_blocks: int):
    """(pricing workgroups per bucket, list length, minor pivots per sweep) for a requested number of pricing workgroups."""
    nlb = min(max((price_blocks + 7) // 8, 1), 2048 // NUM_BUCKETS)
    return nlb, nlb * NUM_BUCKETS, min(max(nlb, 3), 32)


class CandidateListRef(RefSimplex):
    """A full Dantzig sweep keeps the best arc of every pricing workgroup; the next ``minor_cap`` pivots re-price that list only.
    A listed arc that is basic by then, or no longer eligible, is passed over.  ``periods``: per full sweep that found an arc,
    [minor pivots taken, "full" / "emptied" / "open", a listed arc was basic when the list was re-priced, a listed non-basic arc
    was no longer eligible then]; ``events``: (pivot number, "period_end") at the last pivot of every period."""

    def __init__(self, pp_or_pl, price_blocks: int = 8):
        super().__init__(pp_or_pl)
        inst = getattr(pp_or_pl, "pl", pp_or_pl).inst
        self.perm, self.bucket_off = engine_order(inst)
        self.nlb, self.list_len, self.minor_cap = list_geometry(price_blocks)
        e = np.arange(self.m, dtype=np.int64)
        x = np.searchsorted(np.asarray(self.bucket_off[1:]), e, side="right")
        first_group = np.asarray(self.bucket_off, np.int64)[x] >> 2
        group_e = (((e >> 2) - first_group) >> 8) % self.nlb * NUM_BUCKETS + x
        self.group = np.empty(self.m, np.int64)                   # caller's arc -> pricing workgroup
        self.group[self.perm] = group_e
        self.listed = np.zeros(0, np.int64)
        self.minor_left = 0
        self.minor_pivots = self.major_sweeps = self.arcs_priced = 0
        self.periods, self.events = [], []

    @staticmethod
    def _best(arcs, viol):
        """The largest violation, ties to the lowest caller's index; -1 when none is positive."""
        if not len(arcs) or viol.max() <= 0:
            return -1
        return int(arcs[viol == viol.max()].min())

    def select(self) -> int:
        while True:
            viol = -self.state * self.reduced_costs()
            if self.minor_left > 0:
                self.arcs_priced += self.list_len
                if (self.state[self.listed] == 0).any():
                    self.periods[-1][2] = True
                if ((self.state[self.listed] != 0) & (viol[self.listed] <= 0)).any():
                    self.periods[-1][3] = True
                e = self._best(self.listed, viol[self.listed])
                if e < 0:                                          # says nothing about optimality: sweep again
                    self.minor_left = 0
                    self.periods[-1][1] = "emptied"
                    self.events.append((self.pivots, "period_end"))
                    continue
                self.minor_left -= 1
                self.minor_pivots += 1
                self.periods[-1][0] += 1
                if self.minor_left == 0:
                    self.periods[-1][1] = "full"
                    self.events.append((self.pivots + 1, "period_end"))
                return e
            self.major_sweeps += 1
            self.arcs_priced += self.m
            e = self._best(np.arange(self.m), viol)
            if e < 0:
                return -1
            ok = np.flatnonzero(viol > 0)
            by = ok[np.lexsort((ok, -viol[ok], self.group[ok]))]   # per workgroup: largest violation, then lowest index
            self.listed = by[np.r_[True, self.group[by][1:] != self.group[by][:-1]]]
            self.minor_left = self.minor_cap
            self.periods.append([0, "open", False, False])
            return e
