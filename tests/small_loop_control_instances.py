"""Inputs of ``test_gpu_small_loop_control.py`` (``test_small_loop_control_cpu.py`` vets them without a GPU): what the fused LDS
loop keeps in registers across a launch has to survive the launch boundary, and iterations that pivot on nothing have to stay
uniform over the workgroup.  A plain helper like ``small_loop_instances.py``: seeded, no fixtures, every result computed once."""

from __future__ import annotations

import functools

import numpy as np

import oracle
import small_loop_instances as sl
import verdict_instances as vi
from network_flow_solver_amd.generators import ArcSoA, netgen_style

CHOP_STEPS = (1, 2, 3, 7)                # pivots per launch of the chopped solves
CHOP_SHAPES = ((257, 1028), (64, 512))
DEVEX_BLOCK = 16                         # arcs per Devex block on netgen(64, 512): blocks without a candidate on the way
# every statistic mcf_stats exposes that the loop accumulates in registers (minor_pivots / major_sweeps are not exposed:
# arcs_priced -- eight per minor iteration, a whole sweep per major one -- moves with both)
STATS = ("pivots", "degenerate", "bound_flips", "arcs_priced", "cycle_arcs", "subtree_nodes", "nodes_moved")


def emul(inst, rule: int, max_pivots: int = -1, block_size: int = 0) -> dict:
    return _emul(_key(inst), rule, max_pivots, block_size)


_INSTANCES: dict = {}


def _key(inst):
    _INSTANCES.setdefault(inst.name, inst)
    return inst.name


@functools.lru_cache(maxsize=None)
def _emul(key, rule, max_pivots, block_size):
    i = _INSTANCES[key]
    return oracle.emul_solve(i.n, i.tail, i.head, i.cost, i.cap, i.supply, rule=rule, max_pivots=max_pivots, block_size=block_size)


@functools.lru_cache(maxsize=None)
def capped_transport() -> ArcSoA:
    """``sl.transport(1024)`` with every capacity cut to 1 .. 3: bound flips and degenerate pivots under every rule."""
    t = sl.transport(1024)
    cap = np.random.default_rng(7).integers(1, 4, t.m).astype(np.int64)
    return ArcSoA(t.n, t.tail, t.head, t.cost, cap, t.supply, "transport_first_bucket_1024_caps_1_3")


@functools.lru_cache(maxsize=None)
def optimal_at_start() -> ArcSoA:
    """``sl.netgen(64, 512)`` without supplies and with costs >= 1: the start basis is optimal, no pivot."""
    b = sl.netgen(64, 512)
    return ArcSoA(b.n, b.tail, b.head, np.abs(b.cost) + 1, b.cap, np.zeros(b.n, np.int64), "netgen_64_512_no_supply")


def verdict_cases() -> dict:
    """name -> (instance, verdict): the small unbounded / infeasible instances of the verdict tests."""
    g = vi.gpu_instances("small")
    return {k: (g[k][0], g[k][1]) for k in ("unbounded_5", "deep_unbounded", "starved", "cut")}


# ------------------------------------------------------------------ the LDS plan (small_plan of csrc/mcf_engine.hip)
def lds_total(n: int, m: int, devex: bool = True) -> tuple[int, int]:
    """(estimate, sum of the 16-byte-rounded pieces) for n nodes + the root and m arcs; the control block counted as 1 KiB."""
    m_pad = (m + 1023) // 1024 * 1024
    nn, arcw = n + 1, m + n
    r = lambda b: (b + 15) // 16 * 16
    scratch = r(nn * 20) if nn <= 1024 else 0
    total = (4 + devex) * r(m_pad * 4) + r(m_pad) + r(arcw * 16) + r(nn * 8) + 3 * r(nn * 16) + 8 * r(nn * 4) + r((2 * nn + 2) * 16) + scratch + 1024
    return m_pad * 21 + arcw * 16 + nn * 112 + 4096, total


def fits_lds(n: int, m: int, devex: bool = True) -> bool:
    need, total = lds_total(n, m, devex)
    return need < 150 * 1024 and total <= 156 * 1024


@functools.lru_cache(maxsize=None)
def largest_tree():
    """The netgen-style instance with the most nodes that still fits the plan with m = n + n // 8 arcs (the generator wants a
    few more arcs than nodes), Devex weights included -- found by walking down from 1 100 nodes."""
    for n in range(1100, 256, -1):
        if fits_lds(n, n + n // 8):
            return netgen_style(n, n + n // 8, seed=5)
    raise AssertionError("unreachable")
