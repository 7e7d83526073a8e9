"""Every verdict of the engine's integer logic with uncapacitated arcs in play, on the CPU (``-m "not gpu"``).

The CPU emulation (oracle/emul_engine.cpp) runs the very headers the kernels are compiled from; here it is held to
networkx on Python ints and to the certificates of ``verdict_instances`` on all four families -- uncapacitated (optimal),
unbounded, infeasible, deep_unbounded -- so that ``tests/test_gpu_verdicts.py`` can hold the kernels to the emulation.  The
coverage the GPU file relies on (uncapacitated arcs basic at the end, every encoding of "uncapacitated" and the bound
2^60 - 1 on pivot cycles, a verdict on a non-planted arc, a verdict pivot that goes through the scan) is asserted here.
Every comparison is exact."""

import functools

import numpy as np
import pytest

import oracle
import verdict_instances as vi
import wide_range_instances as wri
from conftest import check_tree_invariants

RULES = [0, 1, 2]
# bits 16-19 of `rule`: log2 of the block size of the blocked preorder list, bits 20-31: spare blocks + 1 (0 = auto)
BLOCKED = {"shift2_pool0": 2 << 16, "shift3_pool5": (3 << 16) | (6 << 20)}
STATE_KEYS = ("flow", "potential", "in_tree", "parent", "pred_arc", "order", "depth")


def _emul(inst, rule, **kw):
    kw.setdefault("climb_budget", 0)
    return oracle.emul_solve(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule, **kw)


def _rc(inst, r, arc):
    return int(inst.cost[arc]) + int(r["potential"][inst.tail[arc]]) - int(r["potential"][inst.head[arc]])


def check_verdict(inst, want, r):
    """Outcome class + the yardstick of that class; returns the length of the verdict cycle (unbounded) or 0."""
    assert r["status"] == want, (inst.name, r["status"])
    check_tree_invariants(inst.n, r["parent"], r["size"], r["pos"], r["order"], r["depth"], r["psize"])
    if want == "optimal":
        assert r["unbounded_arc"] == -1 and r["artificial_flow"] == 0
        assert wri.exact_certificate(inst, r["flow"], r["potential"]) == r["objective"]
        return 0
    if want == "unbounded":
        return vi.unbounded_certificate(inst, r, r["unbounded_arc"], _rc(inst, r, r["unbounded_arc"]))
    assert r["unbounded_arc"] == -1
    vi.check_infeasible(inst, r["objective"], r["artificial_flow"], r)
    return 0


def _family(seed, n, m):
    yield vi.uncapacitated(seed, n, m), "optimal", 0
    length = (2, 5, min(n, vi.PATH_BUFFER_CYCLE))[seed % 3]
    yield vi.unbounded(seed, n, m, length), "unbounded", length
    for variant in vi.INFEASIBLE_VARIANTS:
        yield vi.infeasible(seed, n, m, variant), "infeasible", 0


def _against_networkx(seed, n, m):
    for inst, want, _ in _family(seed, n, m):
        assert vi.networkx_verdict(inst) == want, inst.name
        truth = wri.networkx_objective(inst) if want == "optimal" else None
        for rule in RULES:
            r = _emul(inst, rule)
            check_verdict(inst, want, r)
            if want == "optimal":
                assert r["objective"] == truth, (inst.name, rule)


@pytest.mark.parametrize("seed", range(20))
def test_emulation_equals_networkx_on_every_verdict(seed):
    """60 nodes / 500 + 60 arcs, 40 % of the arcs of cost >= 0 uncapacitated: outcome class as networkx sees it; the optimum
    equal to networkx's; the unbounded verdict's cycle all forward, uncapacitated, of the reported cost < 0; the
    infeasible verdict's artificial flow the least possible and its state optimal for what the engine still holds."""
    _against_networkx(seed, *vi.SIZES["small"])


@pytest.mark.slow
@pytest.mark.parametrize("seed", range(3))
def test_emulation_equals_networkx_on_every_verdict_at_1024_nodes(seed):
    _against_networkx(seed, *vi.SIZES["medium"])


def test_deep_unbounded_ends_on_a_scanned_pivot():
    """The chain instance: n - 1 pivots, then the verdict on the return arc, whose cycle is the whole chain -- found by the
    position-space scan (the emulation counts the verdict pivot in `scans` though not in `pivots`)."""
    for n in (48, 300):
        inst = vi.deep_unbounded(n)
        assert vi.networkx_verdict(inst) == "unbounded"
        for rule in RULES:
            r = _emul(inst, rule)
            assert r["status"] == "unbounded" and r["pivots"] == n - 1 and r["unbounded_arc"] == n - 1
            assert r["scans"] == r["pivots"] + 1
            assert check_verdict(inst, "unbounded", r) == n
            climbed = _emul(inst, rule, climb_budget=-1)
            assert climbed["scans"] == 0 and climbed["unbounded_arc"] == n - 1 and climbed["pivots"] == n - 1


# ------------------------------------------------------------------ what the GPU file relies on
@functools.lru_cache(maxsize=None)
def _gpu_instances(size):
    return vi.gpu_instances(size)


@pytest.mark.parametrize("size", ["small", pytest.param("medium", marks=pytest.mark.slow)])
def test_the_gpu_instances_have_their_verdicts_and_uncapacitated_arcs_in_the_basis(size):
    nonplanted = 0
    for name, (inst, want, length) in _gpu_instances(size).items():
        for rule in RULES:
            r = _emul(inst, rule)
            check_verdict(inst, want, r)
            assert (vi.is_uncapacitated(inst.cap) & (r["in_tree"] == 1)).sum() > 0, (name, rule)
            assert r["pivots"] > (40 if name != "deep_unbounded" else 0)          # the verdict comes deep into the solve
            if want == "unbounded" and length and r["unbounded_arc"] < inst.m - length:
                nonplanted += 1
    # The reported arc need not be a planted one: it only has to close a free cycle.  At 60 nodes every verdict of these
    # instances does land on a planted arc, so this condition is met by the 1 024-node case alone, which is marked slow: it
    # holds in a run that includes the slow tests (the default here), not under -m "not slow".
    if size == "medium":
        assert nonplanted > 0


def test_every_encoding_and_the_largest_bound_meet_the_ratio_test():
    """Over the 60-node GPU instances, Dantzig rule: the cycle of every pivot (entering arcs from the emulation's trace,
    the tree before pivot k from the state cut at max_pivots = k) -- arcs encoded -1, 2^60, 2^62, INT64_MAX and arcs
    bounded by 2^60 - 1 all occur on such cycles, next to ordinary capped arcs."""
    seen = dict.fromkeys(vi.FAR + (vi.EDGE_CAP, "capped"), 0)
    for name, (inst, want, _) in _gpu_instances("small").items():
        whole = _emul(inst, 0, trace=4096)
        entering = whole["trace"][: whole["pivots"] + (want == "unbounded")]
        assert (entering >= 0).all() and len(entering) < 4096
        for k in range(0, len(entering), 3):
            state = _emul(inst, 0, max_pivots=k)
            assert state["pivots"] == k and state["in_tree"][entering[k]] == 0
            for a, _ in vi.cycle_of(inst, state["parent"], state["pred_arc"], int(entering[k])):
                if a < inst.m:
                    cp = int(inst.cap[a])
                    seen[cp if cp in seen else "capped"] += 1
    assert all(seen.values()), seen


@pytest.mark.parametrize("layout", list(BLOCKED))
def test_blocked_list_gives_the_same_verdict_pivot_count_and_state(layout):
    for name, (inst, want, _) in _gpu_instances("small").items():
        for rule in RULES:
            dense, blocked = _emul(inst, rule), _emul(inst, rule | BLOCKED[layout])
            assert blocked["status"] == dense["status"] == want
            for key in ("pivots", "degenerate", "unbounded_arc", "artificial_flow", "objective", "scans"):
                assert blocked[key] == dense[key], (name, rule, key)
            for key in STATE_KEYS:
                assert np.array_equal(blocked[key], dense[key]), (name, rule, key)
