"""Seeded sessions of mixed edits, queries and partial solves on one resident handle (``-m gpu``).

One test per (family, rule): it runs that pair's seeds through ``session_model.run_seeds`` -- every step checked against
references that know nothing of the handle's history, the end of every session against a fresh handle, pivot for pivot --
and asserts that the union of the seeds' events holds every event of ``session_model.EVENTS``.  The same seed lists run on
the CPU stand-in in ``tests/test_session_cpu.py``.  A failure prints the script so far for ``session_model.run_script``.

Families and sizes are the smallest at which each engine path exists (``FAMILIES`` of ``tests/test_gpu_add_arcs.py``; the
1024-lane LDS loop through ``MCF_SMALL_THREADS``).

A handle that gives its resident reduced costs up (``tree_blocks=4, rc_drop=1``) runs at 3 000 nodes / 24 000 arcs, the size of
``test_handle_that_dropped_its_reduced_costs``: the engine looks at the re-hung subtree sizes once per 4 096 pivots and a
1 000-node instance is solved in about 2 400, so at 1 000 / 8 000 no solve can report ``rc_dropped_at > 0``.  Under Devex and
the candidate list, as in that test.  At this size a reference verdict costs seconds, so each rule's session is split into
two tests (``RC_DROP_BLOCKS``) that start with a solve from the cold start to the end -- it must report
``rc_dropped_at > 0`` -- and together realise every event; each asserts its own share."""

from __future__ import annotations

import pytest

import session_model as sm

FAMILIES = ("lds", "lds_1024", "mid", "graph", "blocked", "keycodes", "gather")
# an even and an odd seed: the two halves of the agenda (session_model.HALVES); the small paths take a second pair
SEEDS = {f: (1, 2, 3, 4) if f in ("lds", "lds_1024") else (1, 2) for f in FAMILIES}
CASES = [(f, r) for f in FAMILIES for r in sm.RULES]
# (family, base step, blocks): a handle created with no arcs -- everything arrives through add_arcs -- and one that starts infeasible
# the two shares of a dropped-reduced-costs session: (blocks, events that share must realise)
RC_DROP_BLOCKS = {
    "ranges": (("drop_start", "first_range", "past", "supply", "grow_short"),
               ("cost_inside", "cost_past", "rhs_path0", "rhs_path1", "edit_after_repair", "pad_crossing", "range_add_range", "set_basis_after_add")),
    "verdicts": (("drop_start", "caps_bigm", "infeasible", "unbounded", "reset_limit"),
                 ("cap_zero_with_flow", "bigm_by_costs", "bigm_by_add", "infeasible_and_back", "unbounded_and_back", "reset_then_solve",
                  "edit_on_limit")),
}
assert sorted(e for _, ev in RC_DROP_BLOCKS.values() for e in ev) == sorted(sm.EVENTS)
RC_DROP_CASES = [(share, r) for share in RC_DROP_BLOCKS for r in ("devex", "candidate")]
SHORT_SESSIONS = (
    ("empty", {"op": "base", "kind": "empty", "n": 60, "m": 300, "seed": 4}, ("arrive", "first_range", "past", "reset")),
    ("infeasible", {"op": "base", "kind": "infeasible", "n": 60, "m": 500, "seed": 3}, ("starts_infeasible", "first_range", "reset")),
)


@pytest.mark.gpu
@pytest.mark.parametrize("family,rule", CASES, ids=[f"{f}-{r}" for f, r in CASES])
def test_seeded_sessions(gpu_engine_module, monkeypatch, family, rule):
    if family == "lds_1024":
        monkeypatch.setenv("MCF_SMALL_THREADS", "1024")
    sm.run_seeds(gpu_engine_module, family, rule, SEEDS[family])


def dropped_at_the_first_solve(session):
    assert session.first_solve["rc_dropped_at"] > 0, f"rule {session.rule}: the first solve reports rc_dropped_at = {session.first_solve['rc_dropped_at']}"


@pytest.mark.gpu
@pytest.mark.parametrize("share,rule", RC_DROP_CASES, ids=[f"{s}-{r}" for s, r in RC_DROP_CASES])
def test_sessions_on_a_handle_that_dropped_its_reduced_costs(gpu_engine_module, share, rule):
    blocks, required = RC_DROP_BLOCKS[share]
    sm.run_seeds(gpu_engine_module, "rc_drop", rule, (1,), required=required, blocks=blocks, check=dropped_at_the_first_solve)


@pytest.mark.gpu
@pytest.mark.parametrize("family,base,blocks", SHORT_SESSIONS, ids=[s[0] for s in SHORT_SESSIONS])
@pytest.mark.parametrize("rule", list(sm.RULES))
def test_short_sessions(gpu_engine_module, rule, family, base, blocks):
    s = sm.Session(gpu_engine_module, family, rule, 0)
    try:
        sm.Planner(family, rule, 0, base=base, blocks=blocks).script(s)
        s.finish()
    finally:
        s.close()
    assert not s.notes, s.notes
