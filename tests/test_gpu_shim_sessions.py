"""Seeded sessions one layer up: edit scripts on a ``NetworkSimplex`` and on the node / arc dicts it was built from (``-m gpu``).

Everything the shim adds to an edit is on the path: decimal scales, lower-bound shifts, undirected edges, keyed access to
parallel arcs (a key names the LAST arc with it).  Instances are ``random_instances.make(seed)`` (n <= 9; fractional data,
lower bounds and undirected problems among the seeds).  After every edit ``solver.solve()`` is held against
``test_random_cpu.networkx_truth`` of the problem rebuilt from the dicts -- status, the exceptions and the bound of
``test_random_problems_through_the_shim`` (``abs=1e-7``), its balance and bounds check of the reported flows -- and
``solver.certify().verdict`` agrees.  Values are drawn at the instance's own resolution (``flat.cost_scale`` /
``flat.flow_scale``); one edit off that resolution and one capacity below its lower bound must raise ``InvalidProblemError``
and leave the solver as it was.  On an optimal solver ``cost_ranges()``, ``capacity_ranges()`` and ``supply_ranges()`` are each
confirmed by one derived edit: zero pivots, the objective moved by the stated rate.

What an undirected problem is not asked: capacity edits and closing (``close_arcs`` refuses an undirected edge -- that refusal
is asserted), and the cost / capacity derived edits, whose rates are stated for the shifted arc [0, 2C]; its supplies, costs and
new edges are edited like any other's.  New uncapacitated arcs point from a lower to a higher node index, as in
``random_instances``: no uncapacitated cycle, so networkx always answers."""

from __future__ import annotations

import random

import pytest

import network_flow_solver_amd as nfs
from network_flow_solver_amd.exceptions import InvalidProblemError
from random_instances import make

pytestmark = pytest.mark.gpu
STEPS = 10
SEED_GROUPS = [list(range(g, 120, 8)) for g in range(8)]     # 15 tiny sessions per test


def _last(arcs, key):
    """Index of the last arc with this key: the one a keyed update names."""
    return max(i for i, a in enumerate(arcs) if (a["tail"], a["head"]) == key)


def _check(solver, nodes, arcs, directed, note):
    """solve() against networkx on the problem rebuilt from the dicts; returns the result (None when unbounded)."""
    from test_random_cpu import networkx_truth

    problem = nfs.build_problem(nodes, arcs, directed, 1e-6)
    truth_status, truth_obj = networkx_truth(problem)
    if truth_status == "unbounded":
        with pytest.raises(nfs.UnboundedProblemError):
            solver.solve()
        return None
    res = solver.solve()
    assert res.status == truth_status, note
    assert solver.certify().verdict == truth_status, note
    if truth_status == "infeasible":
        assert res.flows == {} and res.objective == 0.0, note
        return res
    assert res.objective == pytest.approx(truth_obj, abs=1e-7), note
    bal = {nd["id"]: nd["supply"] for nd in nodes}
    by_key = {}
    for a in arcs:
        by_key.setdefault((a["tail"], a["head"]), []).append(a)
    for (t, h), f in res.flows.items():
        lo = sum((-x["capacity"] if not directed else x["lower"]) for x in by_key[(t, h)])
        hi = sum((float("inf") if x["capacity"] is None else x["capacity"]) for x in by_key[(t, h)])
        assert lo - 1e-9 <= f <= hi + 1e-9, note
        bal[t] -= f
        bal[h] += f
    assert all(abs(v) <= 1e-9 for v in bal.values()), note
    return res


def _new_arc(rng, ids, directed, cs, fs):
    a, b = rng.sample(range(len(ids)), 2)
    cost = rng.randint(-4 * cs if directed else 0, 12 * cs) / cs
    r = rng.random()
    cap = None if directed and r < 0.15 and a < b else rng.randint(1, 12 * fs) / fs
    lower = 0.0
    if directed and cap is not None and rng.random() < 0.3:
        lower = min(cap, rng.randint(1, 3 * fs) / fs)
    return {"tail": ids[a], "head": ids[b], "capacity": cap, "cost": cost, "lower": lower}


def _edit(rng, solver, nodes, arcs, directed, cs, fs):
    """One seeded edit, on the solver and on the dicts alike.  Returns what it was, for the failure message."""
    ids = [nd["id"] for nd in nodes]
    kinds = ["costs", "supplies", "add"] + (["capacities", "close"] if directed else [])
    kind = rng.choice(kinds) if arcs else rng.choice(["supplies", "add"])
    if kind == "costs":
        changes = {}
        for a in rng.sample(arcs, min(2, len(arcs))):
            changes[(a["tail"], a["head"])] = rng.randint(-4 * cs if directed else 0, 12 * cs) / cs
        assert solver.update_costs(changes) == len(changes)
        for key, c in changes.items():
            arcs[_last(arcs, key)]["cost"] = c
        return kind, changes
    if kind == "supplies":
        a, b = rng.sample(range(len(ids)), 2)
        q = rng.randint(1, 4 * fs) / fs
        changes = {ids[a]: nodes[a]["supply"] + q, ids[b]: nodes[b]["supply"] - q}
        solver.update_supplies(changes)
        nodes[a]["supply"], nodes[b]["supply"] = changes[ids[a]], changes[ids[b]]
        return kind, changes
    if kind == "add":
        new = [_new_arc(rng, ids, directed, cs, fs) for _ in range(rng.randint(1, 2))]
        if arcs and rng.random() < 0.5:                                # a parallel arc: keyed access moves on to it
            twin = rng.choice(arcs)
            new[0]["tail"], new[0]["head"] = twin["tail"], twin["head"]
            if new[0]["capacity"] is None:
                new[0]["capacity"] = 3.0
        rep = solver.add_arcs([dict(a) for a in new])
        assert rep["first_index"] == len(arcs) and rep["count"] == len(new)
        arcs.extend(new)
        return kind, new
    a = rng.choice(arcs)
    key = (a["tail"], a["head"])
    target = arcs[_last(arcs, key)]
    if kind == "capacities":
        cap = target["lower"] + rng.randint(0, 12 * fs) / fs
        if rng.random() < 0.15 and ids.index(key[0]) < ids.index(key[1]):
            cap = None
        solver.update_capacities({key: cap})
        target["capacity"] = cap
        return kind, {key: cap}
    if target["lower"] > 0:
        with pytest.raises(InvalidProblemError, match="cannot be closed"):
            solver.close_arcs([key])
        return "close refused", key
    solver.close_arcs([key])
    target["capacity"] = 0.0
    return kind, key


def _refusals(solver, nodes, arcs, directed, cs, fs, res, note):
    """One edit off the resolution, one capacity below its lower bound, closing an undirected edge: refused, nothing changed."""
    tried = 0
    if arcs:
        key = (arcs[-1]["tail"], arcs[-1]["head"])
        with pytest.raises(InvalidProblemError):
            solver.update_costs({key: arcs[_last(arcs, key)]["cost"] + 1.0 / (3 * cs)})
        tried += 1
        if not directed:
            with pytest.raises(InvalidProblemError, match="cannot be closed"):
                solver.close_arcs([key])
            tried += 1
    with pytest.raises(InvalidProblemError):
        solver.update_supplies({nodes[0]["id"]: nodes[0]["supply"] + 1.0 / (3 * fs), nodes[1]["id"]: nodes[1]["supply"] - 1.0 / (3 * fs)})
    bounded = [a for i, a in enumerate(arcs) if a["lower"] > 0 and _last(arcs, (a["tail"], a["head"])) == i]
    if bounded:
        a = bounded[0]
        with pytest.raises(InvalidProblemError):
            solver.update_capacities({(a["tail"], a["head"]): a["lower"] - 1.0 / fs})
        tried += 1
    again = _check(solver, nodes, arcs, directed, note + " after the refusals")
    if res is not None and again is not None:
        assert again.status == res.status and again.objective == res.objective and again.flows == res.flows and again.iterations == 0, note
    return tried, bool(bounded)


def _single(arcs, key):
    return sum(1 for a in arcs if (a["tail"], a["head"]) == key) == 1


def _derived(solver, nodes, arcs, directed, cs, fs, res, note):
    """On an optimal solver: one edit derived from each kind of range; zero pivots and the objective moved by the stated rate."""
    done = set()
    ids = [nd["id"] for nd in nodes]
    top = max((abs(a["cost"]) for a in arcs), default=0.0)            # (a cost above every cost would raise big-M: ranges hold below it)
    if directed:
        for key, (lo, hi) in solver.cost_ranges().items():
            a = arcs[_last(arcs, key)]
            if not _single(arcs, key):
                continue
            for new in (a["cost"] + 1.0 / cs, a["cost"] - 1.0 / cs):
                if abs(new) <= top and (lo is None or lo <= new) and (hi is None or new <= hi):
                    solver.update_costs({key: new})
                    want = res.objective + res.flows.get(key, 0.0) * (new - a["cost"])
                    a["cost"] = new
                    res = _check(solver, nodes, arcs, directed, note + f" cost of {key} to {new} inside [{lo}, {hi}]")
                    assert res.iterations == 0 and res.objective == pytest.approx(want, abs=1e-7), (note, key, new, lo, hi)
                    done.add("cost")
                    break
            if "cost" in done:
                break
        for key, (lowest, highest, rate, _, _) in solver.capacity_ranges().items():
            a = arcs[_last(arcs, key)]
            if not _single(arcs, key) or a["capacity"] is None or lowest is None:
                continue
            for new in (a["capacity"] + 1.0 / fs, a["capacity"] - 1.0 / fs):
                if new >= a["lower"] and lowest < new and (highest is None or new < highest):   # strictly inside
                    solver.update_capacities({key: new})
                    want = res.objective + rate * (new - a["capacity"])
                    a["capacity"] = new
                    res = _check(solver, nodes, arcs, directed, note + f" capacity of {key} to {new} inside ({lowest}, {highest})")
                    assert res.iterations == 0 and res.objective == pytest.approx(want, abs=1e-7), (note, key, new, lowest, highest, rate)
                    done.add("capacity")
                    break
            if "capacity" in done:
                break
    pairs = [(x, y) for x in ids for y in ids if x != y]
    d = 1.0 / fs
    for (x, y), r in zip(pairs, solver.supply_ranges(pairs)):
        if not r.creates_artificial_flow and (r.limit is None or d < r.limit):
            i, j = ids.index(x), ids.index(y)
            solver.update_supplies({x: nodes[i]["supply"] + d, y: nodes[j]["supply"] - d})
            nodes[i]["supply"] += d
            nodes[j]["supply"] -= d
            want = res.objective + r.rate * d
            res = _check(solver, nodes, arcs, directed, note + f" supply shift {x} -> {y} by {d} below {r.limit}")
            assert res.iterations == 0 and res.objective == pytest.approx(want, abs=1e-7), (note, x, y, r)
            done.add("supply")
            break
    return done


def _session(seed):
    nodes, arcs, directed = make(seed)
    nodes, arcs = [dict(nd) for nd in nodes], [dict(a) for a in arcs]
    solver = nfs.NetworkSimplex(nfs.build_problem(nodes, arcs, directed, 1e-6))
    cs, fs = int(solver.flat.cost_scale), int(solver.flat.flow_scale)
    rng = random.Random(77000 + seed)
    seen = {"directed" if directed else "undirected"}
    if cs > 1 or fs > 1:
        seen.add("scaled")
    script = []
    res = _check(solver, nodes, arcs, directed, f"seed {seed}, start")
    for step in range(STEPS):
        script.append(_edit(rng, solver, nodes, arcs, directed, cs, fs))
        note = f"seed {seed}, step {step}, edits so far {script}"
        seen.add(script[-1][0])
        res = _check(solver, nodes, arcs, directed, note)
        if any(a["lower"] > 0 for a in arcs):
            seen.add("lower")
        if len({(a["tail"], a["head"]) for a in arcs}) < len(arcs):
            seen.add("parallel")
        if res is not None:
            seen.add(res.status)
        if step == STEPS // 2:
            tried, below_lower = _refusals(solver, nodes, arcs, directed, cs, fs, res, note)
            seen.add("off_resolution")
            if below_lower:
                seen.add("below_lower")
        if res is not None and res.status == "optimal" and step in (3, 8):
            seen |= {f"range_{k}" for k in _derived(solver, nodes, arcs, directed, cs, fs, res, note)}
    return seen


@pytest.mark.parametrize("group", range(len(SEED_GROUPS)))
def test_seeded_edit_scripts_through_the_shim(gpu_engine_module, group):
    seen = set()
    for seed in SEED_GROUPS[group]:
        seen |= _session(seed)
    want = {"directed", "costs", "supplies", "capacities", "add", "close", "lower", "parallel", "optimal", "off_resolution", "below_lower",
            "range_cost", "range_capacity", "range_supply"}
    assert want <= seen, sorted(want - seen)


def test_the_seed_groups_hold_every_kind_of_instance(gpu_engine_module):
    """Undirected problems, fractional data, lower bounds and an infeasible state occur among the sessions."""
    seen = set()
    for group in SEED_GROUPS:
        for seed in group[:4]:
            nodes, arcs, directed = make(seed)
            seen.add("directed" if directed else "undirected")
            if any(a["lower"] > 0 for a in arcs):
                seen.add("lower")
            if any(float(x) != int(x) for x in [nd["supply"] for nd in nodes] + [a["cost"] for a in arcs]):
                seen.add("fractional")
    assert seen == {"directed", "undirected", "lower", "fractional"}
