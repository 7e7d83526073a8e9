#!/usr/bin/env python3
"""Record what the REFERENCE's ``validate_flow`` / ``compute_bottleneck_arcs`` (utils.py:169-312) return, as data.

    python tests/golden/make_utils_golden.py --reference DIR     # DIR holds the reference's src/; writes utils_cases.json

Inputs: problems of cases.json (one undirected, one with non-zero lower bounds and parallel arcs among them), one
transshipment problem with the node ids "1" .. "n" of an ``SoAProblem``, and for each the flows the reference's own solve
returned plus one deliberately broken flow dict (an arc over its capacity, one pushed below its lower bound, one arc and
one node the problem does not know).  Outputs: every field of the reference's results.  Nothing but inputs and outputs
is stored.
"""
import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
CASES = ("sample_problem", "textbook_transport", "small_transshipment", "undirected_chain75", "lower_bounds_and_parallel",
         "fractional_costs", "property_seed5", "large_transport")
THRESHOLDS = (0.95, 0.5, 1.0, 0.0)


def broken_flows(flows, arcs):
    """The solved flows with four planted faults (deterministic: positions by order)."""
    out = [[t, h, f] for t, h, f in flows]
    caps = {(a["tail"], a["head"]): a for a in arcs}
    capped = [i for i, (t, h, _) in enumerate(out) if caps.get((t, h), {}).get("capacity") is not None]
    if capped:
        i = capped[0]
        out[i][2] = caps[(out[i][0], out[i][1])]["capacity"] + 1.5
    if len(out) > 1:
        j = len(out) - 1
        a = caps.get((out[j][0], out[j][1]))
        out[j][2] = (a["lower"] if a else 0.0) - 2.0
    out.append(["ghost_u", out[0][0], 3.0])          # an arc and a node the problem does not know
    return out


def record(utils, problem, flows, FlowResult):
    result = FlowResult(objective=0.0, flows={(t, h): f for t, h, f in flows}, status="optimal", iterations=0, duals={})
    v = utils.validate_flow(problem, result)
    entry = {"flows": flows,
             "validate": {"is_valid": v.is_valid, "errors": v.errors, "flow_balance": v.flow_balance,
                          "capacity_violations": [list(k) for k in v.capacity_violations],
                          "lower_bound_violations": [list(k) for k in v.lower_bound_violations]},
             "bottlenecks": {}}
    for th in THRESHOLDS:
        entry["bottlenecks"][repr(th)] = [[b.tail, b.head, b.flow, b.capacity, b.utilization, b.cost, b.slack]
                                          for b in utils.compute_bottleneck_arcs(problem, result, threshold=th)]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference) / "src"))
    from network_solver import build_problem, solve_min_cost_flow, utils
    from network_solver.data import FlowResult

    cases = {c["name"]: c for c in json.loads((HERE / "cases.json").read_text())}
    todo = [(name, cases[name]["nodes"], cases[name]["arcs"], cases[name]["directed"], cases[name]["tolerance"]) for name in CASES]
    # the transshipment problem under the ids an SoAProblem gives its nodes ("1" .. "n", in node order)
    src = cases["small_transshipment"]
    ids = {nd["id"]: str(i + 1) for i, nd in enumerate(src["nodes"])}
    todo.append(("soa_small_transshipment", [{"id": ids[nd["id"]], "supply": nd["supply"]} for nd in src["nodes"]],
                 [dict(a, tail=ids[a["tail"]], head=ids[a["head"]]) for a in src["arcs"]], True, src["tolerance"]))
    out = []
    for name, nodes, arcs, directed, tol in todo:
        problem = build_problem(nodes=nodes, arcs=arcs, directed=directed, tolerance=tol)
        res = solve_min_cost_flow(problem)
        assert res.status == "optimal", (name, res.status)
        flows = [[t, h, float(f)] for (t, h), f in res.flows.items()]
        out.append({"name": name, "directed": directed, "tolerance": tol, "nodes": nodes, "arcs": arcs,
                    "solved": record(utils, problem, flows, FlowResult),
                    "broken": record(utils, problem, broken_flows(flows, arcs), FlowResult)})
        print(name, len(flows), out[-1]["solved"]["validate"]["is_valid"], len(out[-1]["broken"]["validate"]["errors"]), flush=True)
    (HERE / "utils_cases.json").write_text(json.dumps(out, indent=0) + "\n")


if __name__ == "__main__":
    main()
