#!/usr/bin/env python3
"""Dual pivots on the device after supply / capacity changes (mcf_update_rhs_dual) against the route there was before them:
mcf_update_rhs (host repair, path 1) and the primal pivots of the re-solve.

    python scripts/reoptimize_rhs_dual.py [--nodes 262144 --arcs 2097152] [--repeats 3] [--baseline-lib PATH] [--only ROUTES]
                                          [--out profiles/update_rhs_dual_262k_2m.txt]

The instance and the two edits are those of scripts/reoptimize_rhs.py (same seeds).  Every route runs in a child process of its own
under its own `timeout` (nothing more is started on a GPU that has just faulted or hung):

  baseline       mcf_update_rhs + mcf_solve; with --baseline-lib from that library (a build of the parent commit, MCF_HIP_LIB);
  dual default   mcf_update_rhs_dual + mcf_solve with the default options (budget 163 x violations, walk <= 64);
  dual sweep     the arc sweep alone (enter_walk -1), no budget;
  dual walk      the adjacency walk wherever the subtree has at most 4 096 nodes, no budget;
  dual 4x        a budget of 4 x violations_before + 16 (read by a call with budget 0 on the same state first): the hand-over
                 to the repair;
  split          MCF_DUAL_TIMING=1: HIP events round the launches of each of the first 2 000 dual pivots of the supplies edit,
                 once with the sweep alone and once with the walk alone -- leave / enter / pivot / update per pivot.

Per edit and route: wall time of the call and of the re-solve to optimal, dual pivots (sweeps / walks) and primal pivots, the
device time of the phase per dual pivot, and the largest pivots-per-violation ratio.  min / median / max over the repeats
after one warm-up round.  `--only a,b` runs a subset of the routes.
"""
import argparse
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from reoptimize_rhs import capacity_edit, spread, supply_edit, timed  # noqa: E402


def measure(n, m, repeats, route):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(n, m, seed=1)
    eng = engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=engine.RULE_CANDIDATE_LIST)
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    base = eng.result()
    assert base.status == "optimal"
    print(f"[{route}] library {engine.LIB_PATH.name}; instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule; cold solve "
          f"{base.stats['pivots']} pivots in {t_cold:.2f} s; min / median / max of {repeats} runs after one warm-up round", flush=True)
    in_tree = base.in_tree.astype(np.int8)
    at_upper = (~base.in_tree & (inst.cap > 0) & (base.flow == inst.cap)).astype(np.int8)
    table = {"baseline": ("update_rhs", None), "default": ("dual default", dict()), "sweep": ("dual sweep only", dict(enter_walk=-1, max_pivots=1 << 40)),
             "walk": ("dual walk <= 4096", dict(enter_walk=4096, max_pivots=1 << 40)), "4x": ("dual budget 4 x violations + 16", dict(max_pivots=None))}
    if route == "split":
        return split(eng, inst, in_tree, at_upper)
    variants = [table[route]]
    for kind in ("supplies", "capacities"):
        for label, opt in variants:
            rows = []
            for rep in range(repeats + 1):
                if kind == "supplies":
                    idx, new = supply_edit(inst.supply.astype(np.int64), rep)
                    args = dict(nodes=idx, supplies=new)
                else:
                    idx, new = capacity_edit(inst.cap.astype(np.int64), rep)
                    args = dict(arcs=idx, caps=new)
                assert eng.set_basis(in_tree, at_upper)          # every repeat starts from the solved state of the original
                eng.solve(max_pivots=1 << 40)
                p0 = eng.result().stats["pivots"]
                if opt is None:
                    report, t_upd = timed(lambda: eng.update_rhs(**args))
                    dual = dict(dual_pivots=0, sweeps=0, walks=0, device_ms=0.0, ended=-1, reason=0, violations_before=report["tree_violations"],
                                violations_after=report["tree_violations"], wrong_way_after=report["wrong_way"])
                else:
                    if "max_pivots" in opt and opt["max_pivots"] is None:     # the budget needs the census: a call with budget 0, then the same state again
                        seen = eng.update_rhs_dual(**args, max_pivots=0)[1]["violations_before"]
                        eng.update_rhs(nodes=np.arange(inst.n), supplies=inst.supply, arcs=np.arange(inst.m), caps=inst.cap)
                        assert eng.set_basis(in_tree, at_upper)
                        eng.solve(max_pivots=1 << 40)
                        p0 = eng.result().stats["pivots"]
                        use = dict(max_pivots=4 * seen + 16)
                    else:
                        use = opt
                    (report, dual, _), t_upd = timed(lambda: eng.update_rhs_dual(**args, **use))
                _, t_re = timed(lambda: eng.solve(max_pivots=1 << 40))
                res = eng.result()
                assert res.status == "optimal"
                eng.update_rhs(nodes=np.arange(inst.n), supplies=inst.supply, arcs=np.arange(inst.m), caps=inst.cap)   # back to the original data
                if rep:
                    rows.append(dict(path=report["path"], upd=t_upd, re=t_re, piv=res.stats["pivots"] - p0, obj=res.objective, cut=report["arcs_cut"], **dual))
            col = lambda k: [r[k] for r in rows]   # noqa: E731
            per = [r["device_ms"] * 1e3 / r["dual_pivots"] for r in rows if r["dual_pivots"]]
            ratio = max((r["dual_pivots"] / max(1, r["violations_before"]) for r in rows), default=0.0)
            print(f"{kind} / {label}: {idx.size} changed; path {sorted(set(col('path')))}, ended {sorted(set(col('ended')))}, reason {sorted(set(col('reason')))}; "
                  f"violations before {spread(col('violations_before'), 1, '{:.0f}')}, after {spread(col('violations_after'), 1, '{:.0f}')}, wrong-way after "
                  f"{spread(col('wrong_way_after'), 1, '{:.0f}')}, arcs cut {spread(col('cut'), 1, '{:.0f}')}", flush=True)
            print(f"    call {spread(col('upd'), 1e3, '{:.2f}')} ms; dual pivots {spread(col('dual_pivots'), 1, '{:.0f}')} (sweeps {spread(col('sweeps'), 1, '{:.0f}')}, "
                  f"walks {spread(col('walks'), 1, '{:.0f}')}), phase {spread(col('device_ms'), 1, '{:.2f}')} ms"
                  + (f" = {spread(per, 1, '{:.1f}')} us per dual pivot" if per else "") + f", largest pivots / violation {ratio:.2f}; re-solve "
                  f"{spread(col('piv'), 1, '{:.0f}')} primal pivots in {spread(col('re'))} s; call + re-solve {spread([r['upd'] + r['re'] for r in rows])} s; "
                  f"objective {rows[-1]['obj']}", flush=True)
    eng.close()


def split(eng, inst, in_tree, at_upper):
    """The library prints one line per call on stderr (MCF_DUAL_TIMING=1 is set by the parent)."""
    idx, new = supply_edit(inst.supply.astype(np.int64), 1)
    for label, walk in (("sweep alone", -1), ("walk alone", 1 << 30)):
        assert eng.set_basis(in_tree, at_upper)
        eng.solve(max_pivots=1 << 40)
        print(f"split / {label}: supplies edit, the first 2000 dual pivots", flush=True)
        _, dual, _ = eng.update_rhs_dual(nodes=idx, supplies=new, max_pivots=2000, enter_walk=walk)
        print(f"    ended {dual['ended']}, {dual['dual_pivots']} dual pivots ({dual['sweeps']} sweeps, {dual['walks']} walks), phase {dual['device_ms']:.2f} ms", flush=True)
        eng.update_rhs(nodes=np.arange(inst.n), supplies=inst.supply, arcs=np.arange(inst.m), caps=inst.cap)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 18)
    ap.add_argument("--arcs", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default="", help="libmcf_hip.so built from the parent commit (default: this library's own mcf_update_rhs)")
    ap.add_argument("--only", default="baseline,default,sweep,walk,4x,split", help="routes to run, in this order")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step:
        return measure(a.nodes, a.arcs, a.repeats, a.step)
    me = [sys.executable, str(Path(__file__).resolve()), "--nodes", str(a.nodes), "--arcs", str(a.arcs), "--repeats", str(a.repeats)]
    lines, rc = [], 0
    for route in [r for r in a.only.split(",") if r]:
        env = dict(os.environ)
        if route == "baseline" and a.baseline_lib:
            env["MCF_HIP_LIB"] = str(Path(a.baseline_lib).resolve())
        if route == "split":
            env["MCF_DUAL_TIMING"] = "1"
        p = subprocess.Popen(["timeout", "-k", "10", "900", *me, "--step", route], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        for ln in p.stdout:   # (streamed: a long step shows its progress)
            sys.stdout.write(ln)
            sys.stdout.flush()
            lines.append(ln)
        rc = p.wait()
        if rc:                # a route that failed or ran out of time: nothing more is started
            break
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
