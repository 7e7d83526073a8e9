#!/usr/bin/env python3
"""Re-optimising after supply / capacity changes on the resident handle (mcf_update_rhs) against the only route there was
before it: a new handle with the new data, mcf_set_basis from the old result, solve.

    python scripts/reoptimize_rhs.py [--nodes 262144 --arcs 2097152] [--repeats 3] [--out profiles/update_rhs_262k_2m.txt]

One child process under its own `timeout` (nothing more is started on a GPU that has just faulted or hung).  Candidate-list
rule, solved to optimal.  Two edits, each applied to the solved state of the original instance, `--repeats` times after one
warm-up round on a handle of its own:

  supplies    1 % of the nodes, each supply moved by up to +-10 % of itself (at least +-1), pairwise so the balance stays;
  capacities  1 % of the capped arcs, each capacity cut by up to 10 %.

Per edit: the path mcf_update_rhs took, wall time of the call and its device part, pivots and seconds of the re-solve --
and the same for the warm-start route (create + set_basis + solve).  min / median / max over the repeats.
"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SEED = 20261


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def supply_edit(supply, step):
    rng = np.random.default_rng([SEED, 0, step])
    n = supply.shape[0]
    k = max(2, n // 100) // 2 * 2
    idx = rng.choice(n, k, replace=False).astype(np.int64)
    a, b = idx[: k // 2], idx[k // 2:]
    width = np.maximum(1, np.abs(supply[a]) // 10)
    d = rng.integers(-width, width + 1)
    new = supply.copy()
    new[a] += d
    new[b] -= d
    return idx, new[idx]


def capacity_edit(cap, step):
    rng = np.random.default_rng([SEED, 1, step])
    capped = np.nonzero(cap > 0)[0]
    idx = rng.choice(capped, max(1, capped.size // 100), replace=False).astype(np.int64)
    return idx, cap[idx] - rng.integers(0, cap[idx] // 10 + 1)


def spread(xs, unit=1.0, fmt="{:.3f}"):
    xs = sorted(x * unit for x in xs)
    return " / ".join(fmt.format(x) for x in (xs[0], xs[len(xs) // 2], xs[-1]))


def measure(n, m, repeats):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(n, m, seed=1)
    mk = lambda supply, cap: engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, cap, supply, rule=engine.RULE_CANDIDATE_LIST)
    print(f"instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule; figures are min / median / max of {repeats} runs "
          f"after one warm-up round", flush=True)
    eng, t_create = timed(lambda: mk(inst.supply, inst.cap))
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    base = eng.result()
    assert base.status == "optimal"
    print(f"cold: create {t_create:.2f} s, solve {base.stats['pivots']} pivots in {t_cold:.2f} s, objective {base.objective}", flush=True)
    in_tree = base.in_tree.astype(np.int8)
    at_upper = (~base.in_tree & (inst.cap > 0) & (base.flow == inst.cap)).astype(np.int8)
    for kind in ("supplies", "capacities"):
        rows = []
        for rep in range(repeats + 1):
            if kind == "supplies":
                idx, new = supply_edit(inst.supply.astype(np.int64), rep)
                supply, cap = inst.supply.astype(np.int64).copy(), inst.cap
                supply[idx] = new
                args = dict(nodes=idx, supplies=new)
            else:
                idx, new = capacity_edit(inst.cap.astype(np.int64), rep)
                supply, cap = inst.supply, inst.cap.astype(np.int64).copy()
                cap[idx] = new
                args = dict(arcs=idx, caps=new)
            # the resident route: the solved state of the original instance comes back by the inverse edit's route -- a
            # fresh installation of the base basis -- so that every repeat starts from the same state
            assert eng.set_basis(in_tree, at_upper)
            eng.solve(max_pivots=1 << 40)
            p0 = eng.result().stats["pivots"]
            report, t_upd = timed(lambda: eng.update_rhs(**args))
            _, t_re = timed(lambda: eng.solve(max_pivots=1 << 40))
            res = eng.result()
            # the route of the parent commit: new handle, basis of the old result, solve
            warm, t_c = timed(lambda: mk(supply, cap))
            ok, t_b = timed(lambda: warm.set_basis(in_tree, at_upper))
            _, t_s = timed(lambda: warm.solve(max_pivots=1 << 40))
            wres = warm.result()
            warm.close()
            assert (res.status, res.objective) == (wres.status, wres.objective), (res.status, wres.status)
            eng.update_rhs(nodes=np.arange(inst.n), supplies=inst.supply, arcs=np.arange(inst.m), caps=inst.cap)   # back to the original data
            if rep:   # (round 0 is the warm-up: first-use allocations, adjacency, inverse arc map)
                rows.append(dict(path=report["path"], upd=t_upd, dev=report["device_ms"], cut=report["arcs_cut"], viol=report["tree_violations"],
                                 piv=res.stats["pivots"] - p0, re=t_re, accepted=ok, wc=t_c, wb=t_b, wpiv=wres.stats["pivots"], ws=t_s))
        col = lambda k: [r[k] for r in rows]
        print(f"{kind}: {idx.size} changed; status after: {res.status}", flush=True)
        print(f"    mcf_update_rhs   path {sorted(set(col('path')))}, call {spread(col('upd'), 1e3, '{:.2f}')} ms (device part {spread(col('dev'), 1, '{:.2f}')} ms), "
              f"violations {spread(col('viol'), 1, '{:.0f}')}, arcs cut {spread(col('cut'), 1, '{:.0f}')}; re-solve {spread(col('piv'), 1, '{:.0f}')} pivots in "
              f"{spread(col('re'))} s; total {spread([r['upd'] + r['re'] for r in rows])} s", flush=True)
        print(f"    warm-start route basis accepted {sorted(set(col('accepted')))}; create {spread(col('wc'))} s + set_basis {spread(col('wb'))} s + solve "
              f"{spread(col('wpiv'), 1, '{:.0f}')} pivots in {spread(col('ws'))} s; total {spread([r['wc'] + r['wb'] + r['ws'] for r in rows])} s", flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 18)
    ap.add_argument("--arcs", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a.nodes, a.arcs, a.repeats)
    me = [sys.executable, str(Path(__file__).resolve()), "--nodes", str(a.nodes), "--arcs", str(a.arcs), "--repeats", str(a.repeats)]
    lines = []
    p = subprocess.Popen(["timeout", "-k", "10", "900", *me, "--step", "measure"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for ln in p.stdout:   # (streamed: a long step shows its progress)
        sys.stdout.write(ln)
        sys.stdout.flush()
        lines.append(ln)
    rc = p.wait()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
