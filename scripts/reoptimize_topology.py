#!/usr/bin/env python3
"""Adding arcs to the resident handle (mcf_add_arcs) against the only route there was before it: a new handle on the extended
instance, mcf_set_basis from the old result, solve.

    python scripts/reoptimize_topology.py [--nodes 262144 --arcs 2097152] [--repeats 3] [--out profiles/add_arcs_262k_2m.txt]

One child process under its own `timeout` (nothing more is started on a GPU that has just faulted or hung).  Candidate-list
rule, solved to optimal.  The edit: 1 % more arcs with random end points, costs and capacities drawn like the instance's,
applied `--repeats` times after one warm-up round; every round runs on a handle of its own that is created, given the solved
basis of the original instance and confirmed optimal first (outside the timed part), because arcs cannot be taken out again.

Per round: wall time of the mcf_add_arcs call and its device part, pivots and seconds of the re-solve -- and the same for the
warm-start route (create + set_basis + solve).  min / median / max over the repeats.
"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SEED = 20262


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def new_arcs(inst, step):
    rng = np.random.default_rng([SEED, step])
    k = max(1, inst.m // 100)
    t = rng.integers(0, inst.n, k).astype(np.int32)
    h = ((t + 1 + rng.integers(0, inst.n - 1, k)) % inst.n).astype(np.int32)
    return t, h, rng.choice(inst.cost, k).astype(np.int64), rng.choice(inst.cap, k).astype(np.int64)


def spread(xs, unit=1.0, fmt="{:.3f}"):
    xs = sorted(x * unit for x in xs)
    return " / ".join(fmt.format(x) for x in (xs[0], xs[len(xs) // 2], xs[-1]))


def measure(n, m, repeats):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(n, m, seed=1)
    mk = lambda t, h, c, cp: engine.McfEngine(inst.n, t, h, c, cp, inst.supply, rule=engine.RULE_CANDIDATE_LIST)
    print(f"instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule; figures are min / median / max of {repeats} runs "
          f"after one warm-up round", flush=True)
    eng, t_create = timed(lambda: mk(inst.tail, inst.head, inst.cost, inst.cap))
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    base = eng.result()
    eng.close()
    assert base.status == "optimal"
    print(f"cold: create {t_create:.2f} s, solve {base.stats['pivots']} pivots in {t_cold:.2f} s, objective {base.objective}", flush=True)
    in_tree = base.in_tree.astype(np.int8)
    at_upper = (~base.in_tree & (inst.cap > 0) & (base.flow == inst.cap)).astype(np.int8)
    rows = []
    for rep in range(repeats + 1):
        t, h, c, cp = new_arcs(inst, rep)
        k = t.shape[0]
        # the resident route, from the solved state of the original instance
        eng = mk(inst.tail, inst.head, inst.cost, inst.cap)
        assert eng.set_basis(in_tree, at_upper)
        eng.solve(max_pivots=1 << 40)
        p0 = eng.result().stats["pivots"]
        report, t_add = timed(lambda: eng.add_arcs(t, h, c, cp))
        _, t_re = timed(lambda: eng.solve(max_pivots=1 << 40))
        res = eng.result()
        eng.close()
        # the route of the parent commit: new handle on the extended instance, basis of the old result, solve
        ext = [np.concatenate(p) for p in ((inst.tail, t), (inst.head, h), (inst.cost, c), (inst.cap, cp))]
        warm, t_c = timed(lambda: mk(*ext))
        ok, t_b = timed(lambda: warm.set_basis(np.concatenate((in_tree, np.zeros(k, np.int8))), np.concatenate((at_upper, np.zeros(k, np.int8)))))
        _, t_s = timed(lambda: warm.solve(max_pivots=1 << 40))
        wres = warm.result()
        warm.close()
        assert (res.status, res.objective) == (wres.status, wres.objective), (res.status, wres.status)
        if rep:   # (round 0 is the warm-up)
            rows.append(dict(add=t_add, dev=report["device_ms"], elig=report["eligible"], shifted=report["shifted_only"], piv=res.stats["pivots"] - p0,
                             re=t_re, accepted=ok, wc=t_c, wb=t_b, wpiv=wres.stats["pivots"], ws=t_s))
    col = lambda key: [r[key] for r in rows]
    print(f"arcs added: {k} (1 % of m); status after: {res.status}, objective {res.objective}", flush=True)
    print(f"    mcf_add_arcs     call {spread(col('add'), 1e3, '{:.2f}')} ms (device part {spread(col('dev'), 1, '{:.2f}')} ms), eligible new arcs "
          f"{spread(col('elig'), 1, '{:.0f}')}, old arcs in shifted chunks {spread(col('shifted'), 1, '{:.0f}')}; re-solve {spread(col('piv'), 1, '{:.0f}')} "
          f"pivots in {spread(col('re'))} s; total {spread([r['add'] + r['re'] for r in rows])} s", flush=True)
    print(f"    warm-start route basis accepted {sorted(set(col('accepted')))}; create {spread(col('wc'))} s + set_basis {spread(col('wb'))} s + solve "
          f"{spread(col('wpiv'), 1, '{:.0f}')} pivots in {spread(col('ws'))} s; total {spread([r['wc'] + r['wb'] + r['ws'] for r in rows])} s", flush=True)


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
