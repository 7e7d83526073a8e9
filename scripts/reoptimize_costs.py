#!/usr/bin/env python3
"""Re-optimising after cost changes on the resident handle (mcf_update_costs) against the only route there was before it:
a new handle with the new costs, mcf_set_basis from the old result, solve.

    python scripts/reoptimize_costs.py [--instance netgen_1m_16m] [--out profiles/update_costs_netgen_1m_16m.txt]

The driver starts two child processes one after the other, each under its own `timeout`, and stops at the first that
fails (nothing more is started on a GPU that has just faulted or hung):

  measure   candidate-list rule.  Cold solve; then, for 0.1 % and for 1 % of the arcs (fixed seed, each cost moved by up to
            +-10 %, applied on top of each other): wall time of update_costs, pivots and seconds of the re-solve, and the same
            for the warm-start route on a second handle.  Leaves the last basis and costs in a scratch file.
  trace     under `rocprofv3 --kernel-trace --stats`: a fresh handle takes that basis (host work, no kernel) and one 1 % update;
            prints the durations of the k_uc_* kernels and the rebuild kernel's share of 8 TB/s on its compulsory bytes.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SEED = 20260
PEAK_BYTES_PER_S = 8e12


def perturb(cost, share, step):
    rng = np.random.default_rng([SEED, step])
    m = cost.shape[0]
    idx = rng.choice(m, max(1, int(m * share)), replace=False).astype(np.int64)
    width = np.maximum(1, np.abs(cost[idx]) // 10)
    return idx, cost[idx] + rng.integers(-width, width + 1)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def measure(name, scratch):
    from network_flow_solver_amd import engine, generators

    inst = generators.named_instance(name)
    mk = lambda cost: engine.McfEngine(inst.n, inst.tail, inst.head, cost, inst.cap, inst.supply, rule=engine.RULE_CANDIDATE_LIST)
    print(f"instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule", flush=True)
    eng, t_create = timed(lambda: mk(inst.cost))
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    res = eng.result()
    assert res.status == "optimal"
    print(f"cold: create {t_create:.2f} s, solve {res.stats['pivots']} pivots in {t_cold:.2f} s, objective {res.objective}", flush=True)
    cost = inst.cost.copy()
    for step, share in enumerate((0.001, 0.01)):
        idx, new = perturb(cost, share, step)
        at_upper = ~res.in_tree & (inst.cap > 0) & (res.flow == inst.cap)
        in_tree = res.in_tree.astype(np.int8)
        before = res.stats["pivots"]
        _, t_upd = timed(lambda: eng.update_costs(idx, new))
        _, t_re = timed(lambda: eng.solve(max_pivots=1 << 40))
        res = eng.result()
        cost[idx] = new
        assert res.status == "optimal"
        # a second call on the same state (identical costs): the inverse arc map and the temporaries exist by now
        _, t_upd2 = timed(lambda: eng.update_costs(idx, new))
        eng.solve()
        assert eng.result().stats["pivots"] == res.stats["pivots"]
        print(f"{share * 100:g} % of the arcs ({idx.size}): update_costs {t_upd * 1e3:.2f} ms (first call of the handle builds the inverse "
              f"arc map; same call again: {t_upd2 * 1e3:.2f} ms), re-solve {res.stats['pivots'] - before} pivots in {t_re:.3f} s, "
              f"objective {res.objective}", flush=True)
        # the route of the parent commit: new handle, basis of the old result, solve
        warm, t_c = timed(lambda: mk(cost))
        ok, t_b = timed(lambda: warm.set_basis(in_tree, at_upper.astype(np.int8)))
        _, t_s = timed(lambda: warm.solve(max_pivots=1 << 40))
        wres = warm.result()
        warm.close()
        assert ok and wres.status == "optimal" and wres.objective == res.objective
        print(f"    warm-start route: create {t_c:.2f} s + set_basis {t_b:.2f} s + solve {wres.stats['pivots']} pivots in {t_s:.3f} s "
              f"= {t_c + t_b + t_s:.2f} s   (update route: {t_upd + t_re:.3f} s)", flush=True)
    at_upper = ~res.in_tree & (inst.cap > 0) & (res.flow == inst.cap)
    np.savez(scratch, cost=cost, in_tree=res.in_tree.astype(np.int8), at_upper=at_upper.astype(np.int8))
    eng.close()


def trace_child(name, scratch):
    from network_flow_solver_amd import engine, generators

    inst = generators.named_instance(name)
    z = np.load(scratch)
    eng = engine.McfEngine(inst.n, inst.tail, inst.head, z["cost"], inst.cap, inst.supply, rule=engine.RULE_CANDIDATE_LIST)
    assert eng.set_basis(z["in_tree"], z["at_upper"])
    idx, new = perturb(z["cost"], 0.01, 7)
    eng.update_costs(idx, new)
    tree = eng.tree()
    print(f"traced update: {idx.size} arcs, {int((tree['state'][idx] == 0).sum())} of them basic, tree depth {int(tree['depth'].max())}", flush=True)
    eng.close()


def trace_report(out_dir, name):
    from network_flow_solver_amd import generators  # (sizes only)

    n, m = {"netgen_1m_16m": (1 << 20, 16 << 20)}.get(name, (0, 0))
    if not m:
        inst = generators.named_instance(name)
        n, m = inst.n, inst.m
    rows = []
    for f in glob.glob(str(out_dir) + "/**/*kernel_stats.csv", recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_uc_" in r["Name"]]
    assert rows, "no k_uc_* kernel in the trace"
    for r in sorted(rows, key=lambda r: r["Name"]):
        short = r["Name"].split("k_uc_")[1].split("(")[0].split("E")[0]
        print(f"    k_uc_{short:12s} calls {r['Calls']:>3s}  avg {float(r['AverageNs']) / 1e3:9.2f} us  total {float(r['TotalDurationNs']) / 1e3:9.2f} us")
        if "rebuild" in r["Name"]:
            # compulsory bytes: tail, head, cost 4 B each + state 1 B read, reduced cost 8 B written per arc, potentials 8 B per node
            m_pad = (m + 1023) // 1024 * 1024
            nbytes = m_pad * 21 + (n + 1) * 8
            frac = nbytes / (float(r["AverageNs"]) * 1e-9) / PEAK_BYTES_PER_S
            print(f"    k_uc_rebuild: {nbytes / 1e6:.1f} MB compulsory -> {frac:.2f} of 8 TB/s   (k_price, the same gather shape: 0.30)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="netgen_1m_16m")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    ap.add_argument("--scratch", default="")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a.instance, a.scratch)
    if a.step == "trace":
        return trace_child(a.instance, a.scratch)
    tmp = Path(tempfile.mkdtemp(prefix="reopt_"))
    scratch = str(tmp / "basis.npz")
    me = [sys.executable, str(Path(__file__).resolve()), "--instance", a.instance, "--scratch", scratch]
    lines = []

    def run(cmd, env=None, keep=None):
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        for ln in p.stdout:   # (streamed: a long step shows its progress)
            sys.stdout.write(ln)
            sys.stdout.flush()
            if keep is None or keep in ln:   # (keep: drop the profiler's own chatter from the record)
                lines.append(ln)
        return p.wait()

    try:
        rc = run(["timeout", "-k", "10", "900", *me, "--step", "measure"])
        if rc == 0:   # (chained: the trace only runs after a clean measurement)
            prof = tmp / "prof"
            env = dict(os.environ, MCF_USE_GRAPH="0")
            rc = run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(prof),
                      "-o", "run", "--", *me, "--step", "trace"], env=env, keep="traced update")
            if rc == 0:
                import contextlib
                import io

                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    trace_report(prof, a.instance)
                sys.stdout.write(buf.getvalue())
                lines.append(buf.getvalue())
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("".join(lines))
        return rc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main() or 0)
