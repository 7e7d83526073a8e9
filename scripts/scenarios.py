#!/usr/bin/env python3
"""What-if scenarios from one solved handle (mcf_fork + edits + mcf_solve_batch) against the only route there was before
it -- one new handle per scenario on the edited instance, mcf_set_basis from the base result, then the batch solve -- and
the device copy of a large fork against the copy ceiling of the box.

    python scripts/scenarios.py [--out profiles/fork_scenarios.txt] [--baseline-lib PATH] [--parts batch,baseline,batch_memcpy,large,large_memcpy,large_plain,large_nt]

Every part runs in a child process of its own under its own `timeout`; the parts are chained, and nothing more is started on a
GPU after a part failed.  Figures are min / median / max of `--repeats` runs after one warm-up round.

  batch         256 nodes / 2 048 arcs (netgen_8_08a-sized), Dantzig rule on the fused LDS loop, solved to optimal; 1 024
                scenarios, each moving 1 % of the costs by up to +-10 %.  Reported separately: the fork (device_ms of the one
                copy launch and wall time), the per-fork edits (mcf_update_costs), the batch solve, the total.
  baseline      the same scenarios by the route of the parent commit: 1 024 x (McfEngine of the edited instance + set_basis
                from the base result), then solve_batch.  With --baseline-lib the child loads that library (a build of the
                parent commit, MCF_HIP_LIB) -- the route only uses calls the parent has.
  large         netgen-style 262 144 nodes / 2 097 152 arcs, candidate-list rule, solved: one fork and one restore;
                bytes_per_fork / device_ms beside engine.time_copy of the same byte count.
  batch_memcpy  the batch with every fork copied by one hipMemcpyAsync per array (MCF_FORK_MEMCPY=1, read at the call).
  large_memcpy  the same large fork as one hipMemcpyAsync per array.
  large_plain   the same fork with plain stores forced (MCF_FORK_NT=0).
  large_nt      ... with non-temporal stores forced (MCF_FORK_NT=1; the default from 128 MiB per fork on).
"""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SEED = 20263
SCENARIOS = 1024


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def spread(xs, unit=1.0, fmt="{:.3f}"):
    xs = sorted(x * unit for x in xs)
    return " / ".join(fmt.format(x) for x in (xs[0], xs[len(xs) // 2], xs[-1]))


def scenario_edits(inst, rep):
    """1 024 x (arcs, new costs): 1 % of the arcs each, every cost moved by up to +-10 %."""
    rng = np.random.default_rng([SEED, rep])
    k = max(1, inst.m // 100)
    out = []
    for _ in range(SCENARIOS):
        arcs = rng.choice(inst.m, k, replace=False)
        cost = np.maximum(1, np.round(inst.cost[arcs] * rng.uniform(0.9, 1.1, k))).astype(np.int64)
        out.append((arcs, cost))
    return out


def base_solve(engine, inst, **kw):
    eng = engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, **kw)
    eng.solve(max_pivots=1 << 40)
    res = eng.result()
    assert res.status == "optimal"
    return eng, res


def part_batch(repeats, label):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(256, 2048, seed=1)
    eng, base = base_solve(engine, inst, rule=engine.RULE_DANTZIG)
    print(f"[{label}] {inst.name}: {inst.n} nodes, {inst.m} arcs, pricing_mode {base.stats['pricing_mode']}, base solve {base.stats['pivots']} pivots; "
          f"{SCENARIOS} scenarios of {max(1, inst.m // 100)} cost changes each", flush=True)
    rows = []
    for rep in range(repeats + 1):
        edits = scenario_edits(inst, rep)
        report = {}
        forks, t_fork = timed(lambda: eng.fork(SCENARIOS, report=report))
        _, t_edit = timed(lambda: [f.update_costs(a, c) for f, (a, c) in zip(forks, edits)])
        ms, t_solve = timed(lambda: engine.solve_batch(forks))
        results, t_read = timed(lambda: [f.result() for f in forks])
        _, t_close = timed(lambda: [f.close() for f in forks])
        assert all(r.status == "optimal" for r in results)
        pivots = sum(r.stats["pivots"] for r in results) - SCENARIOS * base.stats["pivots"]
        if rep:
            rows.append((report["device_ms"], t_fork, t_edit, t_solve, ms, t_read, t_close, t_fork + t_edit + t_solve + t_read, pivots,
                         sum(r.objective for r in results)))
    names = ("fork device_ms", "fork wall ms", "edits wall ms", "batch solve wall ms", "batch solve kernel ms", "read results wall ms",
             "close forks wall ms", "total (fork + edits + solve + read) ms")
    units = (1.0, 1e3, 1e3, 1e3, 1.0, 1e3, 1e3, 1e3)
    for j, (nm, u) in enumerate(zip(names, units)):
        print(f"[{label}] {nm:42s} {spread([r[j] for r in rows], u)}", flush=True)
    print(f"[{label}] bytes per fork {report['bytes_per_fork']}, arrays per fork {report['segments']}; re-solve pivots over all scenarios "
          f"{spread([r[8] for r in rows], 1, '{:.0f}')}; checksum of objectives (round 1) {rows[0][9]}", flush=True)
    eng.close()


def part_baseline(repeats):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(256, 2048, seed=1)
    eng, base = base_solve(engine, inst, rule=engine.RULE_DANTZIG)
    eng.close()
    in_tree = base.in_tree.astype(np.int8)
    at_upper = (~base.in_tree & (inst.cap > 0) & (base.flow == inst.cap)).astype(np.int8)
    print(f"[baseline] library {engine.LIB_PATH}; {SCENARIOS} x (McfEngine of the edited instance + set_basis), then solve_batch", flush=True)
    rows = []
    for rep in range(repeats + 1):
        edits = scenario_edits(inst, rep)

        def build():
            out = []
            for arcs, cost in edits:
                c = inst.cost.copy()
                c[arcs] = cost
                out.append(engine.McfEngine(inst.n, inst.tail, inst.head, c, inst.cap, inst.supply, rule=engine.RULE_DANTZIG))
            return out
        engines, t_create = timed(build)
        ok, t_basis = timed(lambda: [e.set_basis(in_tree, at_upper) for e in engines])
        ms, t_solve = timed(lambda: engine.solve_batch(engines))
        results, t_read = timed(lambda: [e.result() for e in engines])
        _, t_close = timed(lambda: [e.close() for e in engines])
        assert all(ok) and all(r.status == "optimal" for r in results)
        if rep:
            rows.append((t_create, t_basis, t_solve, ms, t_read, t_close, t_create + t_basis + t_solve + t_read,
                         sum(r.stats["pivots"] for r in results), sum(r.objective for r in results)))
    names = ("create wall ms", "set_basis wall ms", "batch solve wall ms", "batch solve kernel ms", "read results wall ms",
             "close wall ms", "total (create + set_basis + solve + read) ms")
    units = (1e3, 1e3, 1e3, 1.0, 1e3, 1e3, 1e3)
    for j, (nm, u) in enumerate(zip(names, units)):
        print(f"[baseline] {nm:42s} {spread([r[j] for r in rows], u)}", flush=True)
    print(f"[baseline] re-solve pivots over all scenarios {spread([r[7] for r in rows], 1, '{:.0f}')}; checksum of objectives (round 1) {rows[0][8]}",
          flush=True)


def part_large(repeats, label):
    from network_flow_solver_amd import engine, generators

    inst = generators.netgen_style(262144, 2097152, seed=1)
    (eng, base), t_base = timed(lambda: base_solve(engine, inst, rule=engine.RULE_CANDIDATE_LIST))
    print(f"[{label}] {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule, solved in {t_base:.1f} s ({base.stats['pivots']} pivots); "
          f"MCF_FORK_MEMCPY={os.environ.get('MCF_FORK_MEMCPY', '')} MCF_FORK_NT={os.environ.get('MCF_FORK_NT', '')}", flush=True)
    rows = []
    fork = None
    for rep in range(repeats + 1):
        report = {}
        forks, t_fork = timed(lambda: eng.fork(1, report=report))
        rest, t_rest = timed(lambda: engine.restore(forks, eng))
        if rep:
            rows.append((report["device_ms"], t_fork, rest["device_ms"], t_rest))
        if rep == repeats:
            fork = forks[0]
        else:
            forks[0].close()
    nbytes = report["bytes_per_fork"]
    ceiling = engine.time_copy(nbytes, reps=10)
    for j, nm in enumerate(("fork device_ms", "fork wall ms", "restore device_ms", "restore wall ms")):
        print(f"[{label}] {nm:42s} {spread([r[j] for r in rows], 1e3 if 'wall' in nm else 1.0)}", flush=True)
    med = sorted(r[0] for r in rows)[len(rows) // 2]
    print(f"[{label}] bytes per fork {nbytes} in {report['segments']} arrays: {nbytes / med / 1e6:.1f} GB/s copied (read + write: twice that) at the median "
          f"device_ms; engine.time_copy of {nbytes} bytes: {ceiling:.3f} ms = {nbytes / ceiling / 1e6:.1f} GB/s; ratio {ceiling / med:.2f}", flush=True)
    # the fork is a handle like any other: it certifies as the source does
    a, b = eng.certify(), fork.certify()
    assert a["verdict"] == b["verdict"] == "optimal" and a["primal"] == b["primal"]
    fork.close()
    eng.close()


def child(part, repeats):
    if part in ("batch", "batch_memcpy"):
        part_batch(repeats, part)
    elif part == "baseline":
        part_baseline(repeats)
    else:
        part_large(repeats, part)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--parts", default="batch,baseline,batch_memcpy,large,large_memcpy,large_plain,large_nt")
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.repeats)
        return 0
    lines = []
    for part in a.parts.split(","):
        env = dict(os.environ)
        if part == "baseline" and a.baseline_lib:
            env["MCF_HIP_LIB"] = str(Path(a.baseline_lib).resolve())
        if part.endswith("_memcpy"):
            env["MCF_FORK_MEMCPY"] = "1"
        if part in ("large_nt", "large_plain"):
            env["MCF_FORK_NT"] = "1" if part == "large_nt" else "0"
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()), "--child", part, "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"[{part}] exit status {r.returncode}: nothing more is started", flush=True)
            lines.append(f"[{part}] exit status {r.returncode}\n")
            break
    if a.out:
        Path(a.out).write_text("".join(lines))
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
