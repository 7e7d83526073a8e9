#!/usr/bin/env python3
"""Cost ranging on the resident handle (mcf_cost_ranges, all arcs) against the only route there was before it: download the
tree and the result (mcf_get_tree + mcf_get_result) and range on the host, on one core.

    python scripts/cost_ranges.py [--nodes 262144 --arcs 2097152] [--repeats 3] [--out profiles/cost_ranges_262k_2m.txt]

One child process under its own `timeout` (nothing more is started on a GPU that has just faulted or hung).  The instance of
the other reoptimize_* scripts, candidate-list rule, solved to optimal.  After one warm-up call (which allocates the tables):
wall time of the call, answer on the host included, and its device part (HIP events), min / median / max over the repeats,
plus the levels K and the greatest depth.  The host route runs the same per-arc logic (csrc/mcf_ranges_host.cpp, binary
lifting, O((n + m) log depth)) -- a parent-pointer climb per arc would be slower still -- and both answers are compared.
"""
import argparse
import ctypes
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def spread(xs, unit=1.0, fmt="{:.3f}"):
    xs = sorted(x * unit for x in xs)
    return " / ".join(fmt.format(x) for x in (xs[0], xs[len(xs) // 2], xs[-1]))


def host_route(lib, eng, inst):
    """Downloads, then the host restatement on one core: (down, up), seconds of the downloads, seconds of the ranging."""
    (tree, res), t_down = timed(lambda: (eng.tree(), eng.result()))
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))                                          # noqa: E731
    down, up, rep = np.zeros(inst.m, np.int64), np.zeros(inst.m, np.int64), np.zeros(8, np.int64)
    tail, head = np.ascontiguousarray(inst.tail, np.int32), np.ascontiguousarray(inst.head, np.int32)
    cost, state = np.ascontiguousarray(inst.cost, np.int64), np.ascontiguousarray(tree["state"], np.int8)
    rc, t_host = timed(lambda: lib.mcf_cost_ranges_host(inst.n, inst.m, p(tail, i32), p(head, i32), p(cost, i64), p(state, i8), p(tree["parent"], i32),
                                                        p(tree["pred_arc"], i32), p(tree["depth"], i32), p(tree["pi"], i64), inst.m, p(down, i64),
                                                        p(up, i64), p(rep, i64)))
    assert rc == 0 and res.status == "optimal"
    return down, up, t_down, t_host


def measure(n, m, repeats):
    import __graft_entry__ as ge
    from network_flow_solver_amd import engine, generators

    lib = ctypes.CDLL(str(ge.build_ranges_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    lib.mcf_cost_ranges_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i8p, i32p, i32p, i32p, i64p, ctypes.c_int64, i64p, i64p, i64p]
    inst = generators.netgen_style(n, m, seed=1)
    print(f"instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule; figures are min / median / max of {repeats} runs "
          f"after one warm-up call", flush=True)
    eng, t_create = timed(lambda: engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=engine.RULE_CANDIDATE_LIST))
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    base = eng.result()
    assert base.status == "optimal"
    print(f"cold: create {t_create:.2f} s, solve {base.stats['pivots']} pivots in {t_cold:.2f} s, objective {base.objective}", flush=True)
    (down, up, rep), t_first = timed(eng.cost_ranges)
    print(f"first call (allocates {20 * rep['levels'] * (inst.n + 1) / 1e6:.1f} MB of tables, {16 * inst.m / 1e6:.1f} MB of answer): {t_first * 1e3:.2f} ms", flush=True)
    wall, dev = [], []
    for _ in range(repeats):
        (d2, u2, r2), t = timed(eng.cost_ranges)
        assert np.array_equal(d2, down) and np.array_equal(u2, up)
        wall.append(t)
        dev.append(r2["device_ms"])
    hd, hu, t_down, t_host = host_route(lib, eng, inst)       # warm-up of the host route
    downs, hosts = [], []
    for _ in range(repeats):
        hd, hu, t_down, t_host = host_route(lib, eng, inst)
        downs.append(t_down)
        hosts.append(t_host)
    assert np.array_equal(hd, down) and np.array_equal(hu, up)
    eng.close()
    finite = int((down != engine.RANGE_INF).sum() + (up != engine.RANGE_INF).sum())
    print(f"levels K {rep['levels']}, greatest depth {rep['max_depth']}; basic arcs {rep['basic_real']} real + {rep['basic_artificial']} artificial; "
          f"eligible {rep['eligible']}; finite ends {finite} of {2 * inst.m}", flush=True)
    print(f"    mcf_cost_ranges  call {spread(wall, 1e3, '{:.2f}')} ms (device part {spread(dev, 1, '{:.2f}')} ms), all {inst.m} arcs", flush=True)
    print(f"    host route       mcf_get_tree + mcf_get_result {spread(downs, 1e3, '{:.2f}')} ms + ranging on one core {spread(hosts, 1e3, '{:.2f}')} ms; "
          f"total {spread([a + b for a, b in zip(downs, hosts)], 1e3, '{:.2f}')} ms; same answer", flush=True)


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
    p = subprocess.Popen(["timeout", "-k", "10", "600", *me, "--step", "measure"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for ln in p.stdout:   # (streamed: a long step shows its progress)
        sys.stdout.write(ln)
        sys.stdout.flush()
        lines.append(ln)
    rc = p.wait()
    if a.out and rc == 0:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
