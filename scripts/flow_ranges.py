#!/usr/bin/env python3
"""Flow ranging on the resident handle (mcf_capacity_ranges for all arcs, mcf_supply_ranges for 1 M random pairs) against the
only route there was before it: download the tree and the result (mcf_get_tree + mcf_get_result) and range on the host, on
one core.

    python scripts/flow_ranges.py [--nodes 262144 --arcs 2097152] [--pairs 1000000] [--repeats 3] [--out profiles/flow_ranges_262k_2m.txt]

One child process under its own `timeout` (nothing more is started on a GPU that has just faulted or hung).  The instance of
the other reoptimize_* scripts, candidate-list rule, solved to optimal.  After one warm-up call each (which allocates the
tables): wall time of the call, answer on the host included, and its device part (HIP events), min / median / max over the
repeats, plus the levels K and the greatest depth.  The host route runs the same logic (csrc/mcf_flow_ranges_host.cpp, binary
lifting, O((n + queries) log depth)) after gathering every node's tree-arc record with numpy, and both answers are compared.
No speed-up is promised: what was measured is written down.
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


def host_route(lib, eng, inst, xs, ys):
    """Downloads, then the host restatement on one core: (capacity answer, supply answer), seconds of the downloads, of the
    preparation of the node arrays, of the two rangings."""
    (tree, res), t_down = timed(lambda: (eng.tree(), eng.result()))
    assert res.status == "optimal"
    i32, i64, i8 = ctypes.c_int32, ctypes.c_int64, ctypes.c_int8
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))                                          # noqa: E731
    n, m = inst.n, inst.m

    def prepare():
        pred = tree["pred_arc"].astype(np.int64)[:n]
        art = pred >= m
        a = np.where(art, 0, pred)
        up = np.append(np.where(art, tree["pi"][:n] < tree["pi"][n], inst.tail[a] == np.arange(n)), 0).astype(np.int8)
        tflow = np.append(np.where(art, 0, res.flow[a]), 0).astype(np.int64)    # (optimal and feasible: no artificial arc carries flow)
        tcap = np.append(np.where(art, -1, inst.cap[a]), 0).astype(np.int64)
        state = np.ascontiguousarray(tree["state"], np.int8)
        return up, tflow, tcap, state
    (up, tflow, tcap, state), t_prep = timed(prepare)
    tail, head = np.ascontiguousarray(inst.tail, np.int32), np.ascontiguousarray(inst.head, np.int32)
    cost, cap, flow = (np.ascontiguousarray(x, np.int64) for x in (inst.cost, inst.cap, res.flow))
    outs = [np.zeros(m, np.int64) for _ in range(5)]
    rep = np.zeros(10, np.int64)
    rc, t_cap = timed(lambda: lib.mcf_capacity_ranges_host(n, m, p(tail, i32), p(head, i32), p(cost, i64), p(cap, i64), p(flow, i64), p(state, i8),
                                                           p(tree["parent"], i32), p(tree["pred_arc"], i32), p(up, i8), p(tree["depth"], i32),
                                                           p(tflow, i64), p(tcap, i64), p(tree["pi"], i64), 0, *(p(o, i64) for o in outs), p(rep, i64)))
    assert rc == 0
    k = len(xs)
    limit, arc, rate = (np.zeros(k, np.int64) for _ in range(3))
    rising = np.zeros(k, np.int32)
    rc, t_sup = timed(lambda: lib.mcf_supply_ranges_host(n, m, p(tree["parent"], i32), p(tree["pred_arc"], i32), p(up, i8), p(tree["depth"], i32),
                                                         p(tflow, i64), p(tcap, i64), p(tree["pi"], i64), 0, k, p(xs, i32), p(ys, i32),
                                                         p(limit, i64), p(arc, i64), p(rate, i64), p(rising, i32), p(rep, i64)))
    assert rc == 0
    return outs, (limit, arc, rate, rising), t_down, t_prep, t_cap, t_sup


def measure(n, m, pairs, repeats):
    import __graft_entry__ as ge
    from network_flow_solver_amd import engine, generators

    lib = ctypes.CDLL(str(ge.build_flow_ranges_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    lib.mcf_supply_ranges_host.argtypes = [i32, i64, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int, i64, i32p, i32p, i64p, i64p, i64p, i32p, i64p]
    lib.mcf_capacity_ranges_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i8p, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int,
                                             i64p, i64p, i64p, i64p, i64p, i64p]
    inst = generators.netgen_style(n, m, seed=1)
    print(f"instance {inst.name}: {inst.n} nodes, {inst.m} arcs, candidate-list rule; figures are min / median / max of {repeats} runs "
          f"after one warm-up call", flush=True)
    eng, t_create = timed(lambda: engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=engine.RULE_CANDIDATE_LIST))
    _, t_cold = timed(lambda: eng.solve(max_pivots=1 << 40))
    base = eng.result()
    assert base.status == "optimal"
    print(f"cold: create {t_create:.2f} s, solve {base.stats['pivots']} pivots in {t_cold:.2f} s, objective {base.objective}", flush=True)
    rng = np.random.default_rng(1)
    xs, ys = rng.integers(0, n, pairs).astype(np.int32), rng.integers(0, n, pairs).astype(np.int32)
    cap0, t_first = timed(eng.capacity_ranges)
    rep = cap0[5]
    print(f"first capacity call (allocates {28 * rep['levels'] * (inst.n + 1) / 1e6:.1f} MB of tables, {40 * inst.m / 1e6:.1f} MB of answer): "
          f"{t_first * 1e3:.2f} ms", flush=True)
    sup0, t_first = timed(lambda: eng.supply_ranges(xs, ys))
    print(f"first supply call ({36 * pairs / 1e6:.1f} MB of pairs and answer): {t_first * 1e3:.2f} ms", flush=True)
    cw, cd, sw, sd = [], [], [], []
    for _ in range(repeats):
        got, t = timed(eng.capacity_ranges)
        assert all(np.array_equal(a, b) for a, b in zip(got[:5], cap0[:5]))
        cw.append(t)
        cd.append(got[5]["device_ms"])
        got, t = timed(lambda: eng.supply_ranges(xs, ys))
        assert all(np.array_equal(a, b) for a, b in zip(got[:4], sup0[:4]))
        sw.append(t)
        sd.append(got[4]["device_ms"])
    host_route(lib, eng, inst, xs, ys)                           # warm-up of the host route
    downs, preps, caps, sups = [], [], [], []
    for _ in range(repeats):
        hc, hs, t_down, t_prep, t_cap, t_sup = host_route(lib, eng, inst, xs, ys)
        downs.append(t_down)
        preps.append(t_prep)
        caps.append(t_cap)
        sups.append(t_sup)
    assert all(np.array_equal(a, b) for a, b in zip(hc, cap0[:5])) and all(np.array_equal(a, b) for a, b in zip(hs, sup0[:4]))
    eng.close()
    inf = engine.RANGE_INF
    print(f"levels K {rep['levels']}, greatest depth {rep['max_depth']}; basic arcs {rep['basic_real']} real + {rep['basic_artificial']} artificial; "
          f"arcs at capacity {rep['at_capacity']}; capacity sides: {rep['inf_count']} unbounded, {rep['zero_count']} zero of {2 * inst.m}; "
          f"supply pairs: {int((sup0[0] == inf).sum())} unbounded, {int((sup0[0] == 0).sum())} zero of {pairs}", flush=True)
    print(f"    mcf_capacity_ranges  call {spread(cw, 1e3, '{:.2f}')} ms (device part {spread(cd, 1, '{:.2f}')} ms), all {inst.m} arcs", flush=True)
    print(f"    mcf_supply_ranges    call {spread(sw, 1e3, '{:.2f}')} ms (device part {spread(sd, 1, '{:.2f}')} ms), {pairs} pairs", flush=True)
    print(f"    host route           mcf_get_tree + mcf_get_result {spread(downs, 1e3, '{:.2f}')} ms + node arrays (numpy) {spread(preps, 1e3, '{:.2f}')} ms "
          f"+ on one core: capacities {spread(caps, 1e3, '{:.2f}')} ms, supplies {spread(sups, 1e3, '{:.2f}')} ms; "
          f"total {spread([a + b + c + d for a, b, c, d in zip(downs, preps, caps, sups)], 1e3, '{:.2f}')} ms; same answers", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 18)
    ap.add_argument("--arcs", type=int, default=1 << 21)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step == "measure":
        return measure(a.nodes, a.arcs, a.pairs, a.repeats)
    me = [sys.executable, str(Path(__file__).resolve()), "--nodes", str(a.nodes), "--arcs", str(a.arcs), "--pairs", str(a.pairs), "--repeats", str(a.repeats)]
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
