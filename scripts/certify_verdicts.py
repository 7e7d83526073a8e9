#!/usr/bin/env python3
"""mcf_certify_ray / mcf_certify_cut at the verdict family's "scale" size, and on a chain that is the search's worst case.

For every case: the call's device_ms, its wall time, the cut's rounds -- and, measured in the same run, the only
alternative there was before these calls: download the tree (mcf_get_tree) and walk parent pointers on the host (ray), or
download the flows (mcf_get_result) and run a numpy frontier search (cut).  Both sides must agree, or the script fails.

    python scripts/certify_verdicts.py [--size scale] [--chain 4096] [--reps 5] [--out profiles/farkas_verdicts.txt]
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import farkas_yardsticks as fy  # noqa: E402
import verdict_instances as vi  # noqa: E402
from network_flow_solver_amd import engine  # noqa: E402

MCF_INF = 1 << 60
LINES: list[str] = []


def say(text: str) -> None:
    print(text, flush=True)
    LINES.append(text)


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, out)
    return best


def numpy_search(inst, flow):
    """S by whole-array frontier rounds over the downloaded flows: what a caller had to write before mcf_certify_cut."""
    bal = inst.supply.astype(np.int64).copy()
    np.subtract.at(bal, inst.tail, flow)
    np.add.at(bal, inst.head, flow)
    room = vi.is_uncapacitated(inst.cap) | (flow < inst.cap)
    back = flow > 0
    S = bal > 0
    rounds = 0
    while True:
        rounds += 1
        new = np.zeros(inst.n, bool)
        new[inst.head[room & S[inst.tail] & ~S[inst.head]]] = True
        new[inst.tail[back & S[inst.head] & ~S[inst.tail]]] = True
        if not new.any():
            return S, rounds
        S |= new


def time_ray(eng, inst, reps):
    eng.certify_ray()                                               # first call: scratch
    wall, ray = best_of(reps, eng.certify_ray)

    def host():
        tree = eng.tree()
        stats = eng.stats()
        return vi.unbounded_certificate(inst, tree, stats["unbounded_arc"], stats["unbounded_rc"]), tree
    t_host, (length, tree) = best_of(max(1, reps // 2), host)
    cycle = [a for a, _ in vi.cycle_of(inst, tree["parent"], tree["pred_arc"], ray["arc"])]
    assert ray["proven"] and ray["length"] == length and ray["arcs"].tolist() == cycle
    say(f"  ray   {inst.name}: length {ray['length']}, cost {ray['cost']}, proven {ray['proven']}; device {ray['device_ms'] * 1e3:.1f} us, "
        f"call {wall * 1e3:.3f} ms; mcf_get_tree + host walk {t_host * 1e3:.2f} ms ({t_host / wall:.1f}x)")


def time_cut(eng, inst, reps):
    eng.certify_cut()                                               # first call: scratch, supplies, adjacency where none is held
    wall, cut = best_of(reps, eng.certify_cut)

    def host():
        res = eng.result()
        return numpy_search(inst, res.flow)
    t_host, (S, _) = best_of(max(1, reps // 2), host)
    assert cut["proven"] and np.array_equal(cut["S"], S)
    say(f"  cut   {inst.name}: |S| {cut['nodes_in_S']} of {inst.n}, {cut['leaving_arcs']} leaving arcs, excess {cut['excess']}, rounds {cut['rounds']}, "
        f"proven {cut['proven']}; device {cut['device_ms']:.3f} ms, call {wall * 1e3:.3f} ms; mcf_get_result + numpy search {t_host * 1e3:.2f} ms "
        f"({t_host / wall:.1f}x)")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="scale", choices=list(vi.SIZES))
    ap.add_argument("--chain", type=int, default=4096, help="nodes of the chain-shaped worst case of the search")
    ap.add_argument("--rule", type=int, default=engine.RULE_CANDIDATE_LIST)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, m = vi.SIZES[args.size]
    say(f"certify_verdicts: size {args.size} ({n} nodes / {m} arcs), rule {args.rule}, best of {args.reps}")
    cases = [(vi.unbounded(0, n, m, 5), "unbounded"), (vi.infeasible(0, n, m, "cut"), "infeasible"), (vi.infeasible(1, n, m, "starved"), "infeasible")]
    for inst, want in cases:
        with engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=args.rule) as eng:
            t0 = time.perf_counter()
            eng.solve()
            res = eng.result()
            say(f"{inst.name}: {res.status} after {res.stats['pivots']} pivots, {time.perf_counter() - t0:.2f} s, tree_blocks {res.stats['tree_blocks']}")
            if res.status != want:
                return 1
            (time_ray if want == "unbounded" else time_cut)(eng, inst, args.reps)
    chain = fy.chain_cut_instance(args.chain, args.chain - 2, 1000, 400)
    with engine.McfEngine(chain.n, chain.tail, chain.head, chain.cost, chain.cap, chain.supply, rule=engine.RULE_DANTZIG) as eng:
        t0 = time.perf_counter()
        eng.solve()
        res = eng.result()
        say(f"{chain.name}: {res.status} after {res.stats['pivots']} pivots, {time.perf_counter() - t0:.2f} s (one search round per node: the worst case)")
        if res.status != "infeasible":
            return 1
        time_cut(eng, chain, args.reps)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
