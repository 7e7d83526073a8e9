"""The arithmetic the fused LDS loop's front kernel runs once it is budgeted in issue slots, without a GPU: the violation without a
compare (``mcf_narrow_violation_signed``), the register sweep on two accumulators compared as signed 64-bit keys, and the pick that
unpacks the winner's record with selects (``mcf_narrow_pick``) -- the very ``MCF_HD`` functions of ``csrc/mcf_core.h``, called by
``csrc/mcf_small_slots_host.cpp`` in the order of the device code, against the forms the kernel had before, against
``mcf_cand_better`` and against plain Python statements of the rule.  Also vets the inputs of ``test_gpu_small_loop_slots.py``."""

from __future__ import annotations

import ctypes
import shutil
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import small_loop_control_instances as ci
import small_loop_slots_instances as si

INT32_MAX = 2 ** 31 - 1
START = 0xFFFFFFFF                       # mcf_narrow_start(): violation 0, ~id all ones
RC_EDGES = (0, 1, -1, 2, -2, INT32_MAX, -INT32_MAX)


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(str(ge.build_small_slots_host()))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.mcf_slots_violation_host.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.mcf_slots_sweep_batch_host.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, vp, vp]
    lib.mcf_slots_pick_host.argtypes = [vp, i32, vp]
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------ the violation
def _violation_cases():
    rng = np.random.default_rng(11)
    s = [x for x in (-1, 0, 1) for _ in RC_EDGES]
    rc = [r for _ in (-1, 0, 1) for r in RC_EDGES]
    s += rng.integers(-1, 2, 6000).tolist()
    rc += rng.integers(-INT32_MAX, INT32_MAX + 1, 6000).tolist()
    return np.array(s, np.int32), np.array(rc, np.int32)


def test_violation_without_a_compare_is_the_two_select_form(host):
    s, rc = _violation_cases()
    n = len(s)
    sel, flat, sg = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    assert host.mcf_slots_violation_host(_ptr(s), _ptr(rc), n, _ptr(sel), _ptr(flat), _ptr(sg)) == 0
    want = np.maximum(-s.astype(np.int64) * rc.astype(np.int64), 0)
    assert np.array_equal(sel.astype(np.int64), want), "the two-select form is the rule"
    assert sel.tobytes() == flat.tobytes(), "bit for bit"
    assert np.array_equal(sg.astype(np.int64), -s.astype(np.int64) * rc.astype(np.int64)), "signed: -s * rc itself"
    assert (want == INT32_MAX).sum() >= 2 and (want == 0).sum() > n // 3 and (want > 0).sum() > n // 4


# ------------------------------------------------------------------ one lane's sweep
def _partitions(n):
    """Every set partition of n slots as a restricted-growth string: slots with the same letter share a violation."""
    out = []

    def rec(prefix, top):
        if len(prefix) == n:
            out.append(tuple(prefix))
            return
        for b in range(top + 2):
            prefix.append(b)
            rec(prefix, max(top, b))
            prefix.pop()

    rec([0], 0)
    return np.array(out, np.int32)


def _info_inv(ns, extra):
    """small_info(tail, head, q) of slot q: any distinct words with bit 31 clear do."""
    q = np.arange(ns + extra, dtype=np.uint32)
    return (q * 3 + 1) | ((q * 5 + 2) << 11) | (q << 22)


def _run(host, chains, ns, n_lds, st, rc, orig, info):
    cases = len(st)
    st, rc, orig, info = (np.ascontiguousarray(a, t) for a, t in ((st, np.int32), (rc, np.int32), (orig, np.int32), (info, np.uint32)))
    best, inf = np.zeros(cases, np.uint64), np.zeros(cases, np.uint32)
    assert host.mcf_slots_sweep_batch_host(chains, ns, n_lds, cases, _ptr(st), _ptr(rc), _ptr(orig), _ptr(info), _ptr(best), _ptr(inf)) == 0
    return best, inf


def _rule(st, rc, orig, info):
    """Larger violation, then lower id, in plain numpy: (best key, info word) per case."""
    viol = -st.astype(np.int64) * rc.astype(np.int64)
    ok = viol > 0
    score = np.where(ok, viol * (1 << 32) + (0xFFFFFFFF - orig.astype(np.int64)), -1)      # ids are distinct: scores of eligible arcs never tie
    w = score.argmax(axis=1)
    rows = np.arange(len(st))
    any_ = ok.any(axis=1)
    key = (viol[rows, w].astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - orig[rows, w].astype(np.int64)).astype(np.uint64)
    inf = info[rows, w].astype(np.uint32) | np.where(st[rows, w] < 0, np.uint32(0x80000000), np.uint32(0))
    return np.where(any_, key, np.uint64(START)), np.where(any_, inf, np.uint32(0)), w, any_


def _all_forms_agree(host, ns, n_lds, st, rc, orig, info, tag):
    want_key, want_inf, w, any_ = _rule(st, rc, orig, info)
    for chains in (si.CHAINS, 1, 4, 0, -1):       # the kernel's two accumulators; one; four; the serial two-select chain; mcf_cand_better
        best, inf = _run(host, chains, ns, n_lds, st, rc, orig, info)
        assert np.array_equal(best, want_key), (tag, chains, int(np.flatnonzero(best != want_key)[0]))
        assert np.array_equal(inf, want_inf), (tag, chains, int(np.flatnonzero(inf != want_inf)[0]))
    return w, any_


@pytest.mark.parametrize("ns", (si.REG_FEW, si.REG))
def test_sweep_names_the_rules_winner_for_every_pattern_of_equal_violations(host, ns):
    parts = _partitions(ns)
    assert len(parts) == {8: 4140, 10: 115975}[ns]
    rng = np.random.default_rng(ns)
    shuffled = rng.permutation(ns)
    seen = dict(all_distinct=0, all_equal=0, mixed=0, winner_first=0, winner_last=0, tie_across_accumulators=0, tie_inside_an_accumulator=0)
    info = np.broadcast_to(_info_inv(ns, 0), parts.shape)
    slot_state = np.where(np.arange(ns) % 3 == 1, -1, 1).astype(np.int32)       # both states among the slots
    for values in ("rising", "falling"):
        if ns == si.REG and values == "falling":
            parts_v = parts[::2]                     # (every second pattern the other way round: bounded time at ten slots)
        else:
            parts_v = parts
        viol = (10 + parts_v) if values == "rising" else (40 - parts_v)
        st = np.broadcast_to(slot_state, parts_v.shape)
        rc = (-st * viol).astype(np.int32)
        for order, ids in (("ascending", np.arange(ns) + 100), ("descending", 200 - np.arange(ns)), ("shuffled", shuffled + 7)):
            orig = np.broadcast_to(ids.astype(np.int32), parts_v.shape)
            w, any_ = _all_forms_agree(host, ns, 0, st, rc, orig, info[: len(parts_v)], (ns, values, order))
            assert any_.all()
            blocks = parts_v.max(axis=1) + 1
            seen["all_distinct"] += int((blocks == ns).sum())
            seen["all_equal"] += int((blocks == 1).sum())
            seen["mixed"] += int(((blocks > 1) & (blocks < ns)).sum())
            seen["winner_first"] += int((w == 0).sum())
            seen["winner_last"] += int((w == ns - 1).sum())
            top = viol == viol.max(axis=1, keepdims=True)
            chain = np.arange(ns) % si.CHAINS
            wc = chain[w]
            seen["tie_across_accumulators"] += int((top & (chain[None, :] != wc[:, None])).any(axis=1).sum())
            seen["tie_inside_an_accumulator"] += int(((top & (chain[None, :] == wc[:, None])).sum(axis=1) > 1).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("ns", (si.REG_FEW, si.REG))
def test_sweep_never_picks_an_empty_slot_and_finds_a_single_arc_anywhere(host, ns):
    n_lds = 3
    t = ns + n_lds
    info = _info_inv(ns, n_lds)
    rows_st, rows_rc, rows_orig, kinds = [], [], [], []
    # slots from r_n on are empty: reduced cost 0, id 0, whatever state the load returned; the arcs before them all tie, or differ
    for r_n in range(ns + 1):
        for empty_state in (-1, 0, 1):
            for equal in (False, True):
                st = np.where(np.arange(t) % 2 == 0, 1, -1)
                viol = np.full(t, 9) if equal else 5 + (np.arange(t) * 7) % 11
                rc, orig = -st * viol, 50 + np.arange(t)
                st[r_n:], rc[r_n:], orig[r_n:] = empty_state, 0, 0
                rows_st.append(st); rows_rc.append(rc); rows_orig.append(orig); kinds.append("empty_from_%d" % r_n)
    # one eligible arc: in the first slot, in the last register slot, in each LDS position; at the narrow limit too
    for pos in (0, ns - 1, ns, ns + 1, ns + 2):
        for s in (-1, 1):
            for v in (1, INT32_MAX):
                st = np.where(np.arange(t) % 2 == 0, 1, -1)
                rc = st * 3                                         # the wrong sign everywhere: ineligible
                rc[pos], st[pos] = -s * v, s
                st[(pos + 1) % t] = 0                               # a basic arc whose reduced cost is not 0 would be a bug elsewhere; here: masked
                rows_st.append(st); rows_rc.append(rc); rows_orig.append(60 + np.arange(t)); kinds.append("single_at_%d" % pos)
    # an LDS arc ties with the register winner: lower id wins, either way round
    for lds_id in (10, 90):
        st = np.ones(t, np.int64)
        rc = np.full(t, -4)
        rows_st.append(st); rows_rc.append(rc); rows_orig.append(np.concatenate((50 + np.arange(ns), [lds_id, 95, 96]))); kinds.append("lds_tie")
    st, rc, orig = (np.array(x, np.int32) for x in (rows_st, rows_rc, rows_orig))
    w, any_ = _all_forms_agree(host, ns, n_lds, st, rc, orig, np.broadcast_to(info, st.shape), ("edges", ns))
    kinds = np.array(kinds)
    assert not any_[kinds == "empty_from_0"].any(), "nothing in use: the start value, info 0"
    for r_n in range(1, ns + 1):
        sel = kinds == "empty_from_%d" % r_n
        assert any_[sel].all() and (w[sel] < r_n).all(), "an empty slot never wins"
    for pos in (0, ns - 1, ns, ns + 1, ns + 2):
        sel = kinds == "single_at_%d" % pos
        assert sel.sum() == 4 and any_[sel].all() and (w[sel] == pos).all()
    assert set(w[kinds == "lds_tie"].tolist()) == {0, ns}, "the LDS arc wins with the lower id and loses with the higher"


# ------------------------------------------------------------------ the pick
def _pick_cases():
    """16 words per case: four waves' (~id, violation, engine index, info).  Ids are distinct, as a sweep's are."""
    rng = np.random.default_rng(5)
    cases, kinds = [], []

    def slot(viol, orig, e, info):
        return [(~orig) & 0xFFFFFFFF, viol, e, info] if viol else [0, 0, 0xFFFFFFFF if e < 0 else e, info]      # (nothing eligible: key 0)

    for winner in range(4):
        for viol_w in (1, 77, INT32_MAX):
            for neg in (0, 1):
                viols = [max(viol_w - 1 - q, 0) for q in range(4)]
                viols[winner] = viol_w
                ids = rng.permutation(4000)[:4]
                cases.append(sum((slot(viols[q], int(ids[q]), 100 + q, (q + 1) | ((q + 9) << 11) | (q << 22) | (neg << 31)) for q in range(4)), []))
                kinds.append(("winner", winner))
    for equal in (2, 4):                    # equal violations in two and in four waves: the ids decide
        for low in range(equal):
            ids = [500 + q for q in range(4)]
            ids[low] = 3
            viols = [9 if q < equal else 2 for q in range(4)]
            cases.append(sum((slot(viols[q], ids[q], 100 + q, (q + 1) | (q << 22)) for q in range(4)), []))
            kinds.append(("equal_violations", low))
    cases.append(sum((slot(0, 0, -1, 0) for _ in range(4)), []))
    kinds.append(("nothing", -1))
    for only in range(4):                   # one wave found something
        cases.append(sum((slot(6 if q == only else 0, 40 + q, 7 + q, 1 << 31) for q in range(4)), []))
        kinds.append(("winner", only))
    return np.array(cases, np.uint32), kinds


def test_pick_unpacks_the_winning_waves_record_with_selects(host):
    cases, kinds = _pick_cases()
    keys = (cases[:, 1::4].astype(np.uint64) << np.uint64(32)) | cases[:, 0::4].astype(np.uint64)
    for row in keys:
        nz = row[row >> np.uint64(32) != 0]
        assert len(set(nz.tolist())) == len(nz), "distinct ids: two waves never publish the same non-zero key"
    seen = set()
    for c, row, (kind, pos) in zip(cases, keys, kinds):
        out = [np.zeros(7, np.int64), np.zeros(7, np.int64)]
        for flat in (0, 1):
            assert host.mcf_slots_pick_host(_ptr(np.ascontiguousarray(c)), flat, _ptr(out[flat])) == 0
        assert out[0].tobytes() == out[1].tobytes(), (kind, pos)
        key, arc, rc, tail, head, state, pad = out[1].tolist()
        if kind == "nothing":
            assert (key, arc, rc, tail, head, state, pad) == (0, -1, 0, 0, 0, 0, 0)
        else:
            b = int(row.argmax())
            assert b == pos, (kind, pos)
            lo, viol, e, info = (int(x) for x in c[4 * b: 4 * b + 4])
            orig = (~lo) & 0xFFFFFFFF
            st = -1 if info >> 31 else 1
            assert (key, arc, rc, tail, head, state, pad) == (viol, (orig << 32) | e, -st * viol, info & 0x7FF, (info >> 11) & 0x7FF, st, 0)
        seen.add((kind, pos))
    assert {("winner", q) for q in range(4)} <= seen and ("nothing", -1) in seen and sum(k == "equal_violations" for k, _ in seen) == 4


# ------------------------------------------------------------------ the same code under the compiler's checks
def test_stand_alone_program_with_address_and_ub_checks(tmp_path):
    """mcf_small_slots_host.cpp compiled together with a program of its own with -fsanitize=address,undefined, on the same kinds of case."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "small_slots_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_small_slots_driver.cpp"), str(ge.CSRC / "mcf_small_slots_host.cpp")], check=True, cwd=str(ge.CSRC))
    path = tmp_path / "cases.bin"
    lines = 0
    with open(path, "wb") as f:
        s, rc = _violation_cases()
        f.write(struct.pack("<4i", 0, len(s), 0, 0) + s.tobytes() + rc.tobytes())
        lines += len(s)
        for ns in (si.REG_FEW, si.REG):
            parts = _partitions(ns)[:: 37 if ns == si.REG else 3]
            info = _info_inv(ns, 2)
            for j, p in enumerate(parts):
                st = np.where((np.arange(ns + 2) + j) % 3 == 1, -1, 1).astype(np.int32)
                viol = np.concatenate((10 + p, [10 + int(p[j % ns]), 3])).astype(np.int32)
                orig = ((np.arange(ns + 2) * 7 + j) % (ns + 2) + 20).astype(np.int32)      # (7 is prime to 10 and 12: distinct ids)
                f.write(struct.pack("<4i", 1, ns, 2, si.CHAINS) + st.tobytes() + (-st * viol).astype(np.int32).tobytes() + orig.tobytes() + info.tobytes())
                lines += 1
        cases, _ = _pick_cases()
        for c in cases:
            f.write(struct.pack("<4i", 2, 0, 0, 0) + c.tobytes())
            lines += 1
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert len(r.stdout.strip().splitlines()) == lines


# ------------------------------------------------------------------ the GPU file's inputs are what they are meant to be
@pytest.mark.parametrize("m", si.ARC_COUNTS)
def test_gpu_inputs_arc_counts(m):
    inst = si.arc_count(m)
    assert inst.m == m and inst.n <= 64 and ci.fits_lds(inst.n, inst.m) and not inst.supply.any()
    slots = -(-m // si.LANES)
    assert (slots <= si.REG_FEW) == (m <= si.REG_FEW * si.LANES), "the 8-slot sweep up to 2 048 arcs, the 10-slot one beyond"
    if m == si.REG * si.LANES + 1:
        assert slots == si.REG + 1, "one arc priced from LDS"
    tr = si.trace(inst, si.COUNT_STEPS)
    assert tr[0][3] == 0, "arc 0 holds the largest violation of the first sweep"
    assert len(tr) == si.COUNT_STEPS or tr[-1][3] < 0


@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("kind", sorted(si.TIES))
def test_gpu_inputs_planted_ties(kind, order):
    inst = si.tie(kind, order)
    assert ci.fits_lds(inst.n, inst.m) and inst.m == si.REG_FEW * si.LANES
    viol, st, rc, entering = si.trace(inst, si.TIE_STEPS)[0]
    assert (st == 1).all() and np.array_equal(rc, inst.cost), "the start basis: every arc at zero flow, reduced cost = cost"
    tied = np.flatnonzero(viol == viol.max())
    assert len(tied) == 2 and viol.max() == 7 and (viol > 0).sum() == 2
    a, b = (si.engine_slot(inst, int(x)) for x in tied)              # tied[0] is the lower id
    assert entering == tied[0], "the lower id wins"
    assert sorted((a["engine"], b["engine"])) == sorted(si.TIES[kind])
    assert (a["engine"] < b["engine"]) == (order == "ascending"), "ids ascend, or descend, along the engine order"
    want = {"slots_of_one_accumulator": lambda: a["lane"] == b["lane"] and a["slot"] != b["slot"] and a["chain"] == b["chain"],
            "accumulators_of_one_lane": lambda: a["lane"] == b["lane"] and a["chain"] != b["chain"],
            "lanes_of_one_wave": lambda: a["lane"] != b["lane"] and a["wave"] == b["wave"],
            "waves_0_and_3": lambda: {a["wave"], b["wave"]} == {0, 3},
            "waves_1_and_2": lambda: {a["wave"], b["wave"]} == {1, 2}}[kind]
    assert want(), (a, b)


def test_gpu_inputs_single_arc_and_none():
    inst = si.last_slot()
    viol, st, rc, entering = si.trace(inst, 1)[0]
    assert (viol > 0).sum() == 1
    where = si.engine_slot(inst, entering)
    assert (where["lane"], where["slot"], where["wave"]) == (si.LANES - 1, si.REG_FEW - 1, 3)
    viol, st, rc, entering = si.trace(si.nothing(), 1)[0]
    assert entering < 0 and not (viol > 0).any()
    assert ci.emul(si.nothing(), 0)["pivots"] == 0 and ci.emul(si.nothing(), 0)["status"] == "optimal"


def test_gpu_inputs_both_states_with_either_sign():
    inst = si.states()
    assert ci.fits_lds(inst.n, inst.m)
    tr = si.trace(inst, si.STATES_STEPS)
    assert len(tr) == si.STATES_STEPS, "still pivoting at the last compared step"
    seen = set()
    entering_states = set()
    for viol, st, rc, e in tr:
        seen |= {(int(s), int(np.sign(r))) for s, r in zip(st, rc) if s != 0 and r != 0}
        entering_states.add(int(st[e]))
    assert seen == {(1, 1), (1, -1), (-1, 1), (-1, -1)} and entering_states == {1, -1}, "arcs of either state enter"


def test_gpu_inputs_the_narrow_limit():
    import small_loop_front_instances as fi

    inst = si.limit()
    cmax = int(np.abs(inst.cost).max())
    assert fi.rc_bound(fi.big_m(inst.n, cmax), cmax) <= INT32_MAX < fi.rc_bound(fi.big_m(inst.n, cmax + 1), cmax + 1), "one more and the range is wide"


@pytest.mark.parametrize("which", sorted(si.COUNTER_RUNS))
def test_gpu_inputs_counter_runs(which):
    inst = si.counter_run(which)
    end, flips, degenerate = si.COUNTER_RUNS[which]
    em = ci.emul(inst, 0)
    assert ci.fits_lds(inst.n, inst.m) and em["status"] == end and (em["bound_flips"] > 0) == flips and (em["degenerate"] > 0) == degenerate
    assert em["pivots"] > max(si.COUNTER_CAPS), "more than one launch at every cap"
    at = ci.emul(inst, 0, em["pivots"])
    assert at["status"] == "iteration_limit" and at["pivots"] == em["pivots"], "at exactly the solve's pivots the emulation has not yet looked"


def test_gpu_inputs_counter_runs_hold_all_three_events():
    ends = {v[0] for v in si.COUNTER_RUNS.values()}
    assert "unbounded" in ends and any(v[1] for v in si.COUNTER_RUNS.values()) and any(v[2] for v in si.COUNTER_RUNS.values())
