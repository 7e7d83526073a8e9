"""``mcf_update_rhs`` without a device: the shim's mapping function, the host repair (``mcf_repair_basis`` behind
``libmcf_repair_host.so``) and the prefix-sum identity the device pass is built on."""

import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import network_flow_solver_amd as nfs
from conftest import load_synthetic
from network_flow_solver_amd.data import SoAProblem
from network_flow_solver_amd.simplex import flatten_problem, flatten_soa, map_rhs_changes

INF = 1 << 60


# ------------------------------------------------------------------ the mapping function
def _object_flat():
    nodes = [dict(id="a", supply=10.5), dict(id="b", supply=0.0), dict(id="c", supply=-4.0), dict(id="d", supply=-6.5)]
    arcs = [dict(tail="a", head="b", capacity=8.0, cost=1.25, lower=1.5), dict(tail="a", head="c", capacity=6.0, cost=4.0, lower=0.0),
            dict(tail="b", head="d", capacity=9.0, cost=2.5, lower=0.5), dict(tail="c", head="d", capacity=None, cost=1.0, lower=0.0),
            dict(tail="c", head="d", capacity=2.0, cost=0.5, lower=0.0)]
    return flatten_problem(nfs.build_problem(nodes, arcs, True, 1e-6))


def test_mapping_scale_shift_and_last_parallel_arc():
    flat = _object_flat()
    assert flat.flow_scale == 10
    before = (flat.supply.copy(), flat.cap.copy())
    s_idx, s_int, s_val, c_idx, c_int, c_val = map_rhs_changes(flat, {"a": 12.5, "d": -8.5}, {("a", "b"): 6.5, ("c", "d"): None, ("b", "d"): 0.5}, 1e-6)
    ids = list(flat.node_ids)
    # supplies keep the node's lower-bound shift: a sends 1.5 out on a -> b, d receives 0.5 on b -> d
    assert dict(zip(s_idx.tolist(), s_int.tolist())) == {ids.index("a"): 110, ids.index("d"): -80}
    assert s_val.tolist() == [12.5, -8.5]
    keys = list(flat.keys)
    last_cd = max(i for i, k in enumerate(keys) if k == ("c", "d"))
    assert dict(zip(c_idx.tolist(), c_int.tolist())) == {keys.index(("a", "b")): 50, last_cd: -1, keys.index(("b", "d")): 0}
    assert np.isnan(c_val[c_idx.tolist().index(last_cd)])
    assert np.array_equal(flat.supply, before[0]) and np.array_equal(flat.cap, before[1])      # pure
    assert all(x.size == 0 for x in map_rhs_changes(flat, None, None, 1e-6))


def test_mapping_refusals_use_the_reference_wording():
    flat = _object_flat()
    with pytest.raises(nfs.InvalidProblemError, match=r"Supplies do not balance after lower-bound adjustment: total supply 0\.500000 exceeds tolerance"):
        map_rhs_changes(flat, {"a": 11.0}, None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match=r"Arc capacity \(1\) is less than lower bound \(1\.5\) for arc a -> b\. Capacity must be >= lower bound\."):
        map_rhs_changes(flat, None, {("a", "b"): 1.0}, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="not a multiple of 1/10"):
        map_rhs_changes(flat, {"a": 10.25, "c": -3.75}, None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="not a multiple of 1/10"):
        map_rhs_changes(flat, None, {("a", "c"): 6.25}, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="not in the problem"):
        map_rhs_changes(flat, {"zz": 0.0}, None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="not in the problem"):
        map_rhs_changes(flat, None, {("a", "z"): 1.0}, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="mapping"):
        map_rhs_changes(flat, ([0], [1.0]), None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="finite"):
        map_rhs_changes(flat, {"a": float("nan")}, None, 1e-6)


def test_mapping_of_an_soa_problem():
    tail, head = np.array([0, 0, 1, 2], np.int32), np.array([1, 2, 3, 3], np.int32)
    lower, cap = np.array([2, 0, 0, 1], np.int64), np.array([9, 5, -1, 7], np.int64)
    problem = SoAProblem(4, tail, head, np.array([1, 2, 3, 4], np.int64), cap, np.array([6, 0, 0, -6], np.int64), lower)
    flat = flatten_soa(problem)
    s_idx, s_int, _, c_idx, c_int, _ = map_rhs_changes(flat, ([0, 3, 0], [9, -8, 8]), ([0, 2, 3, 3], [4, 11, 0, -1]), 1e-6)
    assert dict(zip(s_idx.tolist(), s_int.tolist())) == {0: 8 - 2, 3: -8 + 1}      # last entry wins; shifts -2 at node 0, +1 at node 3
    assert dict(zip(c_idx.tolist(), c_int.tolist())) == {0: 2, 2: 11, 3: -1}
    with pytest.raises(nfs.InvalidProblemError, match="less than lower bound"):
        map_rhs_changes(flat, None, ([0], [1]), 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="do not balance"):
        map_rhs_changes(flat, ([0], [7]), None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="outside"):
        map_rhs_changes(flat, ([4], [0]), None, 1e-6)
    with pytest.raises(nfs.InvalidProblemError, match="pair"):
        map_rhs_changes(flat, {0: 1}, None, 1e-6)


# ------------------------------------------------------------------ the host repair
@pytest.fixture(scope="module")
def repair_lib():
    lib = ctypes.CDLL(str(ge.build_repair_host()))
    i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
    lib.mcf_repair_host.argtypes = [ctypes.c_int32, ctypes.c_int64, i32p, i32p, i64p, i64p, i64p, i8p, i8p, i8p,
                                    i32p, i32p, i8p, i32p, i8p, i64p, i64p, i64p, ctypes.c_char_p, ctypes.c_int32]
    lib.mcf_repair_host.restype = ctypes.c_int
    return lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _repair(lib, inst, supply, cap, in_tree, at_upper, hang=None):
    n, m = inst.n, inst.m
    tail, head = np.ascontiguousarray(inst.tail, np.int32), np.ascontiguousarray(inst.head, np.int32)
    cost, cap, supply = (np.ascontiguousarray(x, np.int64) for x in (inst.cost, cap, supply))
    it, au = np.ascontiguousarray(in_tree, np.int8), np.ascontiguousarray(at_upper, np.int8)
    out = dict(parent=np.zeros(n + 1, np.int32), pred_arc=np.zeros(n + 1, np.int32), up=np.zeros(n + 1, np.int8), order=np.zeros(n + 1, np.int32),
               state=np.zeros(m, np.int8), flow=np.zeros(m, np.int64), art_flow=np.zeros(n, np.int64), report=np.zeros(4, np.int64))
    err = ctypes.create_string_buffer(256)
    hg = None if hang is None else _p(np.ascontiguousarray(hang, np.int8), ctypes.c_int8)
    rc = lib.mcf_repair_host(n, m, _p(tail, ctypes.c_int32), _p(head, ctypes.c_int32), _p(cost, ctypes.c_int64), _p(cap, ctypes.c_int64),
                             _p(supply, ctypes.c_int64), _p(it, ctypes.c_int8), _p(au, ctypes.c_int8), hg,
                             _p(out["parent"], ctypes.c_int32), _p(out["pred_arc"], ctypes.c_int32), _p(out["up"], ctypes.c_int8),
                             _p(out["order"], ctypes.c_int32), _p(out["state"], ctypes.c_int8), _p(out["flow"], ctypes.c_int64),
                             _p(out["art_flow"], ctypes.c_int64), _p(out["report"], ctypes.c_int64), err, 256)
    return rc, err.value.decode(), out


def _random_forest(inst, rng, keep=0.9):
    """A random spanning forest (union-find over a random arc order, a share of the tree arcs dropped again) and random
    non-basic arcs at capacity."""
    uf = list(range(inst.n))

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x
    in_tree = np.zeros(inst.m, np.int8)
    for e in rng.permutation(inst.m).tolist():
        a, b = find(int(inst.tail[e])), find(int(inst.head[e]))
        if a != b and rng.random() < keep:
            uf[a] = b
            in_tree[e] = 1
    at_upper = ((rng.random(inst.m) < 0.2) & (in_tree == 0)).astype(np.int8)
    return in_tree, at_upper


def _check_repaired(inst, supply, cap, in_tree, out):
    n, m = inst.n, inst.m
    capx = np.where((cap < 0) | (cap >= INF), INF, cap)
    parent, pred, up, order, state, flow, art = (out[k] for k in ("parent", "pred_arc", "up", "order", "state", "flow", "art_flow"))
    # a spanning tree rooted at the root, in preorder
    assert parent[n] == -1 and order[0] == n and sorted(order.tolist()) == list(range(n + 1))
    seen = np.zeros(n + 1, bool)
    seen[n] = True
    for v in order[1:].tolist():
        assert seen[parent[v]] and not seen[v]
        seen[v] = True
        a = int(pred[v])
        if a >= m:
            assert a == m + v and parent[v] == n
        else:
            assert state[a] == 0 and {int(inst.tail[a]), int(inst.head[a])} == {v, int(parent[v])} and bool(up[v]) == (int(inst.tail[a]) == v)
    real_tree = pred[:n][pred[:n] < m]
    assert np.array_equal(np.sort(real_tree), np.nonzero(state == 0)[0])
    # bounds, states, conservation with the artificial arcs (Python ints: balances may leave 64 bits)
    assert (flow >= 0).all() and (flow <= capx).all() and (art >= 0).all() and (art < INF).all()
    assert (flow[state == 1] == 0).all() and (flow[state == -1] == capx[state == -1]).all() and (capx[state == -1] < INF).all()
    bal = [int(s) for s in supply.tolist()]
    for e, f in enumerate(flow.tolist()):
        bal[int(inst.tail[e])] -= f
        bal[int(inst.head[e])] += f
    for v in range(n):
        on_art = pred[v] == m + v
        assert bal[v] == ((int(art[v]) if up[v] else -int(art[v])) if on_art else 0), v
        assert on_art or art[v] == 0
    # no wrong-way degenerate basic arc
    for v in range(n):
        a = int(pred[v])
        if a < m:
            assert not (up[v] and capx[a] < INF and flow[a] == capx[a]) and not (not up[v] and flow[a] == 0), (v, a)
        else:
            assert up[v] or art[v] > 0
    # arcs_cut = the real arcs that left the basis
    violations, wrong, cut, rounds = out["report"].tolist()
    assert cut == int(in_tree.sum()) - int((state == 0).sum()) == violations + wrong and rounds >= 1


def test_repair_on_the_golden_instances(repair_lib):
    for spec, inst in load_synthetic()[:4]:
        rng = np.random.default_rng([3, inst.m])
        for trial in range(3):
            in_tree, at_upper = _random_forest(inst, rng, keep=(1.0, 0.9, 0.5)[trial])
            supply, cap = inst.supply.astype(np.int64).copy(), inst.cap.astype(np.int64).copy()
            k = rng.choice(inst.n, max(2, inst.n // 10), replace=False)          # random edits: supplies redrawn in balance ...
            d = rng.integers(-20, 21, k.size)
            d[-1] -= int(d.sum())
            supply[k] += d
            a = rng.choice(inst.m, max(1, inst.m // 10), replace=False)          # ... capacities cut, dropped or set to 0
            cap[a] = rng.choice([0, -1, 1, 5], a.size)
            rc, msg, out = _repair(repair_lib, inst, supply, cap, in_tree, at_upper)
            assert rc == 0, msg
            _check_repaired(inst, supply, cap, in_tree, out)
            if trial == 0:
                # the repaired basis is a fixed point: given back with its hanging nodes, nothing is cut
                hang = (out["pred_arc"][:inst.n] >= inst.m).astype(np.int8)
                rc, msg, again = _repair(repair_lib, inst, supply, cap, (out["state"] == 0), (out["state"] == -1), hang)
                assert rc == 0 and again["report"][2] == 0, (msg, again["report"])
                assert np.array_equal(again["flow"], out["flow"]) and np.array_equal(again["parent"], out["parent"])


def test_repair_with_balances_beyond_64_bits_and_refusals(repair_lib):
    from network_flow_solver_amd.generators import ArcSoA

    # a star: 12 arcs at capacities near 2^60 into one hub, whose balance passes 2^63
    n = 14
    tail = np.array(list(range(1, 13)) + [0], np.int32)
    head = np.array([0] * 12 + [13], np.int32)
    cap = np.array([INF - 1 - i for i in range(12)] + [5], np.int64)
    inst = ArcSoA(n, tail, head, np.ones(13, np.int64), cap, np.zeros(n, np.int64), "star")
    in_tree = np.zeros(13, np.int8)
    in_tree[12] = 1
    at_upper = 1 - in_tree
    rc, msg, out = _repair(repair_lib, inst, inst.supply, cap, in_tree, at_upper)
    assert rc == 1 and "2^60" in msg            # the hub's artificial arc would have to carry ~12 * 2^60
    at_upper[3:12] = 0
    at_upper[0] = 0                             # two arcs are left: 2^61 - 5 arrive at the hub
    rc, msg, out = _repair(repair_lib, inst, inst.supply, cap, in_tree, at_upper)
    assert rc == 1 and "2^60" in msg
    at_upper[2] = 0                             # one arc of 2^60 - 2
    rc, msg, out = _repair(repair_lib, inst, inst.supply, cap, in_tree, at_upper)
    assert rc == 0, msg
    _check_repaired(inst, inst.supply, cap, in_tree, out)
    cyc = ArcSoA(3, np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int32), np.ones(3, np.int64), np.full(3, 4, np.int64), np.zeros(3, np.int64), "cycle")
    rc, msg, _ = _repair(repair_lib, cyc, cyc.supply, cyc.cap, np.ones(3, np.int8), np.zeros(3, np.int8))
    assert rc == 1 and "cycle" in msg


# ------------------------------------------------------------------ the prefix-sum identity
def test_subtree_sums_from_a_scan_over_the_preorder():
    """x[v] = S[pos[v] + size[v]] - S[pos[v]] with S the exclusive prefix sums of the balances in preorder equals the
    children-before-parents accumulation -- the specification k_rhs_scan_* / k_rhs_flows are tested against on the GPU.
    Python ints: the balances are chosen to leave 64 bits."""
    rng = np.random.default_rng(1)
    for N in (2, 3, 257, 2048, 2049, 5000):
        parent = np.full(N, -1, np.int64)
        for v in range(1, N):
            parent[v] = rng.integers(max(0, v - 40), v) if rng.random() < 0.7 else rng.integers(0, v)
        children = [[] for _ in range(N)]
        for v in range(1, N):
            children[parent[v]].append(v)
        order, stack = [], [0]
        while stack:
            u = stack.pop()
            order.append(u)
            stack.extend(reversed(children[u]))
        pos = np.empty(N, np.int64)
        pos[order] = np.arange(N)
        bal = [int(x) << 40 for x in rng.integers(-(1 << 62), 1 << 62, N).tolist()]
        size, acc = [1] * N, list(bal)
        for v in reversed(order[1:]):
            size[parent[v]] += size[v]
            acc[parent[v]] += acc[v]
        S = [0]
        for u in order:
            S.append(S[-1] + bal[u])
        assert all(S[pos[v] + size[v]] - S[pos[v]] == acc[v] for v in range(N))
