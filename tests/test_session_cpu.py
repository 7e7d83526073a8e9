"""The session harness (``session_model``) without a device: it runs, and it can fail.

**The stand-in handle** has the driver's surface (``McfEngine``'s methods, ``EngineError``, ``solve_batch``) and keeps no
history: after every edit it takes tree, flows and potentials from ``oracle.emul_solve`` on its current instance (warm
through ``warm_in_tree`` / ``warm_at_upper`` while ``m`` is unchanged, cold otherwise), and it answers the post-solve queries
through the host restatements of the device passes (``libmcf_ranges_host.so``, ``libmcf_flow_ranges_host.so``,
``libmcf_certify_host.so``, ``libmcf_farkas_host.so``).  Every seed list of ``tests/test_gpu_sessions.py`` runs on it end
to end with a complete event union.

Checks the driver leaves out on the stand-in (``session_model.Flags``), because a handle that re-solves after every edit
cannot have the property -- nothing else is skipped:

* ``history=False``: the report of ``update_rhs`` (path, tree_violations, wrong_way, art_flips) against the flow
  yardstick; the eligible arc of violation 1 after a cost edit one unit past a range; the pivot count of the solve after
  an edit inside a range (the objective is still asserted); flows / potentials / states carried unchanged across
  ``add_arcs``.
* ``fresh_equal`` stays on: ``reset(); solve()`` equals a fresh stand-in field by field.

**Planted defects**: for each checker one state with one defect, and exactly that checker fails.

**The generator** is deterministic, and the model's edits equal a rebuild from scratch."""

from __future__ import annotations

import copy
import ctypes
import types

import numpy as np
import pytest

import __graft_entry__ as ge
import oracle
import session_model as sm
import test_certify_cpu as tc
import test_cost_ranges_cpu as tr
import test_farkas_cpu as tf
import test_flow_ranges_cpu as tfr
import farkas_yardsticks as fk
import flow_ranges_yardsticks as fy
from network_flow_solver_amd import generators
from network_flow_solver_amd.generators import ArcSoA

MCF_INF = sm.MCF_INF
STAND_IN_FLAGS = sm.Flags(history=False)


# ------------------------------------------------------------------ the host restatements
def _libs():
    if not _libs.cache:
        i32p, i64p, i8p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int8))
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        rng = ctypes.CDLL(str(ge.build_ranges_host()))
        rng.mcf_cost_ranges_host.argtypes = [i32, i64, i32p, i32p, i64p, i8p, i32p, i32p, i32p, i64p, i64, i64p, i64p, i64p]
        rng.mcf_cost_ranges_host.restype = ctypes.c_int
        frng = ctypes.CDLL(str(ge.build_flow_ranges_host()))
        frng.mcf_supply_ranges_host.argtypes = [i32, i64, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int, i64, i32p, i32p, i64p, i64p, i64p, i32p, i64p]
        frng.mcf_capacity_ranges_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i8p, i32p, i32p, i8p, i32p, i64p, i64p, i64p, ctypes.c_int,
                                                  i64p, i64p, i64p, i64p, i64p, i64p]
        frng.mcf_supply_ranges_host.restype = frng.mcf_capacity_ranges_host.restype = ctypes.c_int
        cert = ctypes.CDLL(str(ge.build_certify_host()))
        cert.mcf_certify_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i64p, i64p, ctypes.c_uint32, i64p]
        cert.mcf_certify_host.restype = ctypes.c_int
        cert.mcf_bottlenecks_host.argtypes = [i64, i64p, i64p, i64, i64, i64p, i64]
        cert.mcf_bottlenecks_host.restype = i64
        far = ctypes.CDLL(str(ge.build_farkas_host()))
        far.mcf_ray_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i32p, i32p, i32p, i32p, i32p, i64p, i64p, i64, i64, i32, i64, i64p, i64, i64p]
        far.mcf_ray_host.restype = ctypes.c_int
        far.mcf_cut_host.argtypes = [i32, i64, i32p, i32p, i64p, i64p, i64p, i64p, i8p, i64, i8p, i64p]
        far.mcf_cut_host.restype = ctypes.c_int
        _libs.cache.update(ranges=rng, flow=frng, certify=cert, farkas=far)
    return _libs.cache


_libs.cache = {}


# ------------------------------------------------------------------ the stand-in
class StandInError(Exception):
    def __init__(self, code, message=""):
        super().__init__(f"stand-in error {code}: {message}")
        self.code = code


class StandIn:
    """The driver's surface on the CPU emulation; no history (see the module docstring)."""

    def __init__(self, n, tail, head, cost, cap, supply, rule=0, **_options):
        self.n = int(n)
        self.tail, self.head = np.array(tail, np.int32), np.array(head, np.int32)
        self.cost, self.cap, self.supply = np.array(cost, np.int64), np.array(cap, np.int64), np.array(supply, np.int64)
        self.rule = rule
        self.big_m = sm.big_m_of(self.n, self.cost)
        self.pivots = self.degenerate = 0
        self.published = "running"
        self._error = ""
        self._run(max_pivots=0)

    # -- plumbing
    @property
    def m(self):
        return len(self.tail)

    def inst(self):
        return ArcSoA(self.n, self.tail, self.head, self.cost, self.cap, self.supply, "stand_in")

    def _run(self, max_pivots=-1, warm=None):
        kw = {} if warm is None else dict(warm_in_tree=warm[0], warm_at_upper=warm[1])
        assert sm.big_m_of(self.n, self.cost) == self.big_m, "the emulation derives big-M from the present costs"
        self.r = oracle.emul_solve(self.n, self.tail, self.head, self.cost, self.cap, self.supply, rule=self.rule, max_pivots=max_pivots, **kw)
        capped = (self.cap >= 0) & (self.cap < MCF_INF)
        in_tree = self.r["in_tree"].astype(bool)
        self.state = np.where(in_tree, 0, np.where((self.r["flow"] == self.cap) & capped & (self.cap > 0), -1, 1)).astype(np.int8)
        return self.r

    def _basis(self):
        return self.r["in_tree"].copy(), (self.state == -1).astype(np.int8)

    def _after_edit(self, warm):
        r = self._run(warm=warm)
        self.pivots += r["pivots"]
        self.degenerate += r["degenerate"]
        self.published = "running"

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def last_error(self):
        return self._error

    # -- solve path
    def solve(self, max_pivots=-1):
        if self.r["status"] == "iteration_limit" and max_pivots != 0:   # a partial state comes from a cold start only: go on from there
            done = self.r["pivots"]
            r = self._run(max_pivots=-1 if max_pivots < 0 else done + max_pivots)
            self.pivots += r["pivots"] - done
            self.degenerate += r["degenerate"]
        self.published = self.r["status"]

    def stats(self):
        return {"pivots": self.pivots, "status": self.published}

    def result(self):
        status = "iteration_limit" if self.published == "running" else self.published
        if status == "optimal" and self.r["artificial_flow"]:
            status = "infeasible"
        flow = self.r["flow"].copy()
        objective = sum(int(c) * int(f) for c, f in zip(self.cost.tolist(), flow.tolist()))
        stats = {"pivots": self.pivots, "degenerate": self.degenerate, "pricing_mode": 0, "artificial_flow": int(self.r["artificial_flow"]),
                 "unbounded_arc": int(self.r["unbounded_arc"]), "rc_dropped_at": 0}
        return types.SimpleNamespace(status=status, objective=objective, flow=flow, potential=self.r["potential"].copy(),
                                     in_tree=self.r["in_tree"].astype(bool), stats=stats)

    def reset(self):
        self._run(max_pivots=0)
        self.pivots = self.degenerate = 0
        self.published = "running"

    def set_basis(self, in_tree, at_upper=None):
        au = np.zeros(self.m, np.int8) if at_upper is None else np.asarray(at_upper, np.int8)
        r = self._run(max_pivots=0, warm=(np.asarray(in_tree, np.int8), au))
        self.pivots = self.degenerate = 0
        self.published = "running"
        return bool(r["warm_applied"])

    # -- edits
    def update_costs(self, arcs, costs):
        a, c = np.asarray(arcs, np.int64).reshape(-1), np.asarray(costs, np.int64).reshape(-1)
        if len(a) and (a.min() < 0 or a.max() >= self.m):
            raise StandInError(sm.E_BAD_ARG, "arc index")
        if len(c) and np.abs(c).max() > sm.INT32_MAX:
            raise StandInError(sm.E_RANGE, "cost")
        warm = self._basis()
        self.cost[a] = c
        self.big_m = max(self.big_m, sm.big_m_of(self.n, self.cost))
        self._after_edit(warm)

    def update_rhs(self, nodes=(), supplies=(), arcs=(), caps=()):
        nd, sv = np.asarray(nodes, np.int64).reshape(-1), np.asarray(supplies, np.int64).reshape(-1)
        ar, cv = np.asarray(arcs, np.int64).reshape(-1), np.asarray(caps, np.int64).reshape(-1)
        if (len(nd) and (nd.min() < 0 or nd.max() >= self.n)) or (len(ar) and (ar.min() < 0 or ar.max() >= self.m)):
            raise StandInError(sm.E_BAD_ARG, "index")
        supply = self.supply.copy()
        supply[nd] = sv
        if int(supply.sum()) != 0:
            raise StandInError(sm.E_RANGE, "supplies do not sum to 0")
        warm = self._basis()
        self.supply = supply
        self.cap[ar] = cv
        self._after_edit(warm)
        return {"path": -1, "tree_violations": -1, "wrong_way": -1, "art_flips": -1, "arcs_cut": 0, "repair_rounds": 0, "upper_moved": 0}

    def add_arcs(self, tail, head, cost, cap, priority=None):
        t, h = np.asarray(tail, np.int64).reshape(-1), np.asarray(head, np.int64).reshape(-1)
        c, cp = np.asarray(cost, np.int64).reshape(-1), np.asarray(cap, np.int64).reshape(-1)
        if len(t) and (t.min() < 0 or t.max() >= self.n or h.min() < 0 or h.max() >= self.n or (t == h).any()):
            raise StandInError(sm.E_BAD_ARG, "end point")
        if len(c) and np.abs(c).max() > sm.INT32_MAX:
            raise StandInError(sm.E_RANGE, "cost")
        m0, old = self.m, self.big_m
        self.tail, self.head = np.concatenate([self.tail, t]).astype(np.int32), np.concatenate([self.head, h]).astype(np.int32)
        self.cost, self.cap = np.concatenate([self.cost, c]), np.concatenate([self.cap, cp])
        self.big_m = max(self.big_m, sm.big_m_of(self.n, self.cost))
        self._after_edit(None)
        pi = self.tree()["pi"]
        return {"first_index": m0, "m": self.m, "bigm_grew": int(self.big_m > old), "shifted_only": 0,
                "eligible": int((c + pi[t] - pi[h] < 0).sum())}

    # -- introspection
    def tree(self):
        d = {k: self.r[k].copy() for k in ("parent", "pred_arc", "size", "pos", "order", "depth", "psize")}
        d["state"] = self.state.copy()
        d["pi"] = np.append(self.r["potential"], 0).astype(np.int64)
        return d

    def reduced_costs(self):
        pi = self.tree()["pi"]
        return self.cost + pi[self.tail] - pi[self.head], True

    def pricing_keys(self):
        return np.zeros(self.m, np.int32), False

    def weights(self):
        return np.ones(self.m, np.float32)

    def price_once(self, rule=None, start=0, end=None):
        rc, _ = self.reduced_costs()
        viol = -self.state.astype(np.int64) * rc
        best = int(viol.max(initial=0))
        if best <= 0:
            return None
        arc = int(np.flatnonzero(viol == best)[0])
        return arc, (1 if self.state[arc] > 0 else -1), best

    # -- queries: the host restatements
    def _art(self):
        return fk.artificial_flows(self.inst(), self.r["flow"])

    def certify(self):
        inst = self.inst()
        d = tc.certify_host(_libs()["certify"], inst, self.r["flow"], self.r["potential"])
        art = sum(abs(x) for x in self._art())
        for k in sm.CERT_ZERO:
            d[k] = 0
        status = self.result().status if self.published != "running" else "running"
        d.update(artificial_flow=art, big_m=self.big_m, bigm_term=self.big_m * art, basic_arcs=self.n, rc_compared=self.m, key_compared=0, status=status)
        d["gap"] = d["primal"] + d["bigm_term"] - d["dual"]
        clean = all(d[k] == 0 for k in ("dual_lower_count", "dual_upper_count")) and d["gap"] == 0
        d["verdict"] = ("infeasible" if art else "optimal") if clean else "not_proven"
        d["proves_status"] = status in ("optimal", "infeasible") and d["verdict"] == status
        return d

    def bottlenecks(self, num=1, den=1):
        flow, cap = np.ascontiguousarray(self.r["flow"], np.int64), np.ascontiguousarray(self.cap, np.int64)
        idx = np.zeros(max(self.m, 1), np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))                               # noqa: E731
        count = int(_libs()["certify"].mcf_bottlenecks_host(self.m, p(cap), p(flow), num, den, p(idx), self.m))
        return idx[:count], count

    def certify_ray(self, arc=-1):
        arc = int(self.r["unbounded_arc"]) if arc < 0 else arc
        return_ = tf.ray_host(_libs()["farkas"], self.inst(), self.r, arc, False, self._art())
        return_["arcs"] = np.asarray(return_["arcs"], np.int64)
        return return_

    def certify_cut(self, in_S=None):
        return tf.cut_host(_libs()["farkas"], self.inst(), self.r["flow"], self._art(), in_S)

    def cost_ranges(self, arcs=None):
        pl = types.SimpleNamespace(n=self.n, m=self.m, inst=self.inst(), state=self.state)
        tree = self.tree()
        down, up, rep = tr.ranges_host(_libs()["ranges"], pl, tree, tree["pi"])
        rep["big_m"] = self.big_m
        if arcs is not None:
            idx = np.asarray(arcs, np.int64)
            down, up = down[idx], up[idx]
        return down, up, rep

    def _flow_state(self):
        return fy.resident_state(self.inst(), self.tree(), self.r["flow"])

    def supply_ranges(self, src, dst):
        got = tfr.supply_host(_libs()["flow"], self._flow_state(), self.tree()["pi"], src, dst)
        got[4]["big_m"] = self.big_m
        return got

    def capacity_ranges(self, arcs=None):
        got = tfr.capacity_host(_libs()["flow"], self._flow_state(), self.state, self.cost, self.tree()["pi"])
        got[5]["big_m"] = self.big_m
        if arcs is not None:
            idx = np.asarray(arcs, np.int64)
            got = (*(a[idx] for a in got[:5]), got[5])
        return got


def _solve_batch(engines, max_pivots=None):
    for eng in engines:
        eng.solve(-1 if max_pivots is None else int(max_pivots))
    return 0.0


STAND_IN = types.SimpleNamespace(McfEngine=StandIn, EngineError=StandInError, solve_batch=_solve_batch)


# ------------------------------------------------------------------ the sessions of the GPU file, on the stand-in
def _gpu_cases():
    import test_gpu_sessions as tg
    return tg.CASES, tg.SEEDS


@pytest.mark.parametrize("family,rule", _gpu_cases()[0], ids=[f"{f}-{r}" for f, r in _gpu_cases()[0]])
def test_every_seed_list_of_the_gpu_file_passes_on_the_stand_in_with_a_complete_event_union(family, rule):
    sm.run_seeds(STAND_IN, family, rule, _gpu_cases()[1][family], STAND_IN_FLAGS)


@pytest.mark.parametrize("rule", list(sm.RULES))
def test_short_sessions_on_the_stand_in(rule):
    import test_gpu_sessions as tg
    for family, base, blocks in tg.SHORT_SESSIONS:
        s = sm.Session(STAND_IN, family, rule, 0, STAND_IN_FLAGS)
        sm.Planner(family, rule, 0, base=base, blocks=blocks).script(s)
        s.finish()
        assert not s.notes, s.notes


def _rc_drop_cases():
    import test_gpu_sessions as tg
    return tg.RC_DROP_CASES, tg.RC_DROP_BLOCKS


@pytest.mark.parametrize("share,rule", _rc_drop_cases()[0], ids=[f"{s}-{r}" for s, r in _rc_drop_cases()[0]])
def test_the_dropped_reduced_costs_sessions_on_the_stand_in(share, rule):
    blocks, required = _rc_drop_cases()[1][share]
    sm.run_seeds(STAND_IN, "rc_drop", rule, (1,), STAND_IN_FLAGS, required=required, blocks=blocks)


# ------------------------------------------------------------------ the generator and the model
def _script(seed):
    s = sm.Session(STAND_IN, "lds", "dantzig", seed, STAND_IN_FLAGS)
    sm.Planner("lds", "dantzig", seed).script(s)
    return s


def test_the_generator_is_deterministic_and_a_script_replays():
    a, b = _script(1), _script(1)
    assert a.steps == b.steps and a.events == b.events and len(a.steps) >= 20
    assert _script(3).steps != a.steps
    steps = eval(repr(a.steps))                        # the literal a failure prints
    again = sm.run_script(STAND_IN, "lds", "dantzig", steps, STAND_IN_FLAGS)
    assert again.events == a.events and again.steps == a.steps
    a.close(); b.close()


@pytest.mark.parametrize("seed", (1, 2))
def test_the_models_edits_equal_a_rebuild_from_scratch(seed):
    s = _script(seed)
    now, scratch = s.model.instance(), s.model.rebuild()
    assert now.m == scratch.m > s.model.base.m
    for k in ("tail", "head", "cost", "cap", "supply"):
        assert np.array_equal(getattr(now, k), getattr(scratch, k)), k
    assert s.model.big_m >= sm.big_m_of(now.n, now.cost)
    kinds = {e[0] for e in s.model.log}
    assert kinds == {"costs", "rhs", "add"}


def test_big_m_never_shrinks_and_the_model_refuses_magnitudes_the_oracle_cannot_hold():
    inst = generators.netgen_style(20, 60, seed=1)
    model = sm.SessionModel(inst)
    first = model.big_m
    assert first == (int(np.abs(inst.cost).max()) + 1) * 22
    a = int(np.argmax(np.abs(inst.cost)))
    model.update_costs([a, a], [5, 3 * int(inst.cost[a])])
    grown = model.big_m
    assert grown == (3 * int(inst.cost[a]) + 1) * 22 > first
    model.update_costs([a], [1])
    assert model.big_m == grown and model.cost[a] == 1
    model.update_costs([0], [sm.INT32_MAX])
    model.update_rhs([0, 1], [int(model.supply[0]) + (1 << 40), int(model.supply[1]) - (1 << 40)])
    with pytest.raises(AssertionError, match="exact range"):
        model.instance()


def test_a_failure_names_the_step_and_prints_a_replayable_script():
    s = sm.Session(STAND_IN, "lds", "devex", 7, STAND_IN_FLAGS)
    s.execute({"op": "base", "kind": "netgen", "n": 64, "m": 512, "seed": 3})
    s.execute({"op": "solve", "budget": -1})
    s.h.r["flow"][int(np.flatnonzero(s.h.state == 1)[0])] += 1          # the handle goes wrong behind the driver's back
    with pytest.raises(sm.SessionFailure) as err:
        s.execute({"op": "query", "what": "certify"})
    text = str(err.value)
    assert "family=lds rule=devex seed=7 step 2: {'op': 'query', 'what': 'certify'}" in text
    assert "run_script(engine_module, 'lds', 'devex', [{'op': 'base'," in text
    literal = text.split("run_script(engine_module, 'lds', 'devex', ", 1)[1].rsplit(")", 1)[0]
    assert eval(literal) == s.steps


# ------------------------------------------------------------------ planted defects: exactly one checker fails
@pytest.fixture(scope="module")
def planted():
    """A mid-solve state after an insertion (artificial arcs still basic), and the model it belongs to."""
    s = sm.Session(STAND_IN, "lds", "dantzig", 0, STAND_IN_FLAGS)
    s.execute({"op": "base", "kind": "netgen", "n": 64, "m": 512, "seed": 4})
    model = s.model
    model.add_arcs([1, 2, 3], [2, 3, 4], [7, 8, 9], [5, 5, 5])
    inst = model.instance()
    h = StandIn(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply)
    h.solve(20)
    snap = sm.snapshot(h)
    assert snap["status"] == "iteration_limit" and (snap["tree"]["pred_arc"][: inst.n] >= inst.m).any() and (snap["tree"]["pred_arc"][: inst.n] < inst.m).any()
    pi = snap["tree"]["pi"]
    viol = -sm.states_of(snap) * (inst.cost + pi[inst.tail] - pi[inst.head])
    snap["keys"] = np.array([oracle.emul_vkey(int(v), model.big_m, sm.VKEY_HALF) for v in viol.tolist()], np.int32)
    snap["present"] = True
    cert = dict(h.certify(), key_compared=inst.m)                         # (a handle that keeps key codes compares them all)
    assert sm.state_failures(inst, model.big_m, snap, True, cert, h.price_once(0)) == {}
    return model, inst, snap, cert, h


def _failing(planted, snap=None, cert=None, inst=None, big_m=None):
    model, inst0, snap0, cert0, h = planted
    return sorted(sm.state_failures(inst0 if inst is None else inst, model.big_m if big_m is None else big_m, snap0 if snap is None else snap,
                                    True, cert0 if cert is None else cert, h.price_once(0)))


def test_one_stale_reduced_cost(planted):
    snap = copy.deepcopy(planted[2])
    snap["rc"][17] += 1
    assert _failing(planted, snap) == ["reduced_costs"]


def test_one_stale_key_code(planted):
    snap = copy.deepcopy(planted[2])
    snap["keys"][int(np.flatnonzero(snap["keys"] > 0)[0])] -= 1
    assert _failing(planted, snap) == ["key_codes"]


def test_one_pred_word_not_remapped_after_an_insertion(planted):
    model, inst, snap0, _, _ = planted
    snap = copy.deepcopy(snap0)
    pred = snap["tree"]["pred_arc"]
    v = int(np.flatnonzero(pred[: inst.n] >= inst.m)[-1])
    pred[v] = (inst.m - 3) + v                                            # what it was before the three arcs came
    assert _failing(planted, snap) == ["tree"]


def test_one_devex_weight_off_one(planted):
    snap = copy.deepcopy(planted[2])
    snap["weights"][3] = 2.0
    assert _failing(planted, snap) == ["weights"]
    assert sm.state_failures(planted[1], planted[0].big_m, snap, False) == {}     # (only an edit restarts the weights)


def test_a_supply_not_applied(planted):
    model, inst, _, _, _ = planted
    later = model.copy()
    pred = planted[2]["tree"]["pred_arc"]
    x, y = (int(v) for v in np.flatnonzero(pred[: inst.n] < inst.m)[:2])  # nodes on real tree arcs: no artificial arc absorbs it
    later.update_rhs([x, y], [int(inst.supply[x]) + 1, int(inst.supply[y]) - 1])
    assert _failing(planted, inst=later.instance()) == ["flows"]


def test_a_flow_above_its_capacity(planted):
    model, inst, snap0, _, _ = planted
    snap = copy.deepcopy(snap0)
    a = int(np.flatnonzero(sm.states_of(snap) == 0)[0])
    snap["flow"][a] = inst.cap[a] + 1
    assert _failing(planted, snap) == ["flows"]


def _at_the_later_big_m(planted):
    """The planted state as a handle holds it once a cost raised big-M: every subtree on an artificial arc has moved."""
    model, inst, snap0, cert0, _ = planted
    later = model.copy()
    later.update_costs([0], [2 * int(np.abs(inst.cost).max())])
    assert later.big_m > model.big_m
    inst1 = later.instance()
    snap = copy.deepcopy(snap0)
    shift = later.big_m - model.big_m
    tree = snap["tree"]
    pi, pos, size, order = tree["pi"], tree["pos"], tree["size"], tree["order"]
    pred, par = tree["pred_arc"], tree["parent"]
    moved = pi.copy()
    for v in order[1:].tolist():                                           # preorder: a parent comes before its children
        a, p = int(pred[v]), int(par[v])
        if a >= inst1.m:
            moved[v] = moved[p] + (later.big_m if pi[v] > pi[p] else -later.big_m)
        else:
            moved[v] = moved[p] - int(inst1.cost[a]) if inst1.tail[a] == v else moved[p] + int(inst1.cost[a])
    tree["pi"] = moved
    snap["potential"] = moved[: inst.n] - moved[inst.n]
    snap["rc"] = inst1.cost + moved[inst1.tail] - moved[inst1.head]
    viol = -sm.states_of(snap) * snap["rc"]
    snap["keys"] = np.array([oracle.emul_vkey(int(v), later.big_m, sm.VKEY_HALF) for v in viol.tolist()], np.int32)
    art = cert0["artificial_flow"]
    want = sm.pt.np_cert(inst1, inst1.cost, snap["flow"], snap["potential"])
    cert = dict(cert0, big_m=later.big_m, bigm_term=later.big_m * art, **{k: want[k] for k in want if not k.startswith("imbalance") and k != "gap"})
    cert["gap"] = cert["primal"] + cert["bigm_term"] - cert["dual"]
    assert sm.state_failures(inst1, later.big_m, snap, True, cert) == {}
    return later, inst1, snap, cert, shift


def test_the_handles_big_m_word_one_step_behind(planted):
    later, inst1, snap, cert, _ = _at_the_later_big_m(planted)
    stale = dict(cert, big_m=planted[0].big_m)
    assert sorted(sm.state_failures(inst1, later.big_m, snap, True, stale)) == ["big_m"]


def test_the_potentials_below_one_artificial_arc_at_the_old_big_m(planted):
    later, inst1, snap, cert, shift = _at_the_later_big_m(planted)
    tree = snap["tree"]
    v = int(np.flatnonzero(tree["pred_arc"][: inst1.n] >= inst1.m)[0])
    below = tree["order"][tree["pos"][v]: tree["pos"][v] + tree["size"][v]]
    pi = tree["pi"]
    pi[below] += -shift if pi[v] > pi[inst1.n] else shift                  # that subtree stayed where the old big-M put it
    snap["potential"] = pi[: inst1.n] - pi[inst1.n]
    snap["resident"] = snap["present"] = False                             # (a handle without resident pricing data: one word, one checker)
    assert sorted(sm.state_failures(inst1, later.big_m, snap, True, cert)) == ["potentials"]


def test_an_all_arcs_range_buffer_of_the_old_length(planted):
    model, inst, snap, _, h = planted
    down, up, _ = h.cost_ranges()
    assert sm.check_range_arrays((down, up), inst.m) is None
    msg = sm.check_range_arrays((down[: inst.m - 3], up), inst.m)
    assert msg and str(inst.m - 3) in msg


def test_a_range_off_by_one(planted):
    model, inst, snap, _, h = planted
    down, up, _ = h.cost_ranges()
    want = sm.cost_ranges_want(inst, model.big_m, snap)
    assert sm.check_ranges((down, up), want[:2], ("down", "up")) is None
    bad = up.copy()
    i = int(np.flatnonzero(bad != sm.RINF)[0])
    bad[i] += 1
    msg = sm.check_ranges((down, bad), want[:2], ("down", "up"))
    assert msg and msg.startswith(f"up differs at [{i}]")
    cap = h.capacity_ranges()
    want = fy.capacity_ranges(sm.flow_state(inst, snap), snap["tree"]["state"], inst.cost, snap["tree"]["pi"])
    names = ("down", "up", "down_arc", "up_arc", "rate")
    assert sm.check_ranges(cap[:5], want[:5], names) is None
    worse = [a.copy() for a in cap[:5]]
    worse[2][5] += 1
    assert sm.check_ranges(worse, want[:5], names).startswith("down_arc differs at [5]")


def test_a_read_only_query_that_changed_one_word(planted):
    snap = planted[2]
    assert sm.check_read_only(snap, copy.deepcopy(snap)) is None
    for path in (("tree", "pi"), ("tree", "pred_arc"), ("weights",), ("rc",), ("flow",), ("keys",)):
        after = copy.deepcopy(snap)
        target = after
        for k in path:
            target = target[k]
        target[2] += 1
        assert sm.check_read_only(snap, after) == f"a read-only call changed {['.'.join(path)]}"
    after = copy.deepcopy(snap)
    after["stats"]["pivots"] += 1
    assert "stats.pivots" in sm.check_read_only(snap, after)


def test_the_pricing_checker_sees_a_pivot_that_a_sweep_from_scratch_would_not_select(planted):
    model, inst, snap, cert, h = planted
    hit = h.price_once(0)
    assert hit is not None and sm.check_pricing(inst, snap, hit) is None
    assert sm.check_pricing(inst, snap, None) and sm.check_pricing(inst, snap, (hit[0] + 1, hit[1], hit[2])) and sm.check_pricing(inst, snap, (hit[0], hit[1], hit[2] - 1))


# ------------------------------------------------------------------ the same defects through the driver's query path
class _Defective(StandIn):
    """A stand-in whose queries go wrong in one chosen way."""
    defect = None

    def cost_ranges(self, arcs=None):
        down, up, rep = super().cost_ranges(arcs)
        if arcs is None and self.defect == "old_length":
            return down[:-3], up[:-3], rep
        if arcs is None and self.defect == "off_by_one":
            up = up.copy()
            up[int(np.flatnonzero(up != sm.RINF)[0])] += 1
        return down, up, rep

    def capacity_ranges(self, arcs=None):
        got = super().capacity_ranges(arcs)
        if self.defect == "writes":
            self.r["potential"][1] += 1                                    # a "read-only" call that changes one word
        return got


@pytest.mark.parametrize("defect,what,message", [
    ("old_length", "cost_ranges", "all-arcs range arrays of lengths"),
    ("off_by_one", "cost_ranges", "up differs at"),
    ("writes", "capacity_ranges", "a read-only call changed"),
])
def test_the_driver_reports_a_defective_query(defect, what, message):
    module = types.SimpleNamespace(McfEngine=_Defective, EngineError=StandInError, solve_batch=_solve_batch)
    s = sm.Session(module, "lds", "dantzig", 0, STAND_IN_FLAGS)
    s.execute({"op": "base", "kind": "netgen", "n": 64, "m": 512, "seed": 4})
    s.execute({"op": "solve", "budget": -1})
    s.execute({"op": "query", "what": what, "arcs": [1, 2, 2]})           # the stand-in as it is: passes
    s.h.defect = defect
    with pytest.raises(sm.SessionFailure, match=message) as err:
        s.execute({"op": "query", "what": what, "arcs": [1, 2, 2]})
    assert f"step 3: {{'op': 'query', 'what': '{what}'" in str(err.value)
