"""The fused LDS loop's straight-line decide (``csrc/mcf_core.h``: ``mcf_pivot_decide_flat``) against ``mcf_pivot_decide`` on the
host: ``csrc/mcf_decide_flat_host.cpp`` runs the two functions from the same control block, cycle and path arrays and compares the
two control blocks they leave with ``memcmp``, over an enumeration of pivots -- residuals of either side and the entering arc's
capacity each from {0, 1, 5, 2^32 - 2, 2^32 + 5, MCF_INF} (every tie, the degenerate step, the unbounded cycle), both states, both
parities of the leaving arc's direction bit, the leaving node first, second and last on its side, -1 on the side that does not
leave, a re-hung subtree of one and of three nodes, and seven placements of the new parent against the subtree.  The descriptor
fields of the start hold non-zero junk.  No GPU.

One test builds that file and a stand-alone program round it with the compiler's address and undefined-behaviour checks and runs
the program on the same enumeration.  The last tests vet the inputs of ``test_gpu_small_loop_decide.py``."""

from __future__ import annotations

import ctypes
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

N_COUNTS = 24
CASES = 6 * 6 * 6 * 2 * 2 * 2 * 3 * 2 * 7


@pytest.fixture(scope="module")
def counts():
    lib = ctypes.CDLL(str(ge.build_decide_flat_host()))
    lib.mcf_decide_flat_sweep_host.argtypes = [ctypes.c_void_p]
    lib.mcf_decide_flat_sweep_host.restype = ctypes.c_int
    buf = (ctypes.c_int64 * N_COUNTS)()
    rc = lib.mcf_decide_flat_sweep_host(ctypes.cast(buf, ctypes.c_void_p))
    return rc, list(buf)


def test_flat_decide_leaves_the_control_block_of_decide(counts):
    rc, c = counts
    assert rc == 0 and c[1] == 0, f"first mismatch: case {c[22]}, byte {c[23]} of McfCtx; {c[1]} of {c[0]} cases differ"
    assert c[0] == CASES


def test_enumeration_holds_every_exit_and_edge(counts):
    _, c = counts
    unbounded, flips, first, second, degenerate = c[2:7]
    # all three at or above MCF_INF: one combination of the 216
    assert unbounded == CASES // 216
    assert flips > 0 and first > 0 and second > 0 and degenerate > 0
    assert unbounded + flips + first + second == c[0]
    t_a, t_b, tie, before, at_end, behind = c[7:13]
    assert t_a > 0 and t_b > 0 and tie > 0 and before > 0 and at_end > 0 and behind > 0
    assert before + at_end + behind == first + second
    one_first, one_second, minus, k0, k1, klast = c[13:19]
    assert one_first > 0 and one_second > 0 and minus > 0
    assert k0 > 0 and k1 > 0 and klast > 0 and k0 + k1 + klast == first + second
    assert c[19] == 3 and c[20] == 3            # both parities of the direction bit, both states
    assert c[21] > 0 and c[21] + one_first + one_second == first + second


def test_stand_alone_program_with_address_and_ub_checks(tmp_path, counts):
    """The same code, compiled together with a program of its own with -fsanitize=address,undefined, on the same enumeration."""
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path / "decide_flat_driver"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ge.CSRC / "mcf_decide_flat_driver.cpp"), str(ge.CSRC / "mcf_decide_flat_host.cpp")], check=True,
                   cwd=str(ge.CSRC))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert [int(x) for x in r.stdout.split()] == counts[1]


# ------------------------------------------------------------------ the inputs of test_gpu_small_loop_decide.py
def test_gpu_plants_are_what_their_names_say():
    import planted_pivots as pp
    import small_loop_decide_instances as di

    for name, (_, what, degenerate) in di.PLANTS.items():
        p = di.plant(name)
        snaps, _, status, total = di.trajectory(name)
        s = snaps[0]
        assert p.inst.n <= 70 and status == "optimal" and total >= len(snaps) == pp.K_PIVOTS, name
        assert s["deep"] > 3, name                                    # decided behind the node-parallel search
        assert s["leaving"] == p.leaving and bool(s["flip"]) == (what == "flip") and bool(s["degenerate"]) == degenerate, name
        if what != "flip":
            assert s["t2"] == p.t2 and (p.first == p.u) == (what == "first"), name
    assert di.plant("one_node_first_side").t2 == di.plant("one_node_second_side").t2 == 1
    assert di.plant("stem_1").stem == 1 and di.plant("stem_3").stem >= 3
    # the ties: every named residual equals theta
    assert set(di.PLANTS["all_three_tie_second_leaves"][0]["ties"]) == {"first", "entering", "second"}
    assert set(di.PLANTS["capacity_ties_first_side_flip"][0]["ties"]) == {"first", "entering"}
    assert di.trajectory("degenerate_first_side")[0][0]["theta"] == 0
    # a bound flip directly behind a swap, both decided behind the parallel search
    a, b = di.trajectory("flip_behind_a_swap")[0][:2]
    assert not a["flip"] and b["flip"] and a["deep"] > 3 and b["deep"] > 3
    # the insertion point
    for name, want in di.INSERTIONS.items():
        t_a, t_b, cost_a, cost_b = di.insertion(name)
        got = "same" if t_a == t_b else ("tie" if cost_a == cost_b else ("tA" if cost_a < cost_b else "tB"))
        assert got == want, (name, t_a, t_b, cost_a, cost_b)


def test_gpu_unbounded_and_stepped_inputs():
    import small_loop_control_instances as ci
    import small_loop_decide_instances as di

    for name in di.UNBOUNDED:
        for rule in (0, 1, 2):
            em = ci.emul(di.unbounded(name), rule)
            assert em["status"] == "unbounded" and em["pivots"] - em["bound_flips"] >= 1, (name, rule)
    for n, m in di.STEPPED_SHAPES:
        inst = di.stepped(n, m)
        assert ci.fits_lds(inst.n, len(inst.tail))
        for rule in (0, 1, 2):
            em = ci.emul(inst, rule)
            assert em["status"] == "optimal" and em["pivots"] > di.STEPS and em["bound_flips"] > 0 and em["degenerate"] > 0, (n, m, rule)


def test_traits_are_the_kernels():
    """The kernels that take the straight-line decide, store the descriptor once behind the loop and read the ratio tests' inputs
    in one trip, as test_gpu_small_loop_decide.py's docstring and DESIGN.md state them."""
    text = (ge.CSRC / "mcf_engine.hip").read_text()
    assert "constexpr bool small_decide_flat(int threads, bool front) { return threads == 256 && front; }" in text
    assert "constexpr bool small_desc_once(int threads, bool front) { return threads == 256; }" in text
    assert "constexpr bool small_ratio_one_trip(int threads) { return threads == 256; }" in text
