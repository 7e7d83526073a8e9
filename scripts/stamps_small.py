"""Diagnostic: phase shares of the fused small-instance kernel (build with -DMCF_STAMPS; with -DMCF_WAVE_STAMPS on top, every wave's own clocks)."""
import ctypes, os, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
os.environ.setdefault("MCF_HIP_LIB", str(ROOT / "scripts" / "libmcf_stamps.so"))   # (a -DMCF_STAMPS build; preset it for A/B builds)
sys.path.insert(0, str(ROOT))
import numpy as np
from network_flow_solver_amd import engine, generators
inst = generators.named_instance("netgen_8_08a")
for rule in (0, 1, 2):
    eng = engine.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply, rule=rule)
    eng.solve()
    st = eng.stats()
    out = (ctypes.c_ulonglong * 8)()
    eng._lib.mcf_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    eng._lib.mcf_debug_stamps(eng._h, out)
    v = np.array(list(out), dtype=np.float64)
    names = ["copy_in", "price", "argmax", "walk", "finish", "apply", "copy_out", "fin_last"]   # fin_last: the finishing (last) wave's own clock over its finish pass
    piv = max(st["pivots"], 1)
    print("rule", rule, "pivots", piv, "solve_s", st["solve_seconds"], "ticks/pivot in loop", v[1:6].sum() / piv)
    for n, x in zip(names, v):
        print(f"   {n:9s} {x:14.0f}  per pivot {x / piv:9.1f}  share {100 * x / v.sum():5.1f}%")
    out2 = (ctypes.c_ulonglong * 24)()
    eng._lib.mcf_debug_pivot_stamps.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    eng._lib.mcf_debug_pivot_stamps(eng._h, out2, 1)
    w = np.array(list(out2), dtype=np.float64)
    for n, x in zip(["(to walk start)", "begin", "cycle_init", "climb", "decide"], w[12:17]):
        print(f"      walk/{n:16s} per pivot {x / piv:9.1f}")
    if hasattr(eng._lib, "mcf_debug_wave_stamps"):   # every wave's own clock from the top of the iteration (an A/B library of an earlier commit lacks it)
        out3 = (ctypes.c_ulonglong * 96)()
        eng._lib.mcf_debug_wave_stamps.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
        eng._lib.mcf_debug_wave_stamps(eng._h, out3)
        u = np.array(list(out3), dtype=np.float64).reshape(16, 6)
        waves = int(os.environ.get("MCF_SMALL_THREADS", "256")) // 64
        for q in range(waves):
            print(f"      wave {q:2d} per pivot: at search barrier {u[q, 0] / piv:8.1f}  behind ratio tests {u[q, 1] / piv:8.1f}  behind decide {u[q, 2] / piv:8.1f}"
                  f"  behind apply {u[q, 3] / piv:8.1f}  behind finish {u[q, 4] / piv:8.1f}")
        last = int(np.argmax(u[:waves, 3]))
        print(f"      last at the end barrier: wave {last}, {(u[last, 3] - np.sort(u[:waves, 3])[-2]) / piv:.1f} behind the next")
        if u[1, 5]:
            print(f"      one dependent broadcast LDS read: {u[0, 5] / u[1, 5]:.1f} cycles (mean of {int(u[1, 5])} probes)")
    eng.close()
