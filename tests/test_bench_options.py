"""bench.py's options: a plain run carries the headline only (the secondary measurements need ``--full``), and
``--dump-outputs DIR`` writes what the engine returns after the last timed pivot."""

import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import bench
from conftest import ROOT


def test_bench_lists_full_and_dump_outputs():
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert "--full" in proc.stdout and "--dump-outputs" in proc.stdout


def test_dump_outputs_writes_float_arrays_and_samples_long_ones(tmp_path):
    m, n = bench.DUMP_MAX_ENTRIES + 1000, 300
    res = SimpleNamespace(flow=np.arange(m, dtype=np.int64), potential=-np.arange(n, dtype=np.int64),
                          in_tree=(np.arange(m) % 3 == 0), objective=123456789)
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    total = 0
    for name in ("flow", "potential", "in_tree", "objective"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and a.ndim == 1
        assert np.array_equal(a, b), name                     # the sample is fixed: same arguments, same files
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    flow = np.load(tmp_path / "a" / "flow.npy")
    assert 0 < flow.shape[0] <= bench.DUMP_MAX_ENTRIES and (np.diff(flow) > 0).all()    # sorted distinct entries of flow
    in_tree = np.load(tmp_path / "a" / "in_tree.npy")
    assert np.array_equal(in_tree, (flow % 3 == 0).astype(np.float32))                  # the same indices in every array
    assert np.array_equal(np.load(tmp_path / "a" / "potential.npy"), -np.arange(n, dtype=np.float64))
    assert np.load(tmp_path / "a" / "objective.npy").tolist() == [123456789.0]


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_engine_returns_after_the_timed_pivots(gpu_engine_module, tmp_path):
    """A plain run: headline keys only, ``steps`` timed pivots; its dump equals the result of the same pivots
    (W warm-up, then K) run here on the same seeded instance."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "MCF_BENCH_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "20",
           "--dump-outputs", str(tmp_path / "out")]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = json.loads(proc.stdout.strip().splitlines()[-1])
    assert line["steps"] == 100 and line["ms_per_step"] > 0 and line["value"] > 0
    for key in ("hbm_point", "config_points", "batched_point", "cpu_baseline"):
        assert key not in line, key

    inst = bench.make_instance("netgen_8_08a")
    with gpu_engine_module.McfEngine(inst.n, inst.tail, inst.head, inst.cost, inst.cap, inst.supply,
                                     rule=gpu_engine_module.RULE_DANTZIG, device=0, full_sweeps=1) as eng:
        bench.run_pivots(eng, 20)
        bench.run_pivots(eng, 100)
        res = eng.result()
    out = tmp_path / "out"
    assert np.array_equal(np.load(out / "flow.npy"), res.flow.astype(np.float64))
    assert np.array_equal(np.load(out / "potential.npy"), res.potential.astype(np.float64))
    assert np.array_equal(np.load(out / "in_tree.npy"), res.in_tree.astype(np.float32))
    assert np.load(out / "objective.npy").tolist() == [float(res.objective)]
