"""bench.py --dump-outputs through the command line: a plain run of the small
config writes the plane its last timed step returned -- the same elements
dump_outputs() keeps of a plane computed here from the same seeded block --
and prints the usual result line."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_its_last_plane(gpu, tmp_path):
    import torch
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config",
                        "small", "--steps", "1", "--warmup", "0", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 1 and line["warmup"] == 0 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["cpu_baseline"] is None and "end_to_end_pcie" not in line   # --full only
    assert os.listdir(out) == ["plane.npy"]
    got = np.load(os.path.join(out, "plane.npy"))
    assert got.dtype == np.float32 and got.nbytes <= 64 * 10 ** 6

    spec = importlib.util.spec_from_file_location("bench_gpu_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from pypulsar_amd.sweep import DMSweep
    cfg = bench.CONFIGS["small"]
    C, N, D = cfg["C"], cfg["N"], cfg["D"]
    x = bench.synth_block(C, N, 1000, "f32", gpu)
    sw = DMSweep(np.linspace(cfg["dm_lo"], cfg["dm_hi"], D), bench.band(C), 64e-6, dtype="f32")
    plane = torch.empty((D, sw.n_out(N)), dtype=torch.float32, device=gpu)
    sw(x, out=plane)
    torch.cuda.synchronize()
    assert line["config"]["n_out"] == plane.shape[1]
    ref = str(tmp_path / "ref")
    bench.dump_outputs(ref, [("plane", plane)])
    want = np.load(os.path.join(ref, "plane.npy"))
    sw.close()
    assert got.shape == want.shape and got.shape[0] == D
    # (integer-valued block: the float32 sums are exact, so the planes are equal)
    assert np.array_equal(got, want)
