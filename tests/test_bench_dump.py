"""bench.py --dump-outputs (dump_outputs): every array lands as float32 (or
float64) .npy within the byte budget; an array above its share is sampled at
the same elements on every run, a plane keeping every row and its first and
last columns.  Host logic only (CPU tensors)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return [("plane_0", torch.randn((7, 501), generator=g)),                 # sampled by column
            ("plane_1", torch.randn((3, 40), generator=g)),                  # whole
            ("bytes", torch.randint(0, 255, (5000,), generator=g).to(torch.uint8)),  # flat sample
            ("wide", torch.randn((2, 8), generator=g).double())]            # float64 stays


def test_dump_is_bounded_typed_and_repeatable(bench, tmp_path, monkeypatch):
    budget = 4 * 1024
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    named = _arrays(3)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, named)
    bench.dump_outputs(b, named)
    got = {n: np.load(os.path.join(a, n + ".npy")) for n, _ in named}
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n, _ in named)
    assert sum(v.nbytes for v in got.values()) <= budget
    for n, _ in named:
        assert np.array_equal(got[n], np.load(os.path.join(b, n + ".npy")))
    assert got["plane_0"].dtype == np.float32 and got["bytes"].dtype == np.float32
    assert got["wide"].dtype == np.float64
    assert np.array_equal(got["plane_1"], named[1][1].numpy())
    assert np.array_equal(got["wide"], named[3][1].numpy())
    # the plane: every row, first and last column, columns in order
    p, full = got["plane_0"], named[0][1].numpy()
    assert p.shape[0] == 7 and 2 <= p.shape[1] < 501
    assert np.array_equal(p[:, 0], full[:, 0]) and np.array_equal(p[:, -1], full[:, -1])
    cols = [int(np.flatnonzero((full == p[:, j:j + 1]).all(axis=0))[0]) for j in range(p.shape[1])]
    assert cols == sorted(set(cols))
    # the flat sample: elements of the array, in order
    assert got["bytes"].size < 5000 and set(got["bytes"]) <= set(named[2][1].float().numpy())


def test_dump_sample_depends_on_shape_not_values(bench, tmp_path, monkeypatch):
    """Two builds' outputs are compared element for element: another plane of
    the same shape is sampled at the same columns."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1024)
    x = torch.arange(4 * 300, dtype=torch.float32).view(4, 300)
    bench.dump_outputs(str(tmp_path / "x"), [("p", x)])
    bench.dump_outputs(str(tmp_path / "y"), [("p", x + 0.5)])
    px, py = np.load(str(tmp_path / "x" / "p.npy")), np.load(str(tmp_path / "y" / "p.npy"))
    assert px.shape == py.shape and np.array_equal(px + 0.5, py)


def test_dump_names_ranks(bench, tmp_path):
    bench.dump_outputs(str(tmp_path), [("plane", torch.zeros(2, 2))], world=2, rank=1)
    assert os.listdir(str(tmp_path)) == ["plane_rank1.npy"]


def test_dump_real_budget_counts_the_files(bench, tmp_path):
    """Four planes as the default workload returns them (every row kept, here
    narrower) at the real budget: the files, headers included, stay under
    64 MB and share it equally."""
    named = [("plane_%d" % k, torch.full((4096, 5000), k, dtype=torch.uint8)) for k in range(4)]
    bench.dump_outputs(str(tmp_path), named)
    sizes = [os.path.getsize(str(tmp_path / (n + ".npy"))) for n, _ in named]
    assert sum(sizes) <= 64 * 10 ** 6 and len(set(sizes)) == 1
    p = np.load(str(tmp_path / "plane_3.npy"))
    assert p.shape == (4096, bench.DUMP_BUDGET // 4 // 4 // 4096) and (p == 3).all()


def test_dump_refused_for_a_rehearsal():
    """--rehearse returns no step output: the option is an error there, before
    any GPU call."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rehearse", "2",
                        "--dump-outputs", "unused"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
