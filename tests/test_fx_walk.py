"""The walk order of the persistent stage 1 (pypulsar_amd/csrc/fx_walk.h) on
the CPU: tests/native/fx_walk_check.cpp drains the kernel's per-XCD item
queues with workgroups in a scrambled order and checks that every (group,
element block) item is visited exactly once -- for group counts below 8, odd,
around the 256-group permuted run, and grids larger than the item count --
and that the slot -> group permutation is a bijection with the XCD shares the
header promises.  Built plain and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sweep_plan import _cxx

CSRC = os.path.join(ROOT, "pypulsar_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "fx_walk_check.cpp")


def _build(name, extra):
    out = os.path.join(ROOT, "build", name)
    deps = [SRC, os.path.join(CSRC, "fx_walk.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(map(os.path.getmtime, deps)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.check_call([_cxx(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC] + extra
                              + ["-o", tmp, SRC])
        os.replace(tmp, out)
    return out


@pytest.mark.parametrize("name,extra", [
    ("fx_walk_check", []),
    ("fx_walk_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
])
def test_every_item_once(name, extra):
    exe = _build(name, extra)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()
    assert b"fx_walk ok" in r.stdout
