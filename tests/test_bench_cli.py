"""bench.py's command line: a plain run measures the headline figure only (the companions and baselines sit behind
--full), --steps sets the timed steps, and --dump-outputs writes the timed path's iterate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("dofs_per_s", "solve_iters", "assembly_roofline", "cpu_baseline", "elasticity", "mixed", "config1")


def _parse(monkeypatch, *argv):
    monkeypatch.syspath_prepend(ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_the_companions_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert not (a.elastic or a.mixed or a.config1) and a.no_cpu_baseline


def test_full_run_keeps_the_companions(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert a.elastic and a.mixed and a.config1 and a.matfree and a.reference_api and not a.no_cpu_baseline
    a = _parse(monkeypatch, "--full", "--elastic", "0", "--no-cpu-baseline")
    assert not a.elastic and a.mixed and a.no_cpu_baseline


@pytest.mark.gpu
def test_plain_run_line_and_dumped_iterate(gpu, tmp_path):
    """`bench.py --gpus 1 --n 20 --steps 5 --warmup 2 --dump-outputs DIR`: one JSON line with the headline keys and
    none of --full's, and DIR/x.npy = the Jacobi-PCG iterate after 7 iterations of the same system (fp64; against
    `SellMatrix.pcg` with tol 0 in this process, 1e-12: both run the same kernels, the launches split differently)."""
    from fem355 import mesh, system
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--n", "20", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "CG iterations/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["value"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    assert not [k for k in FULL_ONLY if k in d], sorted(d)
    assert sorted(os.listdir(tmp_path)) == ["x.npy"]
    x = np.load(tmp_path / "x.npy")
    c, t = mesh.kuhn_cube(20, device=gpu)
    assert x.dtype == np.float64 and x.shape == (c.shape[0],)
    f, fixed = mesh.cube_poisson_case(c)
    A = system.assemble_tet4_system(c, t, "poisson", 1.0, 0.0)
    mask = torch.zeros(A.n, dtype=torch.uint8, device=gpu)
    mask[fixed] = 1
    b = f.reshape(-1).to(torch.float64)
    res = A.pcg(b, None, w=A.jacobi(mask), tol=0.0, max_iter=7)
    assert res.iterations == 7
    ref = res.x.cpu().numpy()
    assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()
