#!/usr/bin/env python3
"""Explicit central-difference steps on the stretched, jittered Kuhn cube (prints one JSON line).

Mesh, material and clamp of tools/bench_transient.py: mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2), the z = 0
face clamped, Ti-6Al-4V (E = 113.8e9, nu = 0.342, rho = 4430), 1e6 N in x spread over the far face applied suddenly;
n = 55 (1.0M tets) and n = 119 (10.1M tets). For every material ("linear", "svk", "neo_hookean"): a warm-up run, then
`--steps` (>= 200) steps at dt = 0.9 x the guaranteed stable step in ONE system.ExplicitDynamics.run between two device
events, ending in a synchronise: milliseconds per step, steps/s and element updates/s.

Two yardsticks from code that exists without the explicit path, on the same mesh in the same process:
  matvec_ms   one MatFreeOperator.matvec (chunk kernel + gather), the mean of 50 between device events
  newmark_ms  one implicit Newmark step (system.NewmarkIntegrator on the assembled K, lumped diagonal mass,
              dt = 1 / (20 f_1), rtol 1e-8), the mean of `--newmark-steps`; --no-newmark skips the assembly
and the ratio of the linear step to the matvec.

    python tools/bench_explicit.py --cube-n 55 > profiles/explicit_n55.json
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import element, mesh, solver, system  # noqa: E402

E, NU, RHO = 113.8e9, 0.342, 4430.0
F1 = {55: 134.85, 119: 134.36}
F64 = torch.float64
MATERIALS = ("linear", "svk", "neo_hookean")


def timed(fn, reps):
    """Mean milliseconds of fn() over `reps` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run_material(coords, tets, mask, F, material, steps, warmup):
    xd = system.ExplicitDynamics(coords, tets, RHO, E, NU, material, mask)
    try:
        dt = 0.9 * xd.stable_dt()[0]
        xd.start(F=F)
        xd.run(warmup, dt, F, 1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        res = xd.run(steps, dt, F, 1.0)    # + one force evaluation for the state reached
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / (steps + 1)
        out = {"dt": dt, "steps": steps, "ms_per_step": ms, "steps_per_s": 1e3 / ms,
               "element_updates_per_s": tets.shape[0] * 1e3 / ms, "status": res.status,
               "u_max": float(xd.u.abs().max()), "chunks": xd.op.info()["chunks"]}
        if material == "linear":
            x = torch.randn(xd.n, dtype=F64, device=coords.device)
            y = torch.empty_like(x)
            xd.op.matvec(x, y)
            out["matvec_ms"] = timed(lambda: xd.op.matvec(x, y), 50)
            out["step_over_matvec"] = ms / out["matvec_ms"]
        assert math.isfinite(out["u_max"]) and res.status == system.XD_OK
        return out, xd.mass.clone()
    finally:
        xd.close()


def run_newmark(coords, tets, mask, F, mass, f1, steps):
    N = coords.shape[0]
    K = element.compute_c3d4_K_matrix(coords, tets, E, NU, device=coords.device, dtype=F64)
    A = system.SellMatrix(solver.cached_graph(tets, N), 3)
    A.add_element_matrices(K, tets)
    del K
    dt = 1.0 / (20.0 * f1)
    integ = system.NewmarkIntegrator(A, mass.repeat_interleave(3).contiguous(), mask, dt, tol=0.0, rtol=1e-8,
                                     max_iter=20000)
    try:
        integ.start(None, None, F)
        integ.step(F, 1.0)
        integ.start(None, None, F)
        its = []

        def step():
            it, stt = integ.step(F, 1.0)
            if stt != C.PCG_CONVERGED:
                raise SystemExit(f"Newmark step stopped with status {stt} after {it} iterations")
            its.append(it)
        ms = timed(step, steps)
        return {"dt": dt, "steps": steps, "ms_per_step": ms, "iterations_mean": sum(its) / len(its)}
    finally:
        integ.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--newmark-steps", type=int, default=3)
    ap.add_argument("--no-newmark", action="store_true")
    a = ap.parse_args()
    if a.steps < 200:
        raise SystemExit("--steps must be >= 200")
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)
    fixed, far = mesh.face_nodes(coords, 2, 0.0), mesh.face_nodes(coords, 2, 2.0)
    N = coords.shape[0]
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    mask = mask.view(-1)
    F = torch.zeros((N, 3), dtype=F64, device=dev)
    F[far, 0] = 1e6 / far.numel()
    F = F.view(-1).contiguous()
    out = {"tool": "bench_explicit", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "dofs": 3 * N}
    mass = None
    for m in MATERIALS:
        out[m], mass = run_material(coords, tets, mask, F, m, a.steps, a.warmup)
    if not a.no_newmark:
        out["newmark"] = run_newmark(coords, tets, mask, F, mass, F1.get(a.cube_n, F1[55]), a.newmark_steps)
        out["newmark_over_linear_step"] = out["newmark"]["ms_per_step"] / out["linear"]["ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
