#!/usr/bin/env python3
"""Transient response of the stretched, jittered Kuhn cube (prints one JSON line).

Mesh, material and clamp of tools/bench_modal.py: mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2), the z = 0 face
clamped, Ti-6Al-4V (E = 113.8e9, nu = 0.342, rho = 4430), consistent mass. A load of 1e6 N in x spread over the far
face is applied suddenly at t = 0 and held; dt = 1 / (20 f_1) with f_1 the first natural frequency of DESIGN §8k
(134.85 Hz at n = 55, 134.36 Hz at n = 119; --f1 overrides), 40 steps of average-acceleration Newmark, no damping,
every step solved to rtol 1e-8 of its own right-hand side.

Default mode: system.NewmarkIntegrator, once per warm start (x0 = u_n, and the predictor x0 = u_n + dt v_n). Per step:
PCG iterations (mean, max), milliseconds of the right-hand side, the solve and the update between HIP events, and wall
time. FEM355_SL=0 in the environment keeps K and K_eff in the plain planes, so the solver context rebuilds its paired
copy at every start: the difference in the solve's milliseconds is the per-start conversion cost.

--naive writes the same loop with the public pieces that exist without the integrator: K_eff formed by editing `vals`
in torch, the right-hand side by separate matvecs, SellMatrix.pcg once per step, the update in torch. It imports
nothing the integrator added, so it runs on a checkout without it: same box, same mesh, same run.

    python tools/bench_transient.py --cube-n 55 > profiles/transient_n55.json
    python tools/bench_transient.py --cube-n 55 --naive
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import element, mesh, solver, system  # noqa: E402

E, NU, RHO = 113.8e9, 0.342, 4430.0
F1 = {55: 134.85, 119: 134.36}
F64 = torch.float64


def stats(its, ev, wall, steps):
    ms = [[a.elapsed_time(b) for a, b in zip(e[:-1], e[1:])] for e in ev]
    mean = lambda k: sum(m[k] for m in ms) / len(ms)
    return {"steps": steps, "iterations_mean": sum(its) / len(its), "iterations_max": max(its),
            "rhs_ms": mean(0), "solve_ms": mean(1), "update_ms": mean(2), "wall_ms_per_step": wall / steps * 1e3}


def run_integrator(A, Mg, mask, F, dt, steps, rtol, predictor):
    integ = system.NewmarkIntegrator(A, Mg, mask, dt, tol=0.0, rtol=rtol, max_iter=20000, predictor=predictor)
    integ.start(None, None, F)
    integ.step(F, 1.0)             # warm-up: code objects, the context's buffers
    integ.start(None, None, F)
    integ.events = []
    its = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        it, stt = integ.step(F, 1.0)
        if stt != C.PCG_CONVERGED:
            raise SystemExit(f"step stopped with status {stt} after {it} iterations")
        its.append(it)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = stats(its, integ.events, wall, steps)
    out["keff_solver_layout"] = bool(integ.Keff.solver_layout)
    out["tip_u_max"] = float(integ.u.abs().max())
    integ.close()
    return out


def run_naive(A, Mg, mask, F, dt, steps, rtol, predictor):
    """The same loop from SellMatrix.vals, matvec_multi and pcg alone."""
    dev, N, g = A.device, A.g.n_nodes, A.g
    beta, gamma = 0.25, 0.5
    a0, a2, a3 = 1.0 / (beta * dt * dt), 1.0 / (beta * dt), 1.0 / (2.0 * beta) - 1.0
    Keff = system.SellMatrix(g, 3)
    kv = Keff.vals                      # plain planes [entries / 64, 9, 64]
    kv.copy_(A.plain_values())
    mv = Mg.plain_values().view(-1, 64)
    planes = kv.view(-1, 9, 64)
    for r in (0, 4, 8):
        planes[:, r, :] += a0 * mv
    w = Keff.jacobi(mask)
    free = (w != 0).to(F64)
    mass = lambda x: Mg.matvec_multi(x.view(N, 3)).reshape(-1)
    u = torch.zeros(A.n, dtype=F64, device=dev)
    v, its, ev = u.clone(), [], []
    # a_0 = M^-1 f on the free dofs, component by component
    wm = Mg.jacobi(mask.view(N, 3)[:, 0].contiguous())
    Fn = (F * free).view(N, 3)
    a = torch.zeros((N, 3), dtype=F64, device=dev)
    for r in range(3):
        fr = Fn[:, r].contiguous()
        nrm = float(torch.sqrt(torch.dot(fr, wm * fr)))
        if nrm > 0.0:
            a[:, r] = Mg.pcg(fr, w=wm, tol=1e-12 * nrm, max_iter=10000).x
    a = a.reshape(-1) * free

    def step(u, v, a):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        b = F + mass(a0 * u + a2 * v + a3 * a)
        e[1].record()
        tol = rtol * float(torch.sqrt(torch.dot(b, w * b)))
        res = Keff.pcg(b, x0=u + dt * v if predictor else u, w=w, tol=tol, max_iter=20000)
        if res.status != C.PCG_CONVERGED:
            raise SystemExit(f"step stopped with status {res.status} after {res.iterations} iterations")
        e[2].record()
        un = res.x * free
        an = a0 * (un - u) - a2 * v - a3 * a
        vn = v + dt * ((1.0 - gamma) * a + gamma * an)
        e[3].record()
        return un, vn, an, res.iterations, e

    step(u, v, a)                       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        u, v, a, it, e = step(u, v, a)
        its.append(it)
        ev.append(e)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = stats(its, ev, wall, steps)
    out["tip_u_max"] = float(u.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--f1", type=float, default=None, help="first natural frequency in Hz (default: DESIGN §8k)")
    ap.add_argument("--naive", action="store_true", help="the loop from vals / matvec_multi / pcg alone")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)
    fixed = mesh.face_nodes(coords, 2, 0.0)
    far = mesh.face_nodes(coords, 2, 2.0)
    N = coords.shape[0]
    K = element.compute_c3d4_K_matrix(coords, tets, E, NU, device=dev, dtype=F64)
    V = element.compute_tetrahedral_volumes(coords, tets, device=dev, dtype=F64)
    Ms = (RHO * V / 20.0).view(-1, 1, 1) * (torch.ones((4, 4), dtype=F64, device=dev) + torch.eye(4, dtype=F64, device=dev))
    del V
    g = solver.cached_graph(tets, N)
    A, Mg = system.SellMatrix(g, 3), system.SellMatrix(g, 1)
    A.add_stiffness_and_mass(K, Ms, tets, Mg)
    del K, Ms
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    mask = mask.view(-1)
    F = torch.zeros((N, 3), dtype=F64, device=dev)
    F[far, 0] = 1e6 / far.numel()
    F = F.view(-1).contiguous()
    f1 = a.f1 if a.f1 is not None else F1.get(a.cube_n, F1[55])
    dt = 1.0 / (20.0 * f1)
    run = run_naive if a.naive else run_integrator
    out = {"tool": "bench_transient", "mode": "naive" if a.naive else "integrator", "cube_n": a.cube_n,
           "tets": int(tets.shape[0]), "dofs": A.n, "nnz_blocks": g.nnz, "steps": a.steps, "dt": dt, "f1_hz": f1,
           "rtol": a.rtol, "k_solver_layout": bool(A.solver_layout), "FEM355_SL": os.environ.get("FEM355_SL", "1"),
           "warm": run(A, Mg, mask, F, dt, a.steps, a.rtol, False),
           "predictor": run(A, Mg, mask, F, dt, a.steps, a.rtol, True)}
    assert math.isfinite(out["warm"]["tip_u_max"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
