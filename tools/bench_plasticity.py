#!/usr/bin/env python3
"""Elastoplastic statics of the stretched, jittered Kuhn cube (prints one JSON line).

Mesh, material and clamp of tools/bench_nonlinear.py: mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2), the z = 0
face clamped, E = 113.8e9, nu = 0.342; yield stress 1e-3 E, hardening 0.1 E.

Kernel times between HIP events, best of --reps, same process and mesh, at the graded stretch u_z = a z^2 whose strain
crosses first yield at mid height (about half the elements yield; the share is reported), from a virgin state that is
read from memory like any other: fem_tet4_j2 with the packed tangent, with the full [M,12,12] and with Kt == NULL, every other output written (forces,
potential, trial state, the yield flags), next to fem_tet4_nl (svk) in the same three forms. Bytes per element counted
for the bandwidth figures: the tangent (720 packed / 1152 full), 96 of forces, 8 of potential, 32 of connectivity and,
for fem_tet4_j2, 112 of state (56 read, 56 written) and the flag; the gathered node data (cached) is not counted. The
bandwidth is set against system.stream_ceiling's copy figure from the same run.

Unless --kernels-only: one load-unload solve (load path 0.5, 1.0, 0.0) of a transverse far-face load (--load newtons in
x) by solver.elastoplastic_static_solver's loop on one system.PlasticStatics (tol 1e-8, linear_rtol 1e-6), with the wall
time, the Newton and PCG iterations per step and the share of elements that yielded in each step.

    python tools/bench_plasticity.py --cube-n 55 > profiles/plasticity_n55.json
    python tools/bench_plasticity.py --cube-n 119 --kernels-only > profiles/plasticity_n119.json
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import mesh, solver, system  # noqa: E402

E, NU = 113.8e9, 0.342
SIGMA_Y, HARD = 1e-3 * E, 0.1 * E
F64 = torch.float64
LOAD_PATH = (0.5, 1.0, 0.0)


def best_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = math.inf
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def kernel_times(coords, tets, u, reps):
    lib, dev = C.lib(), coords.device
    M = tets.shape[0]
    st = C.stream(dev)
    e = lambda *s: torch.empty(s, dtype=F64, device=dev)
    Kf, Kp = e(M, 12, 12), e(M, int(lib.fem_ke_sym_stride(4)))
    fe, we, ep, al = e(M, 4, 3), e(M), e(M, 6), e(M)
    ep0, al0 = torch.zeros((M, 6), dtype=F64, device=dev), torch.zeros(M, dtype=F64, device=dev)
    pl = torch.empty(M, dtype=torch.uint8, device=dev)
    idx = torch.full((2,), M, dtype=torch.int64, device=dev)

    def j2(Kt, packed):
        return lambda: C.check(lib.fem_tet4_j2(C.ptr(coords), C.ptr(tets), M, C.ptr(u), E, NU, SIGMA_Y, HARD,
                                               C.ptr(ep0), C.ptr(al0), packed, C.ptr(Kt), C.ptr(fe), C.ptr(we), None,
                                               C.ptr(ep), C.ptr(al), C.ptr(pl), C.ptr(idx[0:1]), st))

    def nl(Kt, packed):
        return lambda: C.check(lib.fem_tet4_nl(C.ptr(coords), C.ptr(tets), M, C.ptr(u), E, NU, C.MAT_SVK, packed,
                                               C.ptr(Kt), C.ptr(fe), C.ptr(we), None, None, C.ptr(idx[0:1]),
                                               C.ptr(idx[1:2]), st))

    out = {}
    for name, fn, state in (("j2", j2, 113), ("nl", nl, 0)):
        for form, Kt, packed, kb in (("packed", Kp, 1, 720), ("full", Kf, 0, 1152), ("trial", None, 0, 0)):
            ms = best_ms(fn(Kt, packed), reps)
            out[f"tet4_{name}_{form}_ms"] = ms
            out[f"tet4_{name}_{form}_gbs"] = (kb + 96 + 8 + 32 + state) * M / (ms * 1e-3) / 1e9
    out["plastic_fraction"] = float(pl.to(F64).mean())
    for form in ("packed", "full", "trial"):
        out[f"j2_over_nl_{form}"] = out[f"tet4_j2_{form}_ms"] / out[f"tet4_nl_{form}_ms"]
    del Kf, Kp
    torch.cuda.empty_cache()
    copy = system.stream_ceiling(dev)["copy"]
    out["stream_copy_gbs"] = copy
    for form in ("packed", "full", "trial"):
        out[f"j2_{form}_of_stream_copy"] = out[f"tet4_j2_{form}_gbs"] / copy
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--load", type=float, default=1.3e7, help="total far-face load in x at load factor 1 (N)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = (coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)).contiguous()
    N = coords.shape[0]
    # uniaxial strain eps_zz = 2 a z reaches first yield (2 mu eps_zz = sigma_y) at z = 1, the middle of the long edge
    ey = SIGMA_Y / (E / (1.0 + NU))
    ug = torch.zeros((N, 3), dtype=F64, device=dev)
    ug[:, 2] = 0.5 * ey * coords[:, 2] ** 2
    out = {"tool": "bench_plasticity", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "dofs": 3 * N,
           "yield_stress": SIGMA_Y, "hardening": HARD, "kernels": kernel_times(coords, tets, ug, a.reps)}
    if a.kernels_only:
        print(json.dumps(out))
        return
    fixed = mesh.face_nodes(coords, 2, 0.0)
    far = mesh.face_nodes(coords, 2, 2.0)
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    F = torch.zeros((N, 3), dtype=F64, device=dev)
    F[far, 0] = a.load / far.numel()
    F = F.view(-1).contiguous()
    ns = system.PlasticStatics(coords, tets, E, NU, SIGMA_Y, HARD, mask.view(-1), graph=solver.cached_graph(tets, N))
    fractions, tips, walls = [], [], []

    def after_step(s, u):
        fractions.append(ns.plastic_fraction())
        ns.commit()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        tips.append(float(u.view(N, 3)[far].norm(dim=1).max()))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()) as log:
        res = solver._newton_statics_loop(ns, F, torch.zeros(3 * N, dtype=F64, device=dev), len(LOAD_PATH), 1e-8, 0.0,
                                          25, 1e-6, 10000, load_factors=LOAD_PATH, after_step=after_step,
                                          potential_round=solver._LS_POT_ROUND, first_tangent=ns.elastic_tangent)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out.update({"load_x": a.load, "load_path": list(LOAD_PATH), "status": res.status, "converged": bool(res.converged),
                "newton_iterations": res.newton_iterations, "pcg_iterations": res.pcg_iterations,
                "step_lengths": res.step_lengths, "plastic_fraction": fractions, "tip_u_max": tips,
                "wall_ms_after_step": walls, "solve_wall_ms": wall * 1e3, "element_launches": ns.launches,
                "equivalent_plastic_strain_max": float(ns.state().equivalent_plastic_strain.max()),
                "log_tail": log.getvalue().strip().splitlines()[-3:]})
    ns.close()
    assert all(math.isfinite(t) for t in tips)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
