#!/usr/bin/env python3
"""Two-level PCG against Jacobi-PCG on the elasticity cube of mesh.cube_elasticity_case (prints one JSON line).

For the n-cube (mesh.kuhn_cube(n), E = 113.8e9, nu = 0.342, z = 0 face fixed, load on the z = 1 face):

  jacobi      Jacobi-PCG on the path solve_tet4 takes today, assembled and matrix-free: iterations to --rtol on
              sqrt(r.z), milliseconds per iteration, the true masked ||b - A x|| / ||b|| reached
  two_level   per candidate of --targets (free nodes per aggregate; the aggregate count is clamped to 512): the setup
              split into aggregation, E and inverse (synchronised wall ms, the space built twice, second build reported),
              then SellMatrix.pcg_two_level tightened until its true residual is at or below the assembled Jacobi
              solve's, so both are solved to the same true relative residual; iterations, ms per iteration, time to
              solution with the setup included
  kernels     the coarse step between HIP events, best of --reps: restriction alone, restriction + dense product +
              prolongation (CoarseSpace.apply), and one matrix product for scale

    python tools/bench_twolevel.py --n 55 > profiles/twolevel_n55.json
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
from fem355 import mesh, system  # noqa: E402

E, NU = 113.8e9, 0.342
F64 = torch.float64


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


def wall_ms(fn, reps=1):
    best, out = math.inf, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=55)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--targets", type=int, nargs="+", default=[500, 1500, 4000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-reps", type=int, default=2)
    a = ap.parse_args()
    C.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.n, device=dev)
    N = coords.shape[0]
    F, fixed = mesh.cube_elasticity_case(coords)
    b = F.to(F64).reshape(-1).contiguous()
    A = system.assemble_tet4_system(coords, tets, "elastic", E, NU)
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    w = A.jacobi(mask.view(-1))
    free = (w != 0).to(F64)
    bn = float((free * b).norm())

    def true_res(x):
        return float((free * (b - A.matvec(x))).norm()) / bn

    out = {"tool": "bench_twolevel", "n": a.n, "tets": int(tets.shape[0]), "nodes": N, "rtol": a.rtol}

    def jacobi_run(op, wj):
        tol = a.rtol * float(torch.sqrt(torch.dot(b, wj * b)))
        op.pcg(b, None, w=wj, mode=C.MODE_PCG, tol=tol, max_iter=20)   # warm-up
        ms, res = wall_ms(lambda: op.pcg(b, None, w=wj, mode=C.MODE_PCG, tol=tol, max_iter=50000, chunk=64),
                          a.solve_reps)
        return {"iterations": int(res.iterations), "status": int(res.status), "solve_ms": ms,
                "ms_per_iteration": ms / max(res.iterations, 1), "true_rel_residual": true_res(res.x),
                "schedule": int(res.schedule)}

    out["jacobi_assembled"] = jacobi_run(A, w)
    target_res = out["jacobi_assembled"]["true_rel_residual"]
    Amf = system.MatFreeOperator(coords, tets, "elastic", E, NU)
    out["jacobi_matfree"] = jacobi_run(Amf, Amf.jacobi(mask.view(-1)))
    del Amf
    nfree = int((w.view(N, 3) != 0).any(1).sum())
    out["free_nodes"] = nfree
    out["two_level"] = []
    seen = {}
    for target in a.targets:
        k = max(1, min(-(-nfree // target), system.COARSE_MAX_AGG))
        if k in seen:
            out["two_level"].append(dict(seen[k], target=target, same_as_target=seen[k]["target"]))
            continue
        A.rigid_coarse_space(coords, w, n_aggregates=k)   # warm-up: allocator, first launches, the plain values
        cs = A.rigid_coarse_space(coords, w, n_aggregates=k)
        setup = sum(cs.times.values())
        rtol, tries = a.rtol, []
        for _ in range(4):   # tighten until the true residual is the assembled Jacobi solve's or better
            tol = rtol * float(torch.sqrt(torch.dot(b, cs.apply(b))))
            ms, res = wall_ms(lambda: A.pcg_two_level(b, coarse=cs, tol=tol, max_iter=50000, chunk=64), a.solve_reps)
            tr = true_res(res.x)
            tries.append({"rtol": rtol, "iterations": int(res.iterations), "true_rel_residual": tr})
            if tr <= target_res or res.status != C.PCG_CONVERGED:
                break
            rtol *= 0.7 * target_res / tr
        r = b.clone()
        rec = {"target": target, "aggregates": cs.n_aggregates, "m": cs.m, "dropped": cs.dropped,
               "records": int(cs.records), "setup_ms": dict(cs.times), "setup_total_ms": setup,
               "iterations": int(res.iterations), "status": int(res.status), "solve_ms": ms,
               "ms_per_iteration": ms / max(res.iterations, 1), "true_rel_residual": tr, "rtol_used": rtol,
               "tries": tries, "time_to_solution_ms": setup + ms,
               "jacobi_time_to_solution_ms": out["jacobi_assembled"]["solve_ms"],
               "kernels_ms": {"restrict": best_ms(lambda: cs.restrict(r), a.reps),
                              "restrict_dense_prolong": best_ms(lambda: cs.apply(r), a.reps),
                              "matvec": best_ms(lambda: A.matvec(r), a.reps)}}
        seen[k] = rec
        out["two_level"].append(rec)
        del cs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
