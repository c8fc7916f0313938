#!/usr/bin/env python3
"""Geometric multigrid PCG against Jacobi-PCG and two-level PCG on the elasticity cube (prints one JSON line).

The coarse mesh is mesh.kuhn_cube(--coarse), refined --levels times (topology.refine_c3d4, RCM numbering); every solver
runs on the finest mesh of that hierarchy (E = 113.8e9, nu = 0.342, z = 0 face fixed, load on the z = 1 face):

  jacobi      Jacobi-PCG on the path solve_tet4 takes today, assembled and matrix-free: iterations to --rtol on
              sqrt(r.z), milliseconds per iteration, the true masked ||b - A x|| / ||b|| reached
  two_level   SellMatrix.pcg_two_level with the default aggregation, tightened until its true residual is at or below
              the assembled Jacobi solve's (the protocol of bench_twolevel.py)
  multigrid   per degree of --degrees: the setup split into refinement (once, shared), level assembly, lmax and coarse
              inverse (synchronised wall ms, the object built twice, second build reported), Multigrid.pcg tightened
              the same way; iterations, ms per iteration, time to solution with the setup included
  sweep       the fused Chebyshev sweep of the finest level between HIP events, best of --reps: its algorithmic bytes
              (Multigrid.algorithmic_bytes_sweep) over that time, against the measured stream ceiling; one plain
              matrix product for scale. The launches run back to back: where the sweep's bytes fit the 256 MB
              memory-side cache (fine n = 56) the rate may be cache-assisted and is no HBM figure

    python tools/bench_multigrid.py --coarse 7 --levels 3 > profiles/multigrid_n56.json
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
from fem355 import mesh, system, topology  # noqa: E402

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
    ap.add_argument("--coarse", type=int, default=7)
    ap.add_argument("--levels", type=int, default=3, help="refinements (the hierarchy has one level more)")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--degrees", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-reps", type=int, default=2)
    ap.add_argument("--skip-matfree", action="store_true")
    ap.add_argument("--skip-two-level", action="store_true")
    a = ap.parse_args()
    C.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    c0, t0 = mesh.kuhn_cube(a.coarse, device=dev)
    topology.refine_c3d4(c0, t0, levels=1)   # warm-up: first launches
    refine_ms, h = wall_ms(lambda: topology.refine_c3d4(c0, t0, levels=a.levels))
    coords, tets = h.fine
    N = coords.shape[0]
    n_fine = a.coarse * 2 ** a.levels
    F, fixed = mesh.cube_elasticity_case(coords)
    b = F.to(F64).reshape(-1).contiguous()
    fixed_mask = torch.zeros(N, dtype=torch.bool, device=dev)
    fixed_mask[fixed] = True
    out = {"tool": "bench_multigrid", "coarse_n": a.coarse, "fine_n": n_fine, "levels": a.levels + 1,
           "tets": int(tets.shape[0]), "nodes": N, "rtol": a.rtol, "refine_ms": refine_ms,
           "level_nodes": [lv.n_nodes for lv in h.levels]}

    mg = system.Multigrid(h, "elastic", E, NU, fixed_mask, degree=a.degrees[0])   # also the warm-up build
    A, w = mg.fine, mg.w[-1]
    out["fine_columns"] = "delta16" if A.use16 else "int32"
    free = (w != 0).to(F64)
    bn = float((free * b).norm())

    def true_res(x):
        return float((free * (b - A.matvec(x))).norm()) / bn

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
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    if not a.skip_matfree:
        Amf = system.MatFreeOperator(coords, tets, "elastic", E, NU)
        out["jacobi_matfree"] = jacobi_run(Amf, Amf.jacobi(mask.view(-1)))
        del Amf

    def tightened(apply, solve):
        """Tighten rtol until the true residual is the assembled Jacobi solve's or better."""
        rtol, tries = a.rtol, []
        for _ in range(4):
            tol = rtol * float(torch.sqrt(torch.dot(b, apply(b))))
            ms, res = wall_ms(lambda: solve(tol), a.solve_reps)
            tr = true_res(res.x)
            tries.append({"rtol": rtol, "iterations": int(res.iterations), "true_rel_residual": tr})
            if tr <= target_res or res.status != C.PCG_CONVERGED:
                break
            rtol *= 0.7 * target_res / tr
        return {"iterations": int(res.iterations), "status": int(res.status), "solve_ms": ms,
                "ms_per_iteration": ms / max(res.iterations, 1), "true_rel_residual": tr, "rtol_used": rtol,
                "tries": tries}

    if not a.skip_two_level:
        A.rigid_coarse_space(coords, w)   # warm-up
        cs = A.rigid_coarse_space(coords, w)
        rec = tightened(cs.apply, lambda tol: A.pcg_two_level(b, coarse=cs, tol=tol, max_iter=50000, chunk=64))
        rec.update(aggregates=cs.n_aggregates, setup_ms=dict(cs.times), setup_total_ms=sum(cs.times.values()))
        rec["time_to_solution_ms"] = rec["setup_total_ms"] + rec["solve_ms"]
        out["two_level"] = rec
        del cs

    out["multigrid"] = []
    for degree in a.degrees:
        mg.close()
        del mg
        torch.cuda.empty_cache()
        mg = system.Multigrid(h, "elastic", E, NU, fixed_mask, degree=degree)
        A, w = mg.fine, mg.w[-1]
        rec = tightened(mg.apply, lambda tol: mg.pcg(b, tol=tol, max_iter=2000, chunk=8))
        setup = dict(mg.times, refine=refine_ms)
        rec.update(degree=degree, setup_ms=setup, setup_total_ms=sum(setup.values()),
                   lmax=[i["lmax"] for i in mg.levels_info()], cycle_ms=best_ms(lambda: mg.apply(b), a.reps))
        rec["time_to_solution_ms"] = rec["setup_total_ms"] + rec["solve_ms"]
        rec["jacobi_time_to_solution_ms"] = out["jacobi_assembled"]["solve_ms"]
        out["multigrid"].append(rec)

    mg.apply(b)
    reps_in = 10
    sweep_ms = best_ms(lambda: [mg.sweep() for _ in range(reps_in)], a.reps) / reps_in
    x = b.clone()
    y = torch.empty_like(b)
    matvec_ms = best_ms(lambda: [A.matvec(x, out=y) for _ in range(reps_in)], a.reps) / reps_in
    nbytes = mg.algorithmic_bytes_sweep()
    ceil = system.stream_ceiling(dev)
    out["sweep"] = {"level": len(h) - 1, "ms": sweep_ms, "algorithmic_bytes": int(nbytes),
                    "GBps": nbytes / sweep_ms / 1e6, "stream_ceiling_GBps": ceil,
                    "fraction_of_copy_ceiling": nbytes / sweep_ms / 1e6 / ceil["copy"],
                    "matvec_ms": matvec_ms, "matvec_bytes": int(A.algorithmic_bytes_spmv()),
                    "matvec_GBps": A.algorithmic_bytes_spmv() / matvec_ms / 1e6}
    mg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
