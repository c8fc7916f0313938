#!/usr/bin/env python3
"""Modal analysis of the stretched, jittered Kuhn cube (prints one JSON line).

`solver.modal_solver` on mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2) with the z = 0 face clamped (Ti-6Al-4V:
E = 113.8e9, nu = 0.342, rho = 4430), k = 6 modes in a block of 8 at tol 1e-6: the iteration count, the seconds of the
solve (a warm-up solve of two iterations comes first), the residuals reached, and the fused K/M product
(fem_spmm_km, one sweep) beside the same two products formed with fem_spmm alone (K in the default passes, the scalar
mass once per component) in the same process, timed with HIP events.

Byte model of one LOBPCG iteration, in [n, m] multi-vector streams of 8 n m bytes: the matrices once
(K blocks with their indices, the scalar mass values) + W gathered; residual 2 reads + 1 write; product 2 writes;
Gram 9 reads; rotation 9 reads + 6 writes: 29 streams + the matrices, against 8 TB/s.

The per-kernel split comes from a run of its own under the profiler, with a fixed iteration count:

    python tools/bench_modal.py --cube-n 119 > profiles/modal_n119.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \\
        python tools/bench_modal.py --cube-n 119 --profile-iters 40
    python tools/bench_modal.py --merge profiles/modal_n119.json <dir>/.../<pid>_kernel_stats.csv   # adds "kernels_us"
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import element, mesh, solver, system  # noqa: E402

E, NU, RHO = 113.8e9, 0.342, 4430.0
PEAK = 8.0e12   # HBM bytes/s (MI355X)
F64 = torch.float64


def events_us(dev, fn, reps):
    """Median microseconds of fn() between two HIP events on the current stream (one warm-up call first)."""
    fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def product_ab(dev, A, Mg, m, reps):
    """The fused product beside fem_spmm alone, on seeded random blocks (microseconds per [n, m] block)."""
    lib = C.lib()
    N, bs, n = A.g.n_nodes, A.bs, A.n
    g = torch.Generator().manual_seed(1)
    X = torch.randn((n, m), dtype=F64, generator=g).to(dev)
    Y, Z = torch.empty_like(X), torch.empty_like(X)
    sp, cols, dcols = C.ptr(A.g.slice_ptr), *A._multi_cols()
    vals, mv = A.plain_values(), Mg.plain_values()
    st = C.stream(dev)

    def fused(nv, Xs, Ys, Zs):
        for x, y, z in zip(Xs, Ys, Zs):
            C.check(lib.fem_spmm_km(N, bs, nv, sp, cols, dcols, C.ptr(vals), C.ptr(mv), C.MASS_SELL, C.ptr(x), C.ptr(y),
                                    C.ptr(z), st), "fem_spmm_km")

    out = {"fused_us": events_us(dev, lambda: fused(m, [X], [Y], [Z]), reps)}
    if m == 8:   # the same block in two passes of 4 columns (pre-split buffers, copies not counted)
        h = [X[:, :4].contiguous(), X[:, 4:].contiguous()]
        hy, hz = [torch.empty_like(v) for v in h], [torch.empty_like(v) for v in h]
        out["fused_two_passes_of_4_us"] = events_us(dev, lambda: fused(4, h, hy, hz), reps)
    # fem_spmm alone: K X in the default passes, and the scalar mass applied to each component's [N, m] block
    comp = [X.view(N, bs, m)[:, r, :].contiguous() for r in range(bs)]
    cz = [torch.empty_like(v) for v in comp]

    def mass_alone():
        for x, z in zip(comp, cz):
            C.check(lib.fem_spmm(N, 1, m, sp, cols, dcols, C.ptr(mv), C.ptr(x), C.ptr(z), st), "fem_spmm")

    out["spmm_K_us"] = events_us(dev, lambda: A.matvec_multi(X), reps)
    out["spmm_M_us"] = events_us(dev, mass_alone, reps)
    out["two_products_us"] = out["spmm_K_us"] + out["spmm_M_us"]
    out["ratio_two_products_over_fused"] = out["two_products_us"] / out["fused_us"]
    return out


def merge_stats(json_path, csv_path):
    """Add the profiler run's per-kernel averages (microseconds per call, calls) to a result line."""
    import csv
    out = json.load(open(json_path))
    rows = [r for r in csv.DictReader(open(csv_path)) if "modal" in r["Name"] or "spmm_km" in r["Name"]]
    out["kernels_us"] = {r["Name"].split("(")[0].replace("void ", ""): {"avg_us": float(r["AverageNs"]) / 1e3,
                                                                        "calls": int(r["Calls"])} for r in rows}
    out["kernels_us_per_iteration"] = sum(v["avg_us"] for v in out["kernels_us"].values())   # one call of each
    print(json.dumps(out))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--merge":   # bench_modal.py --merge result.json kernel_stats.csv
        return merge_stats(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--modes", type=int, default=6)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile-iters", type=int, default=0,
                    help="run only a solve of this many iterations (for a profiler run of its own)")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)
    fixed = mesh.face_nodes(coords, 2, 0.0)
    N = coords.shape[0]
    K = element.compute_c3d4_K_matrix(coords, tets, E, NU, device=dev, dtype=F64)
    V = element.compute_tetrahedral_volumes(coords, tets, device=dev, dtype=F64)
    Ms = (RHO * V / 20.0).view(-1, 1, 1) * (torch.ones((4, 4), dtype=F64, device=dev) + torch.eye(4, dtype=F64, device=dev))
    del V

    def solve(max_iter):
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            return solver.modal_solver(K, Ms, tets, fixed, N, num_modes=a.modes, block=a.block, tol=a.tol,
                                       max_iter=max_iter, device=dev, return_info=True)

    solve(2)   # warm-up: code objects, allocator, the graph cache, the matrix's plain copy
    if a.profile_iters:
        res = solve(a.profile_iters)[3]
        torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "bench_modal", "cube_n": a.cube_n, "profile_iters": res.iterations}))
        return
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    freq, lam, _, res = solve(a.max_iter)
    torch.cuda.synchronize(dev)
    secs = time.perf_counter() - t0

    # the solve's own assembly (graph cached by then), timed apart: seconds - assembly_seconds is the iteration
    g = solver.cached_graph(tets, N)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    A, Mg = system.SellMatrix(g, 3), system.SellMatrix(g, 1)
    A.add_stiffness_and_mass(K, Ms, tets, Mg)
    torch.cuda.synchronize(dev)
    asm = time.perf_counter() - t0
    m = system.modal_block(a.modes, a.block)
    idx = 2 if A.use16 else 4
    mat_bytes = g.nnz * (8 * 9 + idx) + g.nnz * 8
    stream = 8 * A.n * m
    model = mat_bytes + 29 * stream
    its = max(res.iterations, 1)
    out = {"tool": "bench_modal", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "dofs": A.n, "nnz_blocks": g.nnz,
           "modes": a.modes, "block": m, "tol": a.tol, "max_iter": a.max_iter,
           "iterations": res.iterations, "status": res.status, "converged": res.status == C.PCG_CONVERGED,
           "restarts": res.restarts, "seconds": secs, "assembly_seconds": asm,
           "ms_per_iteration": (secs - asm) / its * 1e3,
           "residuals": [float(v) for v in res.residuals], "freq_hz": [float(v) for v in freq],
           "lambda": [float(v) for v in lam],
           "model_bytes_per_iteration": model, "model_ms_at_8TBs": model / PEAK * 1e3,
           "frac_of_8TBs": model / ((secs - asm) / its) / PEAK,
           "product": product_ab(dev, A, Mg, m, a.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
