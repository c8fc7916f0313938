#!/usr/bin/env python3
"""Multi-load-case PCG against sequential single solves on one assembled matrix (prints one JSON line).

For every L of --loads: `SellMatrix.pcg_multi` of L load columns at tol = 0 for --iters iterations, --reps times, beside
the baseline of the same run: the untouched `SellMatrix.pcg` at its default schedule for the same iteration count
(one column; sequential solves of L load cases cost L times that). Both are whole calls (set-up, iterations, the
polls) between device synchronisations, divided by the iteration count; "marginal" is the same with a call of
twice the iterations subtracted, which cancels the set-up. Every GPU step runs in this one process.

Byte model per iteration: matrix blocks * (8 bs^2 + index bytes) + L * 12 vector streams + 3 for the
shared w, against 8 TB/s.

    python tools/bench_multi_rhs.py --cube-n 119 --kind elastic > profiles/multi_rhs_n119.json
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
from fem355 import mesh, system  # noqa: E402

E, NU = 113.8e9, 0.342
PEAK = 8.0e12   # HBM bytes/s (MI355X)


def load_columns(coords, kind, L):
    """[n, L]: elasticity -- the z load of mesh.cube_elasticity_case, x shear, torsion and a point load on the z = 1
    face (then scaled repeats); Poisson -- the unit source and graded ones."""
    N = coords.shape[0]
    if kind == "poisson":
        f = mesh.cube_poisson_case(coords)[0]
        base = [f, f * coords[:, 0:1], f * coords[:, 1:2], f * coords[:, 2:3]]
    else:
        top = mesh.face_nodes(coords, 2, 1.0)
        z = mesh.cube_elasticity_case(coords)[0]
        x = torch.zeros_like(z)
        x[top, 0] = 1e6 / top.numel()
        tors = torch.zeros_like(z)
        tors[top, 0] = -(coords[top, 1] - 0.5) * 1e5
        tors[top, 1] = (coords[top, 0] - 0.5) * 1e5
        point = torch.zeros_like(z)
        point[N - 1, 1] = 1e3
        base = [z, x, tors, point]
    cols = [base[j % 4] * (1.0 if j < 4 else 1e-3 * (j // 4 + j % 4)) for j in range(L)]
    return torch.stack([c.reshape(-1) for c in cols], dim=1).contiguous()


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def measure(dev, call, iters, reps):
    """ms per iteration of call(iterations): whole calls of `iters`, and the marginal cost from calls of 2 * iters."""
    call(iters)   # warm-up: code objects, allocator, the matrix's plain copy
    call(2 * iters)
    one, two = [], []
    for _ in range(reps):   # alternate the two lengths
        one.append(timed(dev, lambda: call(iters)))
        two.append(timed(dev, lambda: call(2 * iters)))
    per = [t / iters for t in one]
    marg = [(b - a) / iters for a, b in zip(one, two)]
    return {"ms_per_iter": statistics.median(per), "ms_per_iter_min": min(per), "ms_per_iter_max": max(per),
            "ms_per_iter_marginal": statistics.median(marg), "reps_ms_per_iter": [round(v, 5) for v in per]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--kind", default="elastic", choices=["elastic", "poisson"])
    ap.add_argument("--loads", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-cols", type=int, default=None,
                    help="columns per lock-step pass (default: system.MULTI_MAX of the block size)")
    a = ap.parse_args()
    loads = [int(v) for v in a.loads.split(",")]
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, device=dev)
    A = system.assemble_tet4_system(coords, tets, a.kind, E if a.kind == "elastic" else 1.0,
                                    NU if a.kind == "elastic" else 0.0)
    A.check_singular()
    fixed = mesh.face_nodes(coords, 2, 0.0)
    mask = torch.zeros((coords.shape[0], A.bs), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    w = A.jacobi(mask.view(-1))
    Bmax = load_columns(coords, a.kind, max(loads))
    idx = 2 if A.use16 else 4
    mat_bytes = A.g.nnz * (8 * A.bs * A.bs + idx)
    vec_bytes = 8 * A.n

    b0 = Bmax[:, 0].contiguous()
    base = measure(dev, lambda k: A.pcg(b0, None, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=k), a.iters, a.reps)
    base["schedule"] = A.pcg(b0, None, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=2).schedule
    out = {"tool": "bench_multi_rhs", "kind": a.kind, "cube_n": a.cube_n, "tets": int(tets.shape[0]),
           "dofs": A.n, "nnz_blocks": A.g.nnz, "index_bytes": idx, "iters": a.iters, "reps": a.reps,
           "max_cols": a.max_cols if a.max_cols is not None else system.MULTI_MAX[A.bs],
           "matrix_bytes": mat_bytes, "vector_bytes": vec_bytes, "baseline_single": base, "multi": []}
    for L in loads:
        B = Bmax[:, :L].contiguous()
        r = measure(dev, lambda k: A.pcg_multi(B, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=k, max_cols=a.max_cols),
                    a.iters, a.reps)
        model = mat_bytes + L * 12 * vec_bytes + 3 * vec_bytes
        r.update({
            "loads": L,
            "passes": [list(p) for p in system.multi_passes(L, A.bs, a.max_cols)],
            "model_bytes": model,
            "model_ms_at_8TBs": model / PEAK * 1e3,
            "frac_of_8TBs": model / (r["ms_per_iter"] * 1e-3) / PEAK,
            "ms_per_iter_per_load": r["ms_per_iter"] / L,
            "sequential_ms_per_iter": L * base["ms_per_iter"],
            "ratio_vs_sequential": L * base["ms_per_iter"] / r["ms_per_iter"],
            "ratio_vs_sequential_marginal": L * base["ms_per_iter_marginal"] / r["ms_per_iter_marginal"],
            # the speed condition's comparison: slowest multi repetition against the fastest baseline repetition
            "ratio_worst_case": L * base["ms_per_iter_min"] / r["ms_per_iter_max"],
        })
        out["multi"].append(r)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
