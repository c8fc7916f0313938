#!/usr/bin/env python3
"""Large-displacement statics of the stretched, jittered Kuhn cube (prints one JSON line).

Mesh, material and clamp of tools/bench_transient.py: mesh.kuhn_cube(n, jitter=0.15) scaled by (1, 0.7, 2), the z = 0
face clamped, E = 113.8e9, nu = 0.342. A transverse load (--load newtons in x, default 4e8) spread over the far face
bends the block by about a tenth of its long edge; it is applied in --load-steps equal steps and every step is solved
by solver.nonlinear_static_solver's loop on one system.NewtonStatics (tol 1e-8, linear_rtol 1e-6).

Per Newton iteration: the wall milliseconds (device synchronised) of the tangent evaluation (element kernel with the
packed tangent + gather + scalars), the assembly (reset + packed row-gather), the Jacobi weights, the PCG solve and its
iterations, and the line search (trial evaluations without the tangent, and how many).

Kernel times between HIP events, best of --reps, same process and mesh: fem_tet4_ke (elastic, full [M,12,12]) against
fem_tet4_nl writing the full [M,12,12] (same 1152 bytes per element, four more node vectors gathered), its packed form
and its Kt == NULL form.

    python tools/bench_nonlinear.py --cube-n 55 > profiles/nonlinear_n55.json
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


def kernel_times(coords, tets, u, material, reps):
    lib, dev = C.lib(), coords.device
    M = tets.shape[0]
    st = C.stream(dev)
    Kf = torch.empty((M, 12, 12), dtype=F64, device=dev)
    Kp = torch.empty((M, int(lib.fem_ke_sym_stride(4))), dtype=F64, device=dev)
    fe, we = torch.empty((M, 4, 3), dtype=F64, device=dev), torch.empty(M, dtype=F64, device=dev)
    idx = torch.full((2,), M, dtype=torch.int64, device=dev)
    mat = C.MATERIALS[material]

    def ke():
        C.check(lib.fem_tet4_ke(C.ptr(coords), C.ptr(tets), M, E, NU, C.KIND_ELASTIC, C.ptr(Kf), C.ptr(idx[0:1]), st))

    def nl(Kt, packed):
        return lambda: C.check(lib.fem_tet4_nl(C.ptr(coords), C.ptr(tets), M, C.ptr(u), E, NU, mat, packed, C.ptr(Kt),
                                               C.ptr(fe), C.ptr(we), None, None, C.ptr(idx[0:1]), C.ptr(idx[1:2]), st))

    out = {"tet4_ke_full_ms": best_ms(ke, reps), "tet4_nl_full_ms": best_ms(nl(Kf, 0), reps),
           "tet4_nl_packed_ms": best_ms(nl(Kp, 1), reps), "tet4_nl_trial_ms": best_ms(nl(None, 0), reps)}
    out["nl_full_over_ke"] = out["tet4_nl_full_ms"] / out["tet4_ke_full_ms"]
    return out


class Timed:
    """Wraps the NewtonStatics methods of one solve: synchronised wall milliseconds per phase, reset per iteration."""

    def __init__(self, ns):
        self.ns, self.acc = ns, {}
        for name, key in (("tangent", "assembly_ms"), ("jacobi", "jacobi_ms"), ("solve_increment", "pcg_ms")):
            setattr(ns, name, self.wrap(getattr(ns, name), lambda *a, _k=key, **k: _k))
        setattr(ns, "evaluate", self.wrap(ns.evaluate, lambda *a, tangent=False, **k: "element_tangent_ms" if tangent
                                          else "element_trial_ms"))

    def wrap(self, fn, key_of):
        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            key = key_of(*a, **k)
            self.acc[key] = self.acc.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return timed

    def take(self):
        out, self.acc = self.acc, {}
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--material", default="neo_hookean", choices=sorted(C.MATERIALS))
    ap.add_argument("--load", type=float, default=4e8, help="total far-face load in x (N)")
    ap.add_argument("--load-steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the kernel times, at the bending field u_x = 0.05 z^2 (for a counter run)")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    coords = (coords * torch.tensor([1.0, 0.7, 2.0], dtype=F64, device=dev)).contiguous()
    fixed = mesh.face_nodes(coords, 2, 0.0)
    far = mesh.face_nodes(coords, 2, 2.0)
    N = coords.shape[0]
    if a.kernels_only:
        u = torch.zeros((N, 3), dtype=F64, device=dev)
        u[:, 0] = 0.05 * coords[:, 2] ** 2
        print(json.dumps({"tool": "bench_nonlinear", "cube_n": a.cube_n, "tets": int(tets.shape[0]),
                          "material": a.material, "kernels": kernel_times(coords, tets, u, a.material, a.reps)}))
        return
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[fixed] = 1
    F = torch.zeros((N, 3), dtype=F64, device=dev)
    F[far, 0] = a.load / far.numel()
    F = F.view(-1).contiguous()
    ns = system.NewtonStatics(coords, tets, E, NU, a.material, mask.view(-1), graph=solver.cached_graph(tets, N))
    timed, records = Timed(ns), []

    def on_iteration(rec):
        rec.update(timed.take())
        records.append(rec)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()) as log:
        res = solver._newton_statics_loop(ns, F, torch.zeros(3 * N, dtype=F64, device=dev), a.load_steps, 1e-8, 0.0, 25,
                                          1e-6, 10000, on_iteration=on_iteration)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    u = res.u.view(N, 3)
    out = {"tool": "bench_nonlinear", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "dofs": 3 * N,
           "material": a.material, "load_x": a.load, "load_steps": a.load_steps, "status": res.status,
           "converged": bool(res.converged), "newton_iterations": res.newton_iterations,
           "tip_u_max": float(u[far].norm(dim=1).max()), "tip_over_long_edge": float(u[far].norm(dim=1).max()) / 2.0,
           "element_launches": ns.launches, "solve_wall_ms": wall * 1e3, "matrix_solver_layout": bool(ns.A.solver_layout),
           "iterations": records, "kernels": kernel_times(coords, tets, res.u.contiguous(), a.material, a.reps),
           "log_tail": log.getvalue().strip().splitlines()[-3:]}
    ns.close()
    assert math.isfinite(out["tip_u_max"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
