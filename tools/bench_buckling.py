#!/usr/bin/env python3
"""Linear buckling: the geometric stiffness kernel and the eigen driver (prints one JSON line).

(a) `fem_geo_scalar` (HIP events, median of --reps) on mesh.kuhn_cube(119) (10.1M c3d4) and on the 2M-element
    c3d8 88^3 / c3d6 2 x 70^3 / c3d10 6 x 48^3 set of `bench.py --full`, jittered, with a seeded displacement -- beside
    `fem_iso_mass_scalar` on the same mesh (the same output bytes and tables; c3d4 has no scalar mass kernel: the
    [M, 4, 4] Poisson block of fem_tet4_ke stands in), and beside the route without the kernel (host clock around a
    device synchronisation): compute_element_stress at the points + compute_shape_gradients and compute_Jacobian per
    point + a torch einsum.
(b) a c3d10 cantilever column, mesh.tet10_cube(--column-n) scaled by (1, 1.5, 8), clamped at z = 0 under a unit axial
    compression, E = 1000, nu = 0.3, k = 3 factors at --tol (1e-6, as tools/bench_modal.py): outer iterations, summed inner PCG iterations, the
    seconds per outer iteration split into inner solves / sweeps / the rest (SellMatrix.buckling_lowest's timers), and
    lambda_1 against Euler's pi^2 E I / (4 L^2) (recorded, not asserted).
(c) the same solve with block = 4 and block = 8.

    python tools/bench_buckling.py --skip-column > profiles/buckling_kernel.json
    python tools/bench_buckling.py --skip-kernel > profiles/buckling_column.json

Progress goes to stderr.
"""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import element, mesh, solver  # noqa: E402

E, NU = 1000.0, 0.3
F64 = torch.float64
SETS = (("c3d4", "kuhn_cube", 119), ("c3d8", "hex_box", 88), ("c3d6", "wedge_box", 70), ("c3d10", "tet10_cube", 48))


def note(msg):
    """Progress on stderr (the result line on stdout stays the only line there)."""
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def det3(J):
    return (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1])
            + J[:, 0, 1] * (J[:, 1, 2] * J[:, 2, 0] - J[:, 1, 0] * J[:, 2, 2])
            + J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))


def events_us(fn, reps):
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


def host_us(dev, fn, reps):
    """Median microseconds of fn() by the host clock, a device synchronisation on both sides (one warm-up call)."""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def torch_route(c, el, et, u, dev):
    """Gs without the kernel: what a user could do before it."""
    if et == "c3d4":
        sig, _ = element.compute_c3d4_element_stress(c, el, u, E, NU, device=dev, dtype=F64)
        vol = element.compute_tetrahedral_volumes(c, el, device=dev, dtype=F64)
        g = torch.empty((el.shape[0], 4, 3), dtype=F64, device=dev)
        C.check(C.lib().fem_tet4_geom(C.ptr(c), C.ptr(el), el.shape[0], None, C.ptr(g), None, None, C.stream(dev)),
                "fem_tet4_geom")
        return torch.einsum("m,mai,mik,mbk->mab", vol, g, sig, g)
    p, w = element.mass_integration_points(et)
    ip = torch.cat([p, w[:, None]], dim=1)
    sig, _ = element.compute_element_stress(c, el, u, E, NU, et, integral_point=ip, single=False, device=dev, dtype=F64)
    if et == "c3d10":
        sig = sig.permute(1, 0, 2, 3)                    # the c3d10 stack is point-major
    Gs = torch.zeros((el.shape[0], el.shape[1], el.shape[1]), dtype=F64, device=dev)
    for q in range(p.shape[0]):
        g = element.compute_shape_gradients(c, el, et, p[q], device=dev).to(F64)
        det = det3(element.compute_Jacobian(c, el, et, p[q], device=dev).to(F64)).abs()
        Gs += torch.einsum("m,mai,mik,mbk->mab", det * float(w[q]), g, sig[:, q], g)
    return Gs


def kernel_case(dev, et, gen, n, reps):
    lib = C.lib()
    c, el = getattr(mesh, gen)(n, jitter=0.15, device=dev)
    M, npe = el.shape
    u = 1e-3 * torch.randn(c.shape, dtype=F64, generator=torch.Generator().manual_seed(1)).to(dev)
    dN, w = (t.to(dev).contiguous() for t in element.geometric_integration_points(et))
    Gs = torch.empty((M, npe, npe), dtype=F64, device=dev)
    bad = torch.zeros(M, dtype=torch.uint8, device=dev)
    st = C.stream(dev)

    def geo(with_u=True):
        C.check(lib.fem_geo_scalar(C.ptr(c), C.ptr(el), M, npe, C.ptr(u) if with_u else None, E, NU,
                                   None if with_u else C.ptr(s0), C.ptr(dN), C.ptr(w), dN.shape[0], C.ptr(Gs), C.ptr(bad),
                                   st), "fem_geo_scalar")

    s0 = torch.ones((M, 3, 3), dtype=F64, device=dev)
    out = {"elements": M, "n_ip": int(dN.shape[0]), "out_bytes": 8 * M * npe * npe,
           "geo_us": events_us(geo, reps), "geo_prestress_only_us": events_us(lambda: geo(False), reps)}
    assert not bool(bad.any())
    note(f"{et}: fem_geo_scalar {out['geo_us']:.0f} us for {M} elements")
    if et == "c3d4":
        bad1 = torch.full((1,), M, dtype=torch.int64, device=dev)
        out["mass_analog"] = "fem_tet4_ke KIND_POISSON [M, 4, 4]"
        out["mass_us"] = events_us(lambda: C.check(lib.fem_tet4_ke(C.ptr(c), C.ptr(el), M, 1.0, 0.0, C.KIND_POISSON,
                                                                   C.ptr(Gs), C.ptr(bad1), st), "fem_tet4_ke"), reps)
    else:
        p, _ = element.mass_integration_points(et)
        Nv = torch.tensor([element._N[et](*[float(v) for v in p[q]]) for q in range(p.shape[0])], dtype=F64).to(dev)
        out["mass_analog"] = "fem_iso_mass_scalar"
        out["mass_us"] = events_us(lambda: C.check(lib.fem_iso_mass_scalar(C.ptr(c), C.ptr(el), M, npe, 1.0, C.ptr(Nv),
                                                                           C.ptr(dN), C.ptr(w), dN.shape[0], C.ptr(Gs),
                                                                           st), "fem_iso_mass_scalar"), reps)
    note(f"{et}: {out['mass_analog']} {out['mass_us']:.0f} us")
    geo()
    mine = Gs.clone()
    ref = torch_route(c, el, et, u, dev)
    out["torch_route_max_rel_diff"] = float((ref - mine).abs().max() / mine.abs().max())   # its gradients are fp32
    del ref, mine
    out["torch_route_us"] = host_us(dev, lambda: torch_route(c, el, et, u, dev), max(reps // 2, 2))
    note(f"{et}: torch route {out['torch_route_us']:.0f} us")
    out["ratio_geo_over_mass"] = out["geo_us"] / out["mass_us"]
    out["ratio_torch_over_geo"] = out["torch_route_us"] / out["geo_us"]
    out["geo_store_GBps"] = out["out_bytes"] / out["geo_us"] / 1e3
    return out


def column(dev, n, blocks, tol, max_iter, floor_iters):
    c, el = mesh.tet10_cube(n, device=dev)
    c = c * torch.tensor([1.0, 1.5, 8.0], dtype=F64, device=dev)
    fixed = mesh.face_nodes(c, 2, 0.0)
    top = mesh.face_nodes(c, 2, 8.0)
    F = torch.zeros_like(c)
    F[top, 2] = -1.0 / top.numel()
    euler = math.pi ** 2 * E * (1.5 * 1.0 ** 3 / 12.0) / (4.0 * 8.0 ** 2)
    out = {"column_n": n, "elements": int(el.shape[0]), "dofs": 3 * int(c.shape[0]), "euler_factor": euler, "runs": {}}
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, u, _ = solver.linear_buckling_solver(c, el, "c3d10", F, fixed, E, NU, num_modes=3, max_iter=1,
                                                   device=dev, return_info=True)        # warm-up, and u_ref
    note(f"column: {out['elements']} elements, {out['dofs']} dofs, reference state solved")
    # (block, tol, outer cap): the measured solves, then one at 1e-8 to record where the residuals level off -- the inner
    # PCG's attainable accuracy (eps cond(K)) bounds the outer residual from below
    plan = [(m, tol, max_iter, f"block{m}") for m in blocks]
    if floor_iters:
        plan.append((blocks[0], 1e-8, floor_iters, f"block{blocks[0]}_tol1e-8"))
    for m, tl, cap, name in plan:
        tm = {}
        orig = solver._sys.SellMatrix.buckling_lowest

        def timed(self, *args, **kw):
            return orig(self, *args, timers=tm, history=True, **kw)

        solver._sys.SellMatrix.buckling_lowest = timed
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                lam, _, _, res = solver.linear_buckling_solver(c, el, "c3d10", None, fixed, E, NU, num_modes=3, block=m,
                                                               u_ref=u, tol=tl, max_iter=cap, device=dev,
                                                               return_info=True)
            torch.cuda.synchronize(dev)
            secs = time.perf_counter() - t0
        finally:
            solver._sys.SellMatrix.buckling_lowest = orig
        its = max(res.iterations, 1)
        note(f"column {name}: status {res.status}, {res.iterations} outer, {res.linear_iterations} inner, {secs:.1f} s")
        out["runs"][name] = {
            "tol": tl, "max_iter": cap, "status": res.status, "converged": res.status == C.PCG_CONVERGED,
            "worst_residual_per_iteration": [float(v) for v in res.history.max(dim=1).values], "outer_iterations": res.iterations, "inner_iterations": res.linear_iterations,
            "seconds_total": secs, "seconds_driver": sum(tm.values()),
            "ms_per_outer": {k: v / its * 1e3 for k, v in tm.items()},
            "factors": [float(v) for v in lam], "residuals": [float(v) for v in res.residuals],
            "lambda1_over_euler": float(lam[0]) / euler}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--column-n", type=int, default=26, help="tet10_cube(n): 6 n^3 elements (26: 105,456)")
    ap.add_argument("--blocks", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--floor-iters", type=int, default=40,
                    help="outer iterations of the extra solve at tol 1e-8 that records the residual floor (0: none)")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-column", action="store_true")
    ap.add_argument("--small", action="store_true", help="tiny meshes (a rehearsal of the tool itself)")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"tool": "bench_buckling", "E": E, "nu": NU}
    if not a.skip_kernel:
        out["kernel"] = {}
        for et, gen, n in SETS:
            out["kernel"][et] = kernel_case(dev, et, gen, 4 if a.small else n, a.reps)
            torch.cuda.empty_cache()
        mixed = [out["kernel"][et] for et in ("c3d8", "c3d6", "c3d10")]
        out["kernel"]["mixed_2M"] = {k: sum(v[k] for v in mixed) for k in ("elements", "geo_us", "mass_us",
                                                                           "torch_route_us")}
    if not a.skip_column:
        out["column"] = column(dev, 2 if a.small else a.column_n, a.blocks, a.tol, a.max_iter, a.floor_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
