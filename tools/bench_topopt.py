#!/usr/bin/env python3
"""Topology optimisation of the jittered Kuhn cube: the scaled assembly, the design-loop kernels and the design
iteration (prints one JSON line).

Mesh mesh.kuhn_cube(n, jitter=0.15) (n = 55: 998,250 tets), E = 1, nu = 0.3. Times between HIP events, best of --reps
after a warm-up, same process; bandwidth figures against system.stream_ceiling's copy figure of the same run.

Assembly: reset() + add_tet4 with a seeded per-element scale in [1e-3, 1] beside the unscaled add_tet4, alternating in
one loop, for bs = 3 in the solver layout and in the plain layout (FEM355_SL=0 for those calls) and for bs = 1 in both;
the ratio scaled / unscaled is reported. --unscaled-only stops there and times only the unscaled calls (it then runs on
a tree without the scaled entry points: --root names the tree whose package is imported).

Kernels: fem_tet4_unit_energy (ce, dct, compliance), one forward filter pass with the fused scale, one adjoint pass, and
fem_oc_update's whole 60-step bisection. Streamed bytes per element are computed from the array shapes by
`streamed_bytes` below; gathered node data (coordinates, displacements, node averages) is cached and not counted.

Design iteration (unless --kernels-only): the cantilever case (x = 0 clamped, a unit load in -z on the edge x = 1,
z = 0), volume fraction 0.4, penal 3, s_min = rho_min = 1e-3, one filter pass, move 0.2, linear_rtol 1e-8: the wall
time of one system.TopOpt.step and of --iters of them, with the PCG iterations per design iteration when every solve
starts from the previous displacement and when this tool zeroes TopOpt's x before every step, and the share of the
wall time spent outside fem_pcg_solve.

    python tools/bench_topopt.py --cube-n 55 > profiles/topopt_n55.json
"""
import argparse
import json
import math
import os
import sys
import time


def _root():
    for i, a in enumerate(sys.argv):
        if a == "--root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if a.startswith("--root="):
            return os.path.abspath(a.split("=", 1)[1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, _root())

import torch  # noqa: E402

import fem355  # noqa: E402,F401
from fem355 import _capi as C  # noqa: E402
from fem355 import mesh, system  # noqa: E402

E, NU = 1.0, 0.3
VOLFRAC, PENAL, S_MIN, RHO_MIN, MOVE = 0.4, 3.0, 1e-3, 1e-3, 0.2
F64 = torch.float64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def best_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    return min(timed(fn) for _ in range(reps))


def assembly_times(coords, tets, reps, scaled):
    """reset() + add_tet4 per (bs, layout): unscaled and scaled alternating, best of reps (ms) and the ratio."""
    dev, N, M = coords.device, coords.shape[0], tets.shape[0]
    g = torch.Generator().manual_seed(1)
    s = (1e-3 + (1.0 - 1e-3) * torch.rand(M, dtype=F64, generator=g)).to(dev)
    out = {}
    for bs in (3, 1):
        graph = system.build_graph(tets, N, solver_layout=bs == 1)
        for layout in ("solver", "plain"):
            os.environ["FEM355_SL"] = "1" if layout == "solver" else "0"
            A = system.SellMatrix(graph, bs)
            nu = NU if bs == 3 else 0.0
            plain = lambda: A.reset().add_tet4(coords, tets, E, nu)
            scl = lambda: A.reset().add_tet4(coords, tets, E, nu, scale=s)
            plain()
            if scaled:
                scl()
            torch.cuda.synchronize()
            assert A.solver_layout == (layout == "solver")
            tp, ts = [], []
            for _ in range(reps):
                tp.append(timed(plain))
                if scaled:
                    ts.append(timed(scl))
            key = f"bs{bs}_{layout}"
            out[key + "_unscaled_ms"] = min(tp)
            out[key + "_unscaled_ms_all"] = tp
            if scaled:
                out[key + "_scaled_ms"] = min(ts)
                out[key + "_scaled_over_unscaled"] = min(ts) / min(tp)
            del A
        del graph
    os.environ.pop("FEM355_SL", None)
    torch.cuda.empty_cache()
    return out


def streamed_bytes(N, M, n_bisect):
    """Compulsory HBM bytes per element of each kernel group, from the array shapes (int64 connectivity [M,4], int32
    incidence [4 M] and pointers [N + 1], fp64 element and node vectors)."""
    conn, inc, ptr, ev, nv = 32 * M, 16 * M, 4 * (N + 1), 8 * M, 8 * N
    pass_node = inc + ptr + 2 * ev + nv + nv   # incidence, V and x once each, Vn read, node vector written
    b = {
        "unit_energy": conn + ev + 2 * ev,                       # conn, rho_t; ce, dct
        "filter_forward_scale": pass_node + conn + nv + 2 * ev,  # + conn, node vector read; rho_t and s written
        "filter_adjoint": (inc + ptr + ev + nv + nv) + conn + nv + ev + ev,   # x only; + conn, nodes, V; out
        "oc_update": 2 * ev + n_bisect * 3 * ev + 3 * ev + ev,   # bracket (dc, V); steps (rho, dc, V); final + store
    }
    return {k: v / M for k, v in b.items()}


def kernel_times(to, reps):
    lib, M = to.lib, to.M
    g = torch.Generator().manual_seed(2)
    rnd = lambda n, lo, hi: (lo + (hi - lo) * torch.rand(n, dtype=F64, generator=g)).to(to.device)
    rho, u = rnd(M, RHO_MIN, 1.0), rnd(3 * to.N, -1e-3, 1e-3)
    dc = -rnd(M, 0.0, 1.0) * to.V[:M]
    st = to._stream

    def energy():
        C.check(lib.fem_tet4_unit_energy(C.ptr(to.coords), C.ptr(to.elements), M, C.ptr(u), to.nu, C.ptr(rho), PENAL,
                                         S_MIN, E, C.ptr(to.ce), C.ptr(to.dct), C.ptr(to.work), C.ptr(to.out[0:1]),
                                         C.ptr(to.idx), st))

    def filt(adjoint):
        return lambda: C.check(lib.fem_density_filter(
            C.ptr(to.elements), M, C.ptr(to.g.inc_ptr), C.ptr(to.g.inc), to.N, C.ptr(to.V), C.ptr(to.Vn), C.ptr(rho), 1,
            adjoint, PENAL, S_MIN, C.ptr(to.node_tmp), C.ptr(to.elem_tmp), C.ptr(to.rho_t),
            None if adjoint else C.ptr(to.s), st))

    def oc():
        C.check(lib.fem_oc_update(C.ptr(rho), C.ptr(dc), C.ptr(to.V), None, M, VOLFRAC, MOVE, RHO_MIN,
                                  system.OC_BISECTIONS, C.ptr(to.work), C.ptr(to.rho_new), C.ptr(to.out[1:3]), st))

    per = streamed_bytes(to.N, M, system.OC_BISECTIONS)
    out = {"bytes_per_element": per}
    for name, fn in (("unit_energy", energy), ("filter_forward_scale", filt(0)), ("filter_adjoint", filt(1)),
                     ("oc_update", oc)):
        ms = best_ms(fn, reps)
        out[name + "_ms"] = ms
        out[name + "_gbs"] = per[name] * M / (ms * 1e-3) / 1e9
    out["oc_update_us_per_bisection"] = out["oc_update_ms"] * 1e3 / system.OC_BISECTIONS
    return out


class TimedLib:
    """The library with fem_pcg_solve's wall time (device idle before and after) added up."""

    def __init__(self, lib):
        self._lib, self.pcg_s = lib, 0.0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def fem_pcg_solve(self, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = self._lib.fem_pcg_solve(*args)
        torch.cuda.synchronize()
        self.pcg_s += time.perf_counter() - t0
        return rc


def design_iterations(coords, tets, iters, warm):
    dev, N, M = coords.device, coords.shape[0], tets.shape[0]
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[mesh.face_nodes(coords, 0, 0.0)] = 1
    edge = torch.nonzero((coords[:, 0] > 1.0 - 1e-9) & (coords[:, 2] < 1e-9)).view(-1)
    F = torch.zeros((N, 3), dtype=F64, device=dev)
    F[edge, 2] = -1.0 / edge.numel()
    to = system.TopOpt(coords, tets, F, mask.view(-1), E, NU, VOLFRAC, PENAL, S_MIN, RHO_MIN, 1, MOVE)
    to.lib = TimedLib(to.lib)
    rho = torch.full((M,), VOLFRAC, dtype=F64, device=dev)
    walls, pcg_walls, its, comp, change = [], [], [], [], []
    try:
        for _ in range(iters):
            torch.cuda.synchronize()
            t0, p0 = time.perf_counter(), to.lib.pcg_s
            if not warm:
                to.x.zero_()
            rec = to.step(rho, 1e-8, 100000)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            pcg_walls.append((to.lib.pcg_s - p0) * 1e3)
            its.append(rec["pcg_iterations"])
            if rec["rho_new"] is None:
                break
            rho = rec["rho_new"].clone()
            comp.append(rec["compliance"])
            change.append(rec["change"])
    finally:
        to.close()
    tot, pcg = sum(walls), sum(pcg_walls)
    return {"iterations": len(walls), "wall_ms": walls, "pcg_solve_ms": pcg_walls, "pcg_iterations": its,
            "first_iteration_wall_ms": walls[0], "total_wall_ms": tot, "share_outside_pcg_solve": (tot - pcg) / tot,
            "outside_pcg_solve_ms_per_iteration": (tot - pcg) / len(walls), "compliance": comp, "change": change}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--root", default=None, help="tree whose fem355 package is imported (default: this file's)")
    ap.add_argument("--unscaled-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    N, M = coords.shape[0], tets.shape[0]
    out = {"tool": "bench_topopt", "cube_n": a.cube_n, "tets": M, "dofs": 3 * N, "other_tree": a.root is not None,
           "assembly": assembly_times(coords, tets, a.reps, not a.unscaled_only)}
    if a.unscaled_only:
        print(json.dumps(out))
        return
    mask = torch.zeros(3 * N, dtype=torch.uint8, device=dev)
    to = system.TopOpt(coords, tets, torch.zeros((N, 3), dtype=F64, device=dev), mask, E, NU, VOLFRAC, PENAL, S_MIN,
                       RHO_MIN, 1, MOVE)
    out["kernels"] = kernel_times(to, a.reps)
    to.close()
    del to
    torch.cuda.empty_cache()
    copy = system.stream_ceiling(dev)["copy"]
    out["stream_copy_gbs"] = copy
    for k in ("unit_energy", "filter_forward_scale", "filter_adjoint", "oc_update"):
        out["kernels"][k + "_of_stream_copy"] = out["kernels"][k + "_gbs"] / copy
    if not a.kernels_only:
        out["design_warm_start"] = design_iterations(coords, tets, a.iters, True)
        out["design_zeroed_start"] = design_iterations(coords, tets, a.iters, False)
        for k in ("design_warm_start", "design_zeroed_start"):
            assert all(math.isfinite(c) for c in out[k]["compliance"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
