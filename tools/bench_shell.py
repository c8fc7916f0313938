#!/usr/bin/env python3
"""Shell elements on the MI355X: element kernel, 6-dof assembly and the static solve (prints one JSON line).

Inputs: the n = 55 Kuhn cube (mesh.kuhn_cube(55, jitter=0.15), E = 113.8e9, nu = 0.342, z = 0 face fixed, 1e6 N in z
over the z = 1 face) with and without an s3 skin on its six faces (6 * 55^2 * 2 triangles, shell [E, nu, 0.01] twice),
and a gently waved sheet of --sheet x --sheet s4 (or twice as many s3) elements.

  kernels   fem_shell_ke between HIP events, best of --reps, for the sheet's s4 and s3 elements in the local and the
            global frame, with the bytes of its own model (connectivity + gathered coordinates in, K_e + unit out)
            and that model's rate
  assembly  the 6-dof system of the skinned cube and of the s4 sheet: block numbering + pattern, then the values
            (solid and shell families), synchronised wall milliseconds, best of 3
  solve     static_structure_solver with tol = 0 at two iteration counts; the rate is the difference quotient, so the
            preprocessing both runs share cancels. With and without the skin, alternating, best of 3.
            --skinless-only runs just the solid solve (also on a build without shell elements).

    python tools/bench_shell.py > profiles/shell_n55.json
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
SHELL = [E, NU, 0.01]
F64 = torch.float64
TET_FACES = ((0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3))


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


def wall_ms(fn, reps=3):
    best, out = math.inf, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def cube_skin(n, tets):
    """The tets' faces that lie on a side of the box -> [6 n^2 2, 3] (lattice node (i, j, k) = (id / m / m, ...))."""
    m = n + 1
    f = tets[:, torch.tensor(TET_FACES, device=tets.device)].reshape(-1, 3)
    ijk = torch.stack([f // (m * m), (f // m) % m, f % m], -1)   # [F, 3 nodes, 3 axes]
    side = ((ijk == 0).all(1) | (ijk == n).all(1)).any(1)
    return f[side].contiguous()


def sheet(n, dev):
    """(coords, s4 [n^2, 4], s3 [2 n^2, 3]) of an n x n sheet over [0, 1]^2 with z = 0.02 sin(7 x) cos(5 y)."""
    ax = torch.arange(n + 1, dtype=F64, device=dev) / n
    X, Y = torch.meshgrid(ax, ax, indexing="ij")
    coords = torch.stack([X, Y, 0.02 * torch.sin(7 * X) * torch.cos(5 * Y)], -1).reshape(-1, 3).contiguous()
    c = torch.arange(n, device=dev)
    I, J = (t.reshape(-1) for t in torch.meshgrid(c, c, indexing="ij"))
    a, b, cc, d = I * (n + 1) + J, (I + 1) * (n + 1) + J, (I + 1) * (n + 1) + J + 1, I * (n + 1) + J + 1
    s4 = torch.stack([a, b, cc, d], 1).contiguous()
    s3 = torch.cat([torch.stack([a, b, cc], 1), torch.stack([a, cc, d], 1)], 0).contiguous()
    return coords, s4, s3


def kernel_times(coords, conn, reps):
    from fem355 import shell
    lib, dev = C.lib(), coords.device
    M, npe = conn.shape
    d = 6 * npe
    K = torch.empty((M, d, d), dtype=F64, device=dev)
    unit = torch.empty((M, 3, 3), dtype=F64, device=dev)
    bad = torch.full((1,), M, dtype=torch.int64, device=dev)
    D6 = shell._host_doubles(shell._d_rows(SHELL, SHELL))
    pts = shell._host_doubles(shell._k_points(shell.s4_integration_points(device="cpu")[0])) if npe == 4 else None
    st = C.stream(dev)

    def run(frame):
        return lambda: C.check(lib.fem_shell_ke(C.ptr(coords), C.ptr(conn), M, npe, D6, pts, frame, C.ptr(K),
                                                C.ptr(unit), C.ptr(bad), st), "fem_shell_ke")

    model = M * (8 * npe + 24 * npe + 8 * d * d + 72)
    out = {"elements": M, "model_bytes": model}
    for name, frame in (("local", C.SHELL_LOCAL), ("global", C.SHELL_GLOBAL)):
        ms = best_ms(run(frame), reps)
        out[name + "_ms"] = ms
        out[name + "_model_GBps"] = model / ms * 1e-6
    assert int(bad.item()) == M
    return out


def assembly_times(coords, solids, shells):
    """solids: [(K_e, conn)], shells: [conn]; K_e of the shells formed outside the timed parts."""
    from fem355 import shell
    N = coords.shape[0]
    Kg = [shell.shell_global_K(coords, s, SHELL, SHELL, device=coords.device)[0] for s in shells]

    def pattern():
        dm = system.SixDofMap(N, shells)
        conns = [el for _, el in solids] + [dm.shell_connectivity(s) for s in shells]
        g = system.build_graph(system.pad_connectivity(conns, max(c.shape[1] for c in conns)), dm.n_blocks)
        incs = [system.incidence(c, dm.n_blocks) for c in conns]
        return dm, g, conns, incs

    pattern_ms, (dm, g, conns, incs) = wall_ms(pattern)

    def values():
        A = system.SellMatrix(g, 3)
        for (K, el), inc in zip(solids, incs):
            A.add_element_matrices(K, el, inc=inc)
        for K, conn, inc in zip(Kg, conns[len(solids):], incs[len(solids):]):
            A.add_element_matrices(K, conn, inc=inc)
        return A

    values_ms, A = wall_ms(values)
    return {"nodes": N, "blocks": dm.n_blocks, "block_nnz": int(g.nnz), "pattern_ms": pattern_ms,
            "values_ms": values_ms, "solver_layout": bool(A.solver_layout)}


def solve_rate(coords, tets, skin, force, fixed, k1, k2):
    """CG iterations per second of static_structure_solver from runs of k1 and k2 iterations (tol 0)."""
    kw = dict(c3d4=tets, material={"E": E, "nu": NU, "membrane": SHELL, "bending": SHELL}, tol=0.0,
              device=str(coords.device), return_info=True)
    if skin is not None:
        kw["s3"] = skin
    times, its = {}, {}
    for k in (k1, k2):
        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                _, res = solver.static_structure_solver(coords, force, fixed, max_iter=k, **kw)
            return res
        times[k], res = wall_ms(run, 1)
        its[k] = int(res.iterations)   # k, unless the CG stopped on one of its guards
    return {"iterations_k1": its[k1], "iterations_k2": its[k2], "wall_ms_k1": times[k1], "wall_ms_k2": times[k2],
            "iterations_per_s": (its[k2] - its[k1]) / ((times[k2] - times[k1]) * 1e-3), "schedule": int(res.schedule)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube-n", type=int, default=55)
    ap.add_argument("--sheet", type=int, default=1000, help="s4 elements per side of the sheet")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k1", type=int, default=200)
    ap.add_argument("--k2", type=int, default=4200)
    ap.add_argument("--skinless-only", action="store_true")
    a = ap.parse_args()
    C.lib()   # no device: fail here
    dev = torch.device("cuda", torch.cuda.current_device())
    coords, tets = mesh.kuhn_cube(a.cube_n, jitter=0.15, device=dev)
    N = coords.shape[0]
    F3, fixed = mesh.cube_elasticity_case(coords)
    force = torch.zeros((N, 6), dtype=F64, device=dev)
    force[:, :3] = F3
    out = {"tool": "bench_shell", "cube_n": a.cube_n, "tets": int(tets.shape[0]), "nodes": N}
    solve_rate(coords, tets, None, force, fixed, 10, 20)   # warm-up of every kernel of the solid path
    if a.skinless_only:
        out["solve_skinless"] = max((solve_rate(coords, tets, None, force, fixed, a.k1, a.k2) for _ in range(3)),
                                    key=lambda r: r["iterations_per_s"])
        print(json.dumps(out))
        return
    skin = cube_skin(a.cube_n, tets)
    out["skin_triangles"] = int(skin.shape[0])
    solve_rate(coords, tets, skin, force, fixed, 10, 20)
    runs = {"solve_skinless": [], "solve_skinned": []}
    for _ in range(3):   # alternating
        runs["solve_skinless"].append(solve_rate(coords, tets, None, force, fixed, a.k1, a.k2))
        runs["solve_skinned"].append(solve_rate(coords, tets, skin, force, fixed, a.k1, a.k2))
    for k, v in runs.items():
        out[k] = max(v, key=lambda r: r["iterations_per_s"])
        out[k]["all_iterations_per_s"] = [r["iterations_per_s"] for r in v]
    from fem355 import element
    Ke = element.compute_c3d4_K_matrix(coords, tets, E, NU, device=dev, dtype=F64)
    out["assembly_cube_skinned"] = assembly_times(coords, [(Ke, tets)], [skin])
    del Ke
    sc, s4, s3 = sheet(a.sheet, dev)
    out["kernel_s4"] = kernel_times(sc, s4, a.reps)
    out["kernel_s3"] = kernel_times(sc, s3[: s4.shape[0]].contiguous(), a.reps)
    out["assembly_sheet_s4"] = assembly_times(sc, [], [s4])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
