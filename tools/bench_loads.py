#!/usr/bin/env python3
"""Distributed loads measurement on the 10M-tet Kuhn cube (n=119).

Each figure is a synchronised wall time of the public call after a warm-up, median of --reps (default 5):
  * gravity            : compute_body_force(uniform g)
  * gravity_thermal    : distributed_loads(gravity + a nodal temperature field), one fem_tet4_loads launch
  * pressure           : compute_surface_load on the whole boundary (face extraction excluded)
  * detour             : the only way to a gravity vector before this module: compute_c3d4_M_matrix followed by
                         compute_nodal_forces on the constant field
plus both forms of fem_tet4_loads (node-centred, and element vectors + gather) for the first two, and the bytes each
path moves: `algorithmic` counts every array once, `issued` what the kernels request (a node-centred thread reads the
connectivity row and the four coordinate rows of every incident tet: 4 visits per tet).

    python tools/bench_loads.py [--n 119] [--reps 5] [--out profiles/loads_n119.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fem355  # noqa: E402,F401
from fem355 import element, loads, mesh, topology  # noqa: E402

F64 = torch.float64
RHO, E, NU, ALPHA = 4.43e-9, 113.8e9, 0.342, 8.6e-6
G = [0.0, 0.0, -9810.0]


def med_wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=119)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loads_n119.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c, t = mesh.kuhn_cube(a.n, device=dev)
    M, N = t.shape[0], c.shape[0]
    Tn = (20.0 + 100.0 * c[:, 2] + 30.0 * c[:, 0] * c[:, 1]).contiguous()
    mat = {"E": E, "nu": NU, "alpha": ALPHA}
    out = {"workload": f"{M:,}-tet c3d4 Kuhn cube n={a.n}, {N:,} nodes", "reps": a.reps,
           "timing": "synchronised wall time of the public call after one warm-up call, median"}

    # bytes: connectivity 32 M, incidence 16 M + 4 (N + 1), coordinates 24 N, output 24 N, nodal T 8 N
    base = 32 * M + 16 * M + 4 * (N + 1) + 24 * N + 24 * N
    node_issued = 16 * M + 4 * (N + 1) + 4 * M * (32 + 96) + 24 * N
    two_issued = M * (32 + 96) + 96 * M + 16 * M + 4 * (N + 1) + 96 * M + 24 * N
    res = {}
    res["gravity"] = {"ms": med_wall_ms(lambda: loads.compute_body_force(c, t, "c3d4", RHO, G, device=dev, dtype=F64),
                                        a.reps), "algorithmic_bytes": base, "issued_bytes": node_issued}
    res["gravity_thermal"] = {
        "ms": med_wall_ms(lambda: loads.distributed_loads(c, c3d4=t, material=mat, gravity=G, rho=RHO, temperature=Tn,
                                                          T_ref=20.0, device=dev), a.reps),
        "algorithmic_bytes": base + 8 * N + 48 * N, "issued_bytes": node_issued + 4 * M * 32 + 48 * N,
        "note": "includes forming the [N,6] array (48 N bytes more)"}
    for form in ("node", "two-pass"):
        issued = node_issued if form == "node" else two_issued
        res[f"kernel_path_gravity_{form}"] = {
            "ms": med_wall_ms(lambda: loads._volume_loads(c, t, "c3d4", body=(RHO, G), device=dev, form=form), a.reps),
            "issued_bytes": issued}
        res[f"kernel_path_gravity_thermal_{form}"] = {
            "ms": med_wall_ms(lambda: loads._volume_loads(c, t, "c3d4", body=(RHO, G),
                                                          thermal=(E, NU, ALPHA, Tn, 20.0), device=dev, form=form),
                              a.reps),
            "issued_bytes": issued + (4 if form == "node" else 1) * M * 32}
    a_n = loads._volume_loads(c, t, "c3d4", body=(RHO, G), thermal=(E, NU, ALPHA, Tn, 20.0), device=dev)
    a_t = loads._volume_loads(c, t, "c3d4", body=(RHO, G), thermal=(E, NU, ALPHA, Tn, 20.0), device=dev,
                              form="two-pass")
    res["forms_max_rel_diff"] = float((a_n - a_t).abs().max() / a_n.abs().max())
    del a_n, a_t

    faces, extra = topology.compute_tetrahedral_surface_faces_with_fourth_node(t, device=dev)
    Fn = faces.shape[0]
    res["pressure"] = {"faces": Fn,
                       "ms": med_wall_ms(lambda: loads.compute_surface_load(c, faces, extra=extra, pressure=1.0e5,
                                                                            device=dev, dtype=F64), a.reps),
                       "algorithmic_bytes": Fn * (24 + 8) + Fn * 72 * 2 + 12 * Fn + 4 * (N + 1) + 24 * N,
                       "note": "face vectors [F,3,3] written and gathered; the incidence of the faces is cached after "
                               "the warm-up"}

    ones = torch.ones((N, 3), dtype=F64, device=dev) * torch.tensor(G, dtype=F64, device=dev)

    def detour():
        Me = element.compute_c3d4_M_matrix(c, t, RHO, device=dev, dtype=F64)
        return element.compute_nodal_forces(Me, t, ones, device=dev, dtype=F64)
    res["detour_mass_matrix_times_field"] = {
        "ms": med_wall_ms(detour, a.reps),
        "algorithmic_bytes": 2 * 1152 * M + 2 * 32 * M + 16 * M + 4 * (N + 1) + 24 * N * 3,
        "note": "compute_c3d4_M_matrix writes [M,12,12] (1152 M bytes), compute_nodal_forces reads it back"}
    f_new = loads.compute_body_force(c, t, "c3d4", RHO, G, device=dev, dtype=F64)
    f_old = detour()
    res["detour_max_rel_diff"] = float((f_new - f_old).abs().max() / f_old.abs().max())
    out["results"] = res
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
