#!/usr/bin/env python3
"""Generate tests/golden/shell_cells.npz and tests/golden/shell_static.npz by importing the REFERENCE itself.

The reference (sml2004/CUDA-powered-mesh-handling-and-Iterative-solvers @ 2025-04-18) is imported read-only from the
directory named by FEM355_REFERENCE (the one holding `solver/`), with a stub `pyvista` module, every call on
device="cpu", dtype=float64 (SURVEY.md §8(c) recipe). Nothing of the reference is copied: only inputs, outputs and
captured stdout are stored. Exits 0 without writing when the reference is absent.

    FEM355_REFERENCE=/path/to/reference python tools/gen_golden_shell.py

Before writing, the conditions the fixtures must meet are asserted: the reference driver converged, the masked true
residual of its result is below tol, and the restatement tests/shell_ref.py reproduces u to 1e-12 relative.
"""
from __future__ import annotations

import contextlib
import io
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CPU, F64 = "cpu", torch.float64
E, NU = 113.8e9, 0.342
MEMBRANE = [113.8e9, 0.342, 0.3]
BENDING = [113.8e9, 0.342, 1.6]   # its own thickness (a swapped argument shows); stiff enough that the rotation block is not what CG waits for
JITTER = 0.25    # of the cell size, every node of the box but the fin's attachment
MOMENT = 1e3     # bound of the nodal moments on the loaded face's skin nodes
HEX_FACES = ((0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7))
WEDGE_TRIS = ((0, 2, 1), (3, 4, 5))
TET_FACES = ((0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3))


def load_reference():
    ref = os.environ.get("FEM355_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "solver")):
        return None
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pyvista", types.ModuleType("pyvista"))
    sys.path.insert(0, os.path.join(ref, "solver"))
    import solver  # noqa
    return solver


def run_quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, re.sub(r"current iteration:[^\r]*\r", "", buf.getvalue())


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()})
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB  keys={sorted(arrays)}")


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def cells():
    """8 s3 and 8 s4 single elements, own nodes each: jittered, scaled, both orientations, rotated well off the axes;
    s4 elements 2 and 5 are warped (node 2 lifted 0.2 edge lengths out of plane), s4 element 7 is a dart whose reflex
    corner makes detJ negative at one integration point."""
    rng = np.random.default_rng(20250418)
    pts, s3, s4 = [], [], []
    for e in range(8):
        size = 0.05 * 4.0 ** rng.uniform(0, 2)
        p = np.array([[0, 0, 0], [1, 0, 0], [0.3, 0.9, 0]], dtype=float) + rng.uniform(-0.15, 0.15, (3, 3)) * [1, 1, 0]
        ids = [len(pts) + k for k in range(3)]
        if e % 2:
            ids = [ids[0], ids[2], ids[1]]
        pts += list((p * size) @ rotation(rng).T + rng.uniform(-1, 1, 3))
        s3.append(ids)
    for e in range(8):
        size = 0.05 * 4.0 ** rng.uniform(0, 2)
        p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=float)
        p += rng.uniform(-0.15, 0.15, (4, 3)) * [1, 1, 0]
        if e in (2, 5):
            p[2, 2] += 0.2
        if e == 7:
            p[2, :2] = [0.22, 0.2]
        ids = [len(pts) + k for k in range(4)]
        if e % 2:
            ids = [ids[0], ids[3], ids[2], ids[1]]
        pts += list((p * size) @ rotation(rng).T + rng.uniform(-1, 1, 3))
        s4.append(ids)
    return torch.tensor(np.array(pts), dtype=F64), torch.tensor(s3), torch.tensor(s4)


def gen_cells(ref):
    coords, s3, s4 = cells()
    N = coords.shape[0]
    rng = np.random.default_rng(5)
    u = torch.from_numpy(rng.standard_normal((N, 6)))
    kw = dict(device=CPU, dtype=F64)
    out = dict(coords=coords, s3=s3, s4=s4, membrane=np.array(MEMBRANE), bending=np.array(BENDING), u=u,
               D=ref.compute_kirchoff_D_matrix(MEMBRANE, BENDING, **kw))
    # s3
    unit = ref.compute_s3_local_unitvector(coords, s3, device=CPU)
    K = ref.compute_s3_K_matrix(coords, s3, MEMBRANE, BENDING, **kw)
    nmq3 = ref.compute_s3_shell_stress(coords, s3, MEMBRANE, BENDING, u, **kw)
    out.update(s3_unit=unit, s3_local=ref.compute_s3_global_to_local_coordinates(coords, s3, unit, **kw),
               s3_J=ref.compute_s3_jacobian(coords, s3, **kw), s3_grads=ref.compute_s3_shape_gradient(coords, s3, **kw),
               s3_B=ref.compute_s3_B_matrix(coords, s3, **kw), s3_K=K,
               s3_forces=ref.compute_shell_nodal_forces(K, s3, u, unit, **kw), s3_nmq=nmq3)
    # s4: geometry at the K rule's points (the `.item()` values of the float32 points)
    unit = ref.compute_s4_local_unitvector(coords, s4, device=CPU)
    gp, _ = ref.s4_integration_points(device=CPU)
    pts = [(gp[f, 0].item(), gp[f, 1].item()) for f in range(4)]
    K = ref.compute_s4_K_matrix(coords, s4, MEMBRANE, BENDING, **kw)
    Kp = ref.compute_s4_K_matrix(coords, s4, MEMBRANE, BENDING, single=False, **kw)
    nmq4 = ref.compute_s4_shell_stress(coords, s4, MEMBRANE, BENDING, u, **kw)
    out.update(s4_unit=unit, s4_local=ref.compute_s4_global_to_local_coordinates(coords, s4, unit, **kw),
               s4_points=np.array(pts),
               s4_J=torch.stack([ref.compute_s4_jacobian(coords, s4, x, y, **kw) for x, y in pts], -1),
               s4_grads=torch.stack([ref.compute_s4_shape_gradient(coords, s4, x, y, **kw) for x, y in pts], -1),
               s4_B=torch.stack([ref.compute_s4_B_matrix_single(coords, s4, x, y, **kw) for x, y in pts], -1),
               s4_B_sum=ref.compute_s4_B_matrix(coords, s4, **kw), s4_K=K, s4_K_points=Kp,
               s4_forces=ref.compute_shell_nodal_forces(K, s4, u, unit, **kw), s4_nmq=nmq4)
    dets = torch.det(out["s4_J"].permute(0, 3, 1, 2))   # [M, 4]
    print("s4 detJ per point:\n", dets)
    assert bool((dets[7] < 0).any()), "the dart has no negative-detJ point"
    t = MEMBRANE[2]
    for tag, nmq in (("s3", nmq3), ("s4", nmq4)):
        for ztag, z in (("z0", 0.0), ("zt", t / 2)):
            pp = ref.compute_shell_postprocess_values(nmq, t, z=z, **kw)
            out.update({f"{tag}_post_{ztag}_{k}": v for k, v in pp.items()})
    save("shell_cells", **out)


def static_mesh():
    """The conforming box of mixed_static.npz with every node but the fin's attachment moved (surface nodes too), an
    s4 skin on the free hex faces, an s3 skin on the free tet and wedge triangles, and a planar 2 x 2 s4 fin in the
    plane z = 1 attached along the box edge x = 1, z = 1."""
    d = np.load(os.path.join(OUT, "mixed_static.npz"))
    coords = torch.from_numpy(d["coords"]).clone()
    t4, w6, h8 = (torch.from_numpy(d[k]) for k in ("c3d4", "c3d6", "c3d8"))
    n, m = 3, 4
    h = 1.0 / n
    N0 = coords.shape[0]
    idx = torch.arange(m)
    grid = torch.stack(torch.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3)   # lattice (i, j, k) per node

    def on_boundary(face):   # every node of the face on one side of the box
        g = grid[face]
        return bool(((g == 0).all(0) | (g == n).all(0)).any())

    s4 = [el[list(f)].tolist() for el in h8 for f in HEX_FACES if on_boundary(el[list(f)])]
    s3 = [el[list(f)].tolist() for el in w6 for f in WEDGE_TRIS if on_boundary(el[list(f)])]
    s3 += [el[list(f)].tolist() for el in t4 for f in TET_FACES if on_boundary(el[list(f)])]
    attach = [(3 * m + j) * m + 3 for j in range(3)]
    rng = np.random.default_rng(4242)
    move = torch.from_numpy(rng.uniform(-JITTER * h, JITTER * h, (N0, 3)))
    move[attach] = 0.0
    coords = coords + move
    fin_nodes = []
    for layer in (1, 2):
        for j in range(3):
            fin_nodes.append(coords[attach[j]] + torch.tensor([layer * h, 0.0, 0.0], dtype=F64))
    rows = [attach, [N0 + j for j in range(3)], [N0 + 3 + j for j in range(3)]]
    for a in range(2):
        for j in range(2):
            s4.append([rows[a][j], rows[a + 1][j], rows[a + 1][j + 1], rows[a][j + 1]])
    coords = torch.cat([coords, torch.stack(fin_nodes)], 0)
    fin_outer = torch.arange(N0, N0 + 6)
    force = torch.zeros((N0 + 6, 6), dtype=F64)
    force[:N0, :3] = torch.from_numpy(d["force"])[:, :3]
    skin = torch.zeros(N0 + 6, dtype=torch.bool)
    skin[torch.tensor(s3).reshape(-1)] = True
    skin[torch.tensor(s4).reshape(-1)] = True
    loaded = torch.nonzero((grid[:, 2] == n) & skin[:N0]).view(-1)
    force[loaded, 3:] = torch.from_numpy(rng.uniform(-MOMENT, MOMENT, (loaded.numel(), 3)))
    base = torch.from_numpy(d["fixed"])
    return coords, t4, w6, h8, torch.tensor(s3), torch.tensor(s4), force, base, fin_outer


def gen_static(ref):
    import shell_ref as SR
    coords, t4, w6, h8, s3, s4, force, base, fin_outer = static_mesh()
    N = coords.shape[0]
    material = {"E": E, "nu": NU, "membrane": MEMBRANE, "bending": BENDING}
    fixed = torch.cat([base, fin_outer])
    tol = 1e-6
    u, txt = run_quiet(ref.static_structure_solver, coords, force, fixed, c3d4=t4, c3d6=w6, c3d8=h8, s3=s3, s4=s4,
                       material=material, tol=tol, max_iter=20000, device=CPU, dtype=F64)
    m = re.search(r"Converged after (\d+) iterations", txt)
    assert m, "the reference driver did not converge:\n" + txt[-300:]
    n_iter = int(m.group(1))
    kw = dict(device=CPU, dtype=F64)

    def apply(v):
        y = torch.zeros((N, 6), dtype=F64)
        y[:, :3] += ref.compute_nodal_forces(ref.compute_c3d4_K_matrix(coords, t4, E, NU, **kw), t4, v[:, :3], **kw)
        y[:, :3] += ref.compute_nodal_forces(ref.compute_c3d8_K_matrix(coords, h8, E, NU, **kw), h8, v[:, :3], **kw)
        y[:, :3] += ref.compute_nodal_forces(ref.compute_c3d6_K_matrix(coords, w6, E, NU, **kw), w6, v[:, :3], **kw)
        for s, kf, uf in ((s3, ref.compute_s3_K_matrix, ref.compute_s3_local_unitvector),
                          (s4, ref.compute_s4_K_matrix, ref.compute_s4_local_unitvector)):
            y += ref.compute_shell_nodal_forces(kf(coords, s, MEMBRANE, BENDING, **kw), s, v, uf(coords, s, device=CPU),
                                                **kw)
        return y

    r = force - apply(u)
    r[fixed] = 0.0
    res = float(torch.linalg.norm(r))
    assert res < tol, f"masked true residual {res:.3e} >= tol"
    blocks = {"c3d4": t4, "c3d6": w6, "c3d8": h8, "s3": s3, "s4": s4}
    u_re, it_re, status, _ = SR.static_structure(coords, force, fixed, blocks, material, tol=tol, max_iter=20000)
    err = float((u_re - u).abs().max() / u.abs().max())
    assert status == "converged" and err < 1e-12 and abs(it_re - n_iter) <= 2, (status, err, it_re, n_iter)
    p = torch.from_numpy(np.random.default_rng(31).standard_normal((N, 6)))
    save("shell_static", coords=coords, c3d4=t4, c3d6=w6, c3d8=h8, s3=s3, s4=s4, force=force, fixed=fixed,
         fixed_box=base, fin_outer=fin_outer, membrane=np.array(MEMBRANE), bending=np.array(BENDING), E=E, nu=NU,
         tol=tol, u=u, n_iter=n_iter, stdout=np.array(txt), residual=res, p=p, Kp=apply(p))
    print(f"shell_static: {n_iter} iterations, residual {res:.3e}, restatement rel err {err:.2e} ({it_re} it)")


def main():
    ref = load_reference()
    if ref is None:
        print("reference not found (set FEM355_REFERENCE to the directory holding solver/): nothing written")
        return 0
    torch.manual_seed(0)
    gen_cells(ref)
    gen_static(ref)
    return 0


if __name__ == "__main__":
    sys.exit(main())
