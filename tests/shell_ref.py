"""Torch-CPU restatement of the shell semantics fem355 reproduces (`solver/shell.py` and the driver
`solver/solver.py:11-135` of the reference), fp64, written from their description: the oracle of the shell
tests wherever no recorded fixture exists, and itself pinned to the fixtures by tests/test_shell_cpu.py.

Conventions: unit [M,3,3] rows a, b, c; local = (x - x0) unit^T; dofs per node (u, v, w, thx, thy, thz); local K has
rows 6 n + dof. Solid families come from oracle/ref_cpu.py.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import ref_cpu as R

F64 = torch.float64
G32 = float(np.float32(1.0 / np.sqrt(3.0)))   # the reference's Gauss abscissa: 1/sqrt(3) rounded to float32
G64 = 1.0 / np.sqrt(3.0)
SIGNS = ((1, -1), (1, 1), (-1, 1), (-1, -1))  # (xi, eta) / g of the four points, in the reference's order


def D_matrix(membrane, bending):
    Em, num, tm = (float(v) for v in membrane)
    Eb, nub, tb = (float(v) for v in bending)
    a = Em * tm / (1 - num ** 2)
    b = Eb * tb ** 3 / (12 * (1 - nub ** 2))
    D = torch.zeros((6, 6), dtype=F64)
    D[:3, :3] = torch.tensor([[a, num * a, 0], [num * a, a, 0], [0, 0, a * (1 - num) / 2]], dtype=F64)
    D[3:, 3:] = torch.tensor([[b, nub * b, 0], [nub * b, b, 0], [0, 0, b * (1 - nub) / 2]], dtype=F64)
    return D


def frame(coords, conn):
    """unit [M,3,3]: s3 projects b on the raw edge and normalises afterwards, s4 normalises a first."""
    x = coords.to(F64)[conn]
    a = x[:, 1] - x[:, 0]
    b = x[:, -1] - x[:, 0]
    if conn.shape[1] == 4:
        a = a / a.norm(dim=1, keepdim=True)
    b = b - ((a * b).sum(1, keepdim=True) / (a * a).sum(1, keepdim=True)) * a
    if conn.shape[1] == 3:
        a = a / a.norm(dim=1, keepdim=True)
    b = b / b.norm(dim=1, keepdim=True)
    return torch.stack([a, b, torch.cross(a, b, dim=1)], dim=1)


def local_coordinates(coords, conn, unit):
    x = coords.to(F64)[conn]
    return torch.einsum("mna,mda->mnd", x - x[:, :1], unit)


def k_factors(g=G32):
    """Per point (1 - xi, 1 + xi, 1 - eta, 1 + eta) in double from the double value of the abscissa (the K rule)."""
    return [[1 - sx * g, 1 + sx * g, 1 - se * g, 1 + se * g] for sx, se in SIGNS]


def b_factors():
    """The same factors rounded to float32: the summed B iterates over the float32 point tensor."""
    g = np.float32(G32)
    one = np.float32(1.0)
    return [[float(one - np.float32(sx) * g), float(one + np.float32(sx) * g), float(one - np.float32(se) * g),
             float(one + np.float32(se) * g)] for sx, se in SIGNS]


def param_derivs(npe, f=None):
    if npe == 3:
        return torch.tensor([-1.0, 1.0, 0.0], dtype=F64), torch.tensor([-1.0, 0.0, 1.0], dtype=F64)
    xm, xp, em, ep = f
    return (0.25 * torch.tensor([-em, em, ep, -ep], dtype=F64), 0.25 * torch.tensor([-xm, -xp, xp, xm], dtype=F64))


def jacobian(local, f=None):
    dxi, det = param_derivs(local.shape[1], f)
    x, y = local[..., 0], local[..., 1]
    return torch.stack([torch.stack([(dxi * x).sum(1), (det * x).sum(1)], -1),
                        torch.stack([(dxi * y).sum(1), (det * y).sum(1)], -1)], 1)


def gradients(local, f=None):
    """[M, npe, 2] = J^-1 (dN/dxi, dN/deta) -- J^-1 itself, not its transpose (the reference's contraction)."""
    dxi, det = param_derivs(local.shape[1], f)
    Ji = torch.inverse(jacobian(local, f))
    return torch.einsum("mab,nb->mna", Ji, torch.stack([dxi, det], -1))


def B_matrix(grads):
    M, npe, _ = grads.shape
    B = torch.zeros((M, 6, 6 * npe), dtype=F64)
    for n in range(npe):
        dx, dy = grads[:, n, 0], grads[:, n, 1]
        B[:, 0, 6 * n] = dx
        B[:, 1, 6 * n + 1] = dy
        B[:, 2, 6 * n] = dy
        B[:, 2, 6 * n + 1] = dx
        B[:, 3, 6 * n + 4] = -dx
        B[:, 4, 6 * n + 3] = dy
        B[:, 5, 6 * n + 3] = dy
        B[:, 5, 6 * n + 4] = dx
    return B


def geometry(coords, conn):
    unit = frame(coords, conn)
    return unit, local_coordinates(coords, conn, unit)


def s3_K(coords, conn, membrane, bending):
    _, loc = geometry(coords, conn)
    B = B_matrix(gradients(loc))
    detJ = torch.det(jacobian(loc))
    return torch.einsum("mai,ab,mbj->mij", B, D_matrix(membrane, bending), B) * (detJ * 0.5).view(-1, 1, 1)


def s4_K_points(coords, conn, membrane, bending, g=G32):
    """[M, 24, 24, 4]: the four points' terms (unit weights, signed detJ)."""
    _, loc = geometry(coords, conn)
    D = D_matrix(membrane, bending)
    out = []
    for f in k_factors(g):
        B = B_matrix(gradients(loc, f))
        out.append(torch.einsum("mai,ab,mbj->mij", B, D, B) * torch.det(jacobian(loc, f)).view(-1, 1, 1))
    return torch.stack(out, -1)


def s4_K(coords, conn, membrane, bending, g=G32):
    return s4_K_points(coords, conn, membrane, bending, g).sum(-1)


def shell_K(coords, conn, membrane, bending):
    return s3_K(coords, conn, membrane, bending) if conn.shape[1] == 3 else s4_K(coords, conn, membrane, bending)


def s4_B_points(coords, conn):
    _, loc = geometry(coords, conn)
    return torch.stack([B_matrix(gradients(loc, f)) for f in b_factors()], -1)


def to_local(conn, u, unit):
    g = u.to(F64)[conn]
    return torch.cat([torch.einsum("mnj,mkj->mnk", g[..., :3], unit), torch.einsum("mnj,mkj->mnk", g[..., 3:], unit)], -1)


def nodal_forces(K, conn, u, unit):
    """[N,6]: gather, rotate into the frames, K_local, rotate back, index_add on 6 node + c."""
    M, npe = conn.shape
    fl = torch.bmm(K, to_local(conn, u, unit).reshape(M, -1, 1)).view(M, npe, 6)
    fg = torch.cat([torch.einsum("mkj,mnk->mnj", unit, fl[..., :3]), torch.einsum("mkj,mnk->mnj", unit, fl[..., 3:])], -1)
    dofs = (conn.unsqueeze(-1) * 6 + torch.arange(6)).reshape(-1)
    return torch.zeros(u.shape[0] * 6, dtype=F64).index_add(0, dofs, fg.reshape(-1)).view(-1, 6)


def stress(coords, conn, membrane, bending, u):
    """[M,6] = D B u_e with the local B applied to the global rows of u; s4: B summed over the points."""
    _, loc = geometry(coords, conn)
    B = B_matrix(gradients(loc)) if conn.shape[1] == 3 else s4_B_points(coords, conn).sum(-1)
    eps = torch.bmm(B, u.to(F64)[conn].reshape(conn.shape[0], -1, 1)).squeeze(2)
    return eps @ D_matrix(membrane, bending).t()


def postprocess(nmq, t, z=0.0):
    s = nmq[:, :3] * (1.0 / t) + nmq[:, 3:6] * (6.0 * z / t ** 2)
    sx, sy, txy = s[:, 0], s[:, 1], s[:, 2]
    half, diff = 0.5 * (sx + sy), 0.5 * (sx - sy)
    rad = torch.sqrt(diff * diff + txy * txy)
    s1, s2 = half + rad, half - rad
    return {"sx": sx, "sy": sy, "txy": txy, "s1": s1, "s2": s2,
            "theta_p": 0.5 * torch.atan2(2.0 * txy, (sx - sy).clamp(min=1e-30)), "tau_max": 0.5 * (s1 - s2),
            "vm_stress": torch.sqrt(s1 * s1 - s1 * s2 + s2 * s2 + 1e-30)}


# ----------------------------------------------------------------------------- 6N-dof dense assembly and the driver
def global_K(K, unit):
    """T^T K T with T = blockdiag(unit) per node and per translation / rotation triple, rows 6 n + dof."""
    M, d, _ = K.shape
    T = torch.zeros((M, d, d), dtype=F64)
    for k in range(d // 3):
        T[:, 3 * k:3 * k + 3, 3 * k:3 * k + 3] = unit
    return T.transpose(1, 2) @ K @ T


def block_order(npe):
    """Position in 6 n + dof order of each row of the assembly's block order [t0 .. t(npe-1), r0 .. r(npe-1)]."""
    return torch.tensor([6 * n + 3 * h + i for h in range(2) for n in range(npe) for i in range(3)])


def dense_K(N, solids, shells):
    """[6N, 6N] from solid families (K_e [M, 3 npe, 3 npe], conn) on columns 0-2 and shell families (local K_e, conn,
    unit) on all six."""
    A = torch.zeros((6 * N, 6 * N), dtype=F64)
    for K, conn in solids:
        dofs = (conn.unsqueeze(-1) * 6 + torch.arange(3)).reshape(conn.shape[0], -1)
        for e in range(conn.shape[0]):
            A[dofs[e].unsqueeze(1), dofs[e].unsqueeze(0)] += K[e]
    for K, conn, unit in shells:
        Kg = global_K(K, unit)
        dofs = (conn.unsqueeze(-1) * 6 + torch.arange(6)).reshape(conn.shape[0], -1)
        for e in range(conn.shape[0]):
            A[dofs[e].unsqueeze(1), dofs[e].unsqueeze(0)] += Kg[e]
    return A


def families(coords, blocks, material):
    """(solid families, shell families) of `blocks` = {"c3d4" | "c3d8" | "c3d6" | "s3" | "s4": conn}."""
    solids, shells = [], []
    for et in ("c3d4", "c3d8", "c3d6"):
        el = blocks.get(et)
        if el is not None:
            E, nu = material["E"], material["nu"]
            solids.append((R.tet4_K(coords, el, E, nu) if et == "c3d4" else R.iso_K(coords, el, et, E, nu), el))
    for et in ("s3", "s4"):
        el = blocks.get(et)
        if el is not None:
            shells.append((shell_K(coords, el, material["membrane"], material["bending"]), el, frame(coords, el)))
    return solids, shells


def operator(N, solids, shells):
    def apply(v):
        out = torch.zeros((N, 6), dtype=F64)
        for K, el in solids:
            out[:, :3] += R.nodal_forces(K, el, v[:, :3].contiguous()).view(N, 3)
        for K, el, unit in shells:
            out += nodal_forces(K, el, v, unit)
        return out
    return apply


def static_structure(coords, force, fixed, blocks, material, u_init=None, tol=1e-10, max_iter=1000, eps=1e-30):
    """The driver's CG on [N,6] with `fixed` nodes zeroed in all six columns -> (u, iterations, status, stdout)."""
    N = coords.shape[0]
    apply = operator(N, *families(coords, blocks, material))
    u = torch.zeros((N, 6), dtype=F64) if u_init is None else u_init.clone().to(F64)
    u[fixed] = 0.0
    r = force.to(F64) - apply(u)
    r[fixed] = 0.0
    p = r.clone()
    rs_old = torch.sum(r * r)
    for i in range(max_iter):
        Ap = apply(p)
        pAp = torch.sum(p * Ap)
        if pAp.abs() < eps or pAp < 0.0:
            return u, i + 1, "breakdown", (f"Terminating early at iteration {i + 1}: p^T K p = {pAp.item():.3e}, "
                                           "which is invalid for SPD systems.")
        alpha = rs_old / (pAp + eps)
        u += alpha * p
        u[fixed] = 0.0
        r -= alpha * Ap
        r[fixed] = 0.0
        rs_new = torch.sum(r * r)
        if torch.sqrt(rs_new) < tol:
            return u, i + 1, "converged", f"Converged after {i + 1} iterations. Residual norm: {rs_new.item():.3e}"
        beta = rs_new / (rs_old + eps)
        p = r + beta * p
        p[fixed] = 0.0
        rs_old = rs_new
    return u, max_iter, "max_iter", "CG did not converge within the maximum number of iterations."
