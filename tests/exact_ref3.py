"""Exact-rational references of the third generation of element kernels -- the explicit dynamics' internal force,
strain energy, lumped mass and stable step (csrc/explicit.hip), the topology optimisation's volumes, unit strain
energy, sensitivities, compliance and scaled operator (csrc/topopt.hip, the scaled assembly of csrc/assemble.hip) on
the hard-geometry cases of tests/exact_ref.py, and the s3 / s4 shell kernels (csrc/shell.hip) on a warped patch of its
own -- with the calibration references their tests use
(tests/test_exact_ref_cpu.py, tests/test_gpu_hard_geometry_xd.py). A plain helper module.

The rules are exact_ref's: every fp64 input is the exact rational it is, all arithmetic is `fractions.Fraction`, the
square root of the stable step goes through `exact_ref._sqrt` and ln J of the neo-Hooke material through
`exact_ref2._ln` (2^-128 relative), a result is rounded once, when it becomes a tensor, and everything is memoised per
(case, quantity). The element formulas are exact_ref's and exact_ref2's (`tet4_geom`, `_tet4_K_fr`, `hyper_element`):

  explicit   f_int = sum_e fe, linear fe = K_e u_e (u = exact_ref.tet4_u), svk / neo_hookean fe = V P g_a of
             hyper_element (u = exact_ref2.hyper_u, a unit-mesh field pushed through the case's linear map); the
             magnitude sum of a dof is sum_e |fe|. Energy: sum_e u_e.K_e u_e / 2, sum_e V W. Lumped mass m_i = sum_e
             rho |det| / 24.
             Stable step dt_e = 1 / (c_d sqrt(sum_a |g_a|^2)), c_d^2 = (max(lam, 0) + 2 mu) / rho: with g_a = c_a / det,
             dt_e = sqrt(rho det^2 / ((max(lam, 0) + 2 mu) sum_a |c_a|^2)), one square root.
  topopt     V_e = |det| / 6; ce_e = u_e.K_e(1, nu) u_e = u_e.K_e(E0, nu) u_e / E0; s_e = s_min + (1 - s_min) rho_t^3 (a
             cube: penal = 3), dct_e = -3 (1 - s_min) rho_t^2 E0 ce_e, compliance = sum_e s_e E0 ce_e, and the product
             y = (sum_e s_e K_e) x with its magnitude sum sum_e s_e |K_e| |x_e|.

Calibration (CPU fp64, never the code under test): the restatements' formulas -- hyperelastic_ref.Model through
exact_ref2.hyper_model, explicit_ref's mass and step, topopt_ref.Model's unit energy -- on the edge-difference
gradients and |det| / 6 of exact_ref.tet4_geom_edges_fp64.

Shells (csrc/shell.hip, tests/shell_ref.py, quirks included): the patch generator and its seven cases, the frame
(node 0 the origin, a along edge 0->1, b the part of edge 0->last orthogonal to a, c = a x b), the local coordinates,
J and the gradients J^-1 (dN/dxi, dN/deta) from local x and y only, the s3 matrix detJ / 2 B^T D B, the four s4 terms
detJ B^T D B with the fp32-rounded abscissa as the rational it is, T^T K T in shell_ref.block_order, NMQ = D B u_e with
the local B on the global rows of u (s4: B summed over the points with fp32-rounded factors), and the product
y = sum_e R_e^T K_e R_e u with K_e and the frames as fp64 inputs. The frame's two square roots are taken to 2^-128 and
its unit vectors kept to 2^-256. Calibration: shell_ref as it is.

Cost, measured on one CPU core: c3d4 3 s per case (the three forces and energies 1.7 s, the topopt quantities 1.2 s
on top of exact_ref's memoised K_e); shells 2 s per family and case (whole-patch geometry 0.1 s, the 8 sampled element
matrices 0.2 s for s3 and 0.9 s for s4, NMQ and the whole-patch operator 0.7 s); everything, all cases, 50 s.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction as Fr

import torch

import exact_ref as X
import exact_ref2 as X2
from exact_ref import _dot, _rows, _sqrt, to_tensor
from oracle import ref_cpu as R

F64 = torch.float64
E, NU, RHO = X.E, X.NU, X.RHO
XD_MATERIALS = ("linear", "svk", "neo_hookean")
PENAL, S_MIN = 3.0, 1e-3                   # tests/test_gpu_topopt.py


# ----------------------------------------------------------------------------- explicit dynamics
def xd_u(case, material):
    """The displacement of a case's force: the small random field for the linear material, the finite-strain field of
    exact_ref2 for the other two."""
    return X.tet4_u(case) if material == "linear" else X2.hyper_u(case)


def _xd_elements(c, t, u, material, E_=E, nu_=NU):
    """([fe [4][3]], [we]) per element as Fractions."""
    U = _rows(u)
    fes, wes = [], []
    if material == "linear":
        for K, el in zip(X.tet4_K_fr(c, t, "elastic", E_, nu_), t.tolist()):
            ue = [U[n][k] for n in el for k in range(3)]
            f = [sum(K[i][j] * ue[j] for j in range(12)) for i in range(12)]
            fes.append([f[3 * a:3 * a + 3] for a in range(4)])
            wes.append(sum(ue[i] * f[i] for i in range(12)) / 2)
        return fes, wes
    lam, mu = X2._lam_mu(E_, nu_)
    for (det, C), el in zip(X.tet4_geom(c, t), t.tolist()):
        o = X2.hyper_element(det, C, [U[n] for n in el], lam, mu, material, tangent=False)
        fes.append(o["fe"])
        wes.append(o["we"])
    return fes, wes


def xd_force(c, t, u, material, E_=E, nu_=NU):
    """(f_int [N,3], magnitude sums [N,3], strain energy (one number))."""
    fes, wes = _xd_elements(c, t, u, material, E_, nu_)
    f, mag = X2._scatter(fes, [[[abs(v) for v in r] for r in fe] for fe in fes], t, c.shape[0])
    return f, mag, float(sum(wes))


def xd_mass(c, t, rho=RHO):
    """[N]: sum over the node's elements of rho |det| / 24."""
    rho = Fr(float(rho))
    m = [Fr(0)] * c.shape[0]
    for (det, _), el in zip(X.tet4_geom(c, t), t.tolist()):
        for n in el:
            m[n] += rho * abs(det) / 24
    return to_tensor(m)


def xd_dt(c, t, E_=E, nu_=NU, rho=RHO):
    """[M]: the per-element stable step."""
    lam, mu = X2._lam_mu(E_, nu_)
    cd2 = (max(lam, Fr(0)) + 2 * mu) / Fr(float(rho))
    return to_tensor([_sqrt(det * det / (cd2 * sum(_dot(ca, ca) for ca in C))) for det, C in X.tet4_geom(c, t)])


# ----------------------------------------------------------------------------- topology optimisation
@functools.lru_cache(maxsize=None)
def to_rho_t(M=162, seed=52):
    """Seeded filtered density in [0.2, 1]."""
    return 0.2 + 0.8 * torch.rand(M, dtype=F64, generator=torch.Generator().manual_seed(seed))


def simp_fr(rho_t):
    """s_e = s_min + (1 - s_min) rho_t^3 as Fractions."""
    sm = Fr(S_MIN)
    return [sm + (1 - sm) * r ** 3 for r in _rows(rho_t)]


def to_energy(K_fr, t, u, rho_t, E0=E):
    """(ce [M], dct [M], compliance) from the exact K_e(E0, nu)."""
    U, E0, sm = _rows(u), Fr(float(E0)), Fr(S_MIN)
    ce = []
    for K, el in zip(K_fr, t.tolist()):
        ue = [U[n][k] for n in el for k in range(3)]
        ce.append(sum(ue[i] * sum(K[i][j] * ue[j] for j in range(12)) for i in range(12)) / E0)
    rt, s = _rows(rho_t), simp_fr(rho_t)
    dct = [-3 * (1 - sm) * r * r * E0 * c_ for r, c_ in zip(rt, ce)]
    return to_tensor(ce), to_tensor(dct), float(sum(s_ * E0 * c_ for s_, c_ in zip(s, ce)))


def to_matvec(K_fr, t, x, rho_t):
    """(y, mag) [3N] of (sum_e s_e K_e) x."""
    Ks = [[[s * v for v in row] for row in K] for s, K in zip(simp_fr(rho_t), K_fr)]
    y, _, mag, _ = X.ebe_products(Ks, t, x)
    return y, mag


# ----------------------------------------------------------------------------- per case
@functools.lru_cache(maxsize=None)
def tet4_exact3(case, quantity):
    """Exact reference of one quantity of one c3d4 case (a key of exact_ref.tet4_case): "xd_<material>" (f_int, mag,
    energy), "mass" [N], "dt" [M], "vol" [M], "energy" (ce, dct, compliance) for exact_ref.tet4_u and to_rho_t,
    "matvec" (y, mag) for exact_ref.tet4_x(case, "elastic")."""
    c, t = X.tet4_case(case)
    if quantity.startswith("xd_"):
        mat = quantity[3:]
        return xd_force(c, t, xd_u(case, mat), mat)
    if quantity == "mass":
        return xd_mass(c, t)
    if quantity == "dt":
        return xd_dt(c, t)
    if quantity == "vol":
        return X.tet4_exact(case, "vol")
    if quantity == "energy":
        return to_energy(X._tet4_K_fr(case, "elastic"), t, X.tet4_u(case), to_rho_t(t.shape[0]))
    if quantity == "matvec":
        return to_matvec(X._tet4_K_fr(case, "elastic"), t, X.tet4_x(case, "elastic"), to_rho_t(t.shape[0]))
    raise KeyError(quantity)


def mass_fp64(c, t, V, rho=RHO):
    """explicit_ref.lumped_mass with the given volumes."""
    q = rho * V / 4.0
    return torch.zeros(c.shape[0], dtype=F64).index_add_(0, t.reshape(-1), q.repeat_interleave(4))


def dt_fp64(g, E_=E, nu_=NU, rho=RHO):
    """explicit_ref.element_dt's formula on the given gradients [M,4,3]."""
    import hyperelastic_ref as HR
    lam, mu = HR.lame(E_, nu_)
    cd = math.sqrt((max(lam, 0.0) + 2.0 * mu) / rho)
    return 1.0 / (cd * torch.sqrt((g * g).sum((1, 2))))


def force_fp64(c, t, u, material, V, g):
    """(f_int [N,3], energy) of the restatements on the given volumes and gradients: linear V sigma(eps) g_a, svk /
    neo_hookean through hyperelastic_ref.Model."""
    if material == "linear":
        import hyperelastic_ref as HR
        lam, mu = HR.lame(E, NU)
        H = torch.einsum("mai,maj->mij", u[t], g)
        eps = 0.5 * (H + H.transpose(1, 2))
        sig = lam * eps.diagonal(dim1=1, dim2=2).sum(1).view(-1, 1, 1) * torch.eye(3, dtype=F64) + 2.0 * mu * eps
        fe = V.view(-1, 1, 1) * torch.einsum("mij,maj->mai", sig, g)
        f = torch.zeros(c.shape[0], 3, dtype=F64).index_add_(0, t.reshape(-1), fe.reshape(-1, 3))
        return f, float(0.5 * (V * (sig * eps).sum((1, 2))).sum())
    m = X2.hyper_model(c, t, material)
    m.g, m.V = g, V
    return m.f_int(u), float(m.energies(u).sum())


def topopt_model(c, t, V, g, nu_=NU):
    """topopt_ref.Model on the given volumes and gradients."""
    import topopt_ref as TR
    m = TR.Model.__new__(TR.Model)
    m.coords, m.tets, m.N, m.M = c, t, c.shape[0], t.shape[0]
    m.E, m.nu = 1.0, float(nu_)
    m.g, m.V = g, V
    return m


@functools.lru_cache(maxsize=None)
def tet4_calibration3(case, quantity):
    """The fp64 restatements' values of tet4_exact3's quantities, on edge-difference gradients and |det| / 6."""
    import topopt_ref as TR
    c, t = X.tet4_case(case)
    det, g = X.tet4_geom_edges_fp64(c, t)
    V = det.abs() / 6.0
    if quantity.startswith("xd_"):
        mat = quantity[3:]
        return force_fp64(c, t, xd_u(case, mat), mat, V, g)
    if quantity == "mass":
        return mass_fp64(c, t, V)
    if quantity == "dt":
        return dt_fp64(g)
    if quantity == "vol":
        return V
    rho_t = to_rho_t(t.shape[0])
    if quantity == "energy":
        ce = topopt_model(c, t, V, g).unit_energy(X.tet4_u(case).reshape(-1))
        s = TR.simp(rho_t, PENAL, S_MIN)
        return ce, -PENAL * (1.0 - S_MIN) * rho_t ** (PENAL - 1.0) * E * ce, float((s * E * ce).sum())
    if quantity == "matvec":
        K = X.tet4_K_edges_fp64(c, t, E, NU) * TR.simp(rho_t, PENAL, S_MIN).view(-1, 1, 1)
        return R.nodal_forces(K, t, X.tet4_x(case, "elastic")).reshape(-1)
    raise KeyError(quantity)


def rel_err(a, b):
    """|a - b| / |b| of two numbers."""
    return abs(float(a) - float(b)) / abs(float(b))


def node_err(a, b):
    """max over entries of |a - b| / |b| (positive per-node or per-element values)."""
    a, b = a.detach().to("cpu", F64).reshape(-1), b.reshape(-1)
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def tet4_calibration_err3(case, quantity, part=None):
    """Error of the calibration form against exact in the tests' measure: the force per dof against the magnitude sum
    (part "f") and the energy relative (part "w"); mass, step, volumes, ce (part "ce") and dct (part "dct") per entry
    relative; the compliance relative (part "c"); the product per dof against its magnitude sum."""
    ex, cal = tet4_exact3(case, quantity), tet4_calibration3(case, quantity)
    if quantity.startswith("xd_"):
        return X.dof_err(cal[0], ex[0], ex[1]) if part == "f" else rel_err(cal[1], ex[2])
    if quantity == "energy":
        i = ("ce", "dct", "c").index(part)
        return rel_err(cal[2], ex[2]) if i == 2 else node_err(cal[i], ex[i])
    if quantity == "matvec":
        return X.dof_err(cal, ex[0], ex[1])
    return node_err(cal, ex)


# ----------------------------------------------------------------------------- shells: the patch and its cases
SHELL_CASES = ("plain", "shift1e4", "shift1e6", "scale1e-3", "scale1e3", "squash1e-4", "squash1e-4_rot")
SHELL_TYPES = ("s3", "s4")
SHELL_NX, SHELL_NY, SHELL_H = 9, 8, 0.1
# 8 elements per family: element 0, the last of the first 64-element block and the first of the next, the last
# element, both start orders (even: as generated, odd: one place further round)
SHELL_SAMPLE = {"s4": (0, 1, 31, 62, 63, 64, 65, 71), "s3": (0, 1, 63, 64, 65, 127, 128, 143)}
SHELL_SQUASH = (1.0, 1e-4, 1e-4)


@functools.lru_cache(maxsize=None)
def shell_params():
    """(membrane, bending) = [E, nu, t] twice: the settings of tests/golden/shell_cells.npz."""
    import os

    import numpy as np
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_cells.npz"))
    return torch.from_numpy(g["membrane"]).clone(), torch.from_numpy(g["bending"]).clone()


@functools.lru_cache(maxsize=None)
def shell_unit_patch(seed=61):
    """(coords [90,3], quads [72,4]): a 9 x 8 grid of quads of spacing 0.1, the nodes moved in-plane by up to 0.15 of
    the spacing (seeded), on the shallow doubly curved surface z = 0.05 sin(2 pi x / 0.9) sin(2 pi y / 0.55) taken at
    the moved positions; counter-clockwise node order."""
    nx, ny, h = SHELL_NX, SHELL_NY, SHELL_H
    i, j = torch.meshgrid(torch.arange(nx + 1), torch.arange(ny + 1), indexing="ij")
    xy = torch.stack([i.reshape(-1), j.reshape(-1)], 1).to(F64) * h
    xy = xy + 0.15 * h * (2.0 * torch.rand(xy.shape, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 1.0)
    z = 0.05 * torch.sin(2.0 * math.pi * xy[:, 0] / 0.9) * torch.sin(2.0 * math.pi * xy[:, 1] / 0.55)
    node = lambda a, b: a * (ny + 1) + b
    quads = [[node(a, b), node(a + 1, b), node(a + 1, b + 1), node(a, b + 1)] for a in range(nx) for b in range(ny)]
    return torch.cat([xy, z.view(-1, 1)], 1).contiguous(), torch.tensor(quads, dtype=torch.long)


def shell_linear_map(case):
    """The 3 x 3 matrix of a shell case. The squash compresses the in-plane axis y and, with it, the height z by 1e-4:
    y alone would leave the rise of the surface along the short edges (0.03 against 1e-5) and no sliver."""
    if case == "plain" or case.startswith("shift"):
        return torch.eye(3, dtype=F64)
    if case.startswith("scale"):
        return float(case[5:]) * torch.eye(3, dtype=F64)
    if case.startswith("squash"):
        L = torch.diag(torch.tensor(SHELL_SQUASH, dtype=F64))
        return X._orthogonal() @ L if case.endswith("_rot") else L
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def shell_case(etype, case):
    """(coords, conn): the unit patch through the case's map (shifts along exact_ref.SHIFT_DIR); s3 splits each quad
    into [0, 1, 2] and [0, 2, 3] (144 elements); every second element starts one place further round."""
    c, q = shell_unit_patch()
    if etype == "s3":
        conn = torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)
    else:
        conn = q.clone()
    conn[1::2] = conn[1::2].roll(-1, 1)
    c = c @ shell_linear_map(case).T
    if case.startswith("shift"):
        c = c + float(case[5:]) * torch.tensor(X.SHIFT_DIR, dtype=F64)
    return c.contiguous(), conn.contiguous()


@functools.lru_cache(maxsize=None)
def shell_u(seed=62):
    """Seeded nodal values [90, 6] (translations and rotations) of the stress and operator comparisons."""
    N = (SHELL_NX + 1) * (SHELL_NY + 1)
    return 1e-3 * torch.randn(N, 6, dtype=F64, generator=torch.Generator().manual_seed(seed))


def shell_geom_factors():
    """The point at which J and the gradients of s4 are compared: the K rule's second point (xi, eta) = (g32, g32)."""
    import shell_ref as SR
    return SR.k_factors()[1]


# ----------------------------------------------------------------------------- shells: exact element quantities
def _trim(q):
    return X2._trim(q, 256)


def shell_frame_fr(xe):
    """(unit [3][3] rows a, b, c; local [npe][3]) of one element from its nodes' coordinates: node 0 the origin, a along
    edge 0->1, b the part of edge 0->last orthogonal to a, both normalised, c = a x b. s3 and s4 differ in when a is
    normalised, which the exact value does not see. The two square roots are taken to 2^-128 and the unit vectors
    kept to 2^-256."""
    a, b = X._sub(xe[1], xe[0]), X._sub(xe[-1], xe[0])
    aa = _dot(a, a)
    s = _dot(a, b) / aa
    b = [b[k] - s * a[k] for k in range(3)]
    na, nb = _sqrt(aa), _sqrt(_dot(b, b))
    a = [_trim(v / na) for v in a]
    b = [_trim(v / nb) for v in b]
    unit = [a, b, X._cross(a, b)]
    return unit, [[_dot(X._sub(x, xe[0]), r) for r in unit] for x in xe]


def _param_derivs(npe, f):
    if npe == 3:
        return [Fr(-1), Fr(1), Fr(0)], [Fr(-1), Fr(0), Fr(1)]
    xm, xp, em, ep = (Fr(float(v)) for v in f)
    return [-em / 4, em / 4, ep / 4, -ep / 4], [-xm / 4, -xp / 4, xp / 4, xm / 4]


def shell_point_fr(local, f=None):
    """(J [2][2], det J, gradients [npe][2]) at one point from local x, y only: (dN/dx, dN/dy)_n = J^-1 (dN_n/dxi,
    dN_n/deta) with J = [[dx/dxi, dx/deta], [dy/dxi, dy/deta]] -- J^-1 and not its transpose."""
    npe = len(local)
    dxi, det = _param_derivs(npe, f)
    J = [[sum(dxi[n] * local[n][r] for n in range(npe)), sum(det[n] * local[n][r] for n in range(npe))]
         for r in range(2)]
    dj = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    Ji = [[J[1][1] / dj, -J[0][1] / dj], [-J[1][0] / dj, J[0][0] / dj]]
    return J, dj, [[Ji[r][0] * dxi[n] + Ji[r][1] * det[n] for r in range(2)] for n in range(npe)]


def _shell_cols(g):
    """{local dof: (block, strain column [3])} of a node with gradients (dx, dy): membrane rows on (u, v), bending rows
    kx = -dN/dx thy, ky = dN/dy thx, kxy = dN/dy thx + dN/dx thy; nothing on w and thz."""
    dx, dy = g
    z = Fr(0)
    return {0: (0, [dx, z, dy]), 1: (0, [z, dy, dx]), 3: (1, [z, dy, dy]), 4: (1, [-dx, z, dx])}


def shell_D_fr():
    """((D00, D01, D22) of the membrane block, the same of the bending block), rational from [E, nu, t]."""
    out = []
    for (E_, nu_, t_), bend in zip(shell_params(), (False, True)):
        E_, nu_, t_ = Fr(float(E_)), Fr(float(nu_)), Fr(float(t_))
        a = E_ * t_ ** 3 / (12 * (1 - nu_ ** 2)) if bend else E_ * t_ / (1 - nu_ ** 2)
        out.append((a, nu_ * a, a * (1 - nu_) / 2))
    return out


def _shell_term(grads, weight, D):
    """weight B^T D B [6 npe][6 npe] at one point."""
    npe = len(grads)
    cols = [_shell_cols(g) for g in grads]
    K = [[Fr(0)] * (6 * npe) for _ in range(6 * npe)]
    for a in range(npe):
        for c_, (ha, va) in cols[a].items():
            for b in range(npe):
                for d_, (hb, vb) in cols[b].items():
                    if ha != hb:
                        continue
                    D0, D1, D2 = D[ha]
                    K[6 * a + c_][6 * b + d_] = weight * (D0 * (va[0] * vb[0] + va[1] * vb[1])
                                                          + D1 * (va[0] * vb[1] + va[1] * vb[0]) + D2 * va[2] * vb[2])
    return K


def shell_K_terms_fr(xe):
    """(the points' terms [[d][d]] -- one, detJ / 2 B^T D B, for s3; four, detJ B^T D B at the K rule's points with the
    fp32-rounded abscissa as the rational it is, for s4 --, unit)."""
    import shell_ref as SR
    unit, local = shell_frame_fr(xe)
    D = shell_D_fr()
    if len(xe) == 3:
        _, dj, g = shell_point_fr(local)
        return [_shell_term(g, dj / 2, D)], unit
    terms = []
    for f in SR.k_factors():
        _, dj, g = shell_point_fr(local, f)
        terms.append(_shell_term(g, dj, D))
    return terms, unit


def _sum_terms(terms):
    d = len(terms[0])
    return [[sum(T[i][j] for T in terms) for j in range(d)] for i in range(d)]


def shell_global_fr(K, unit):
    """T^T K T, T = blockdiag(unit) per node and per translation / rotation triple, in shell_ref.block_order."""
    import shell_ref as SR
    d = len(K)
    KT = [[sum(K[i][3 * (j // 3) + k] * unit[k][j % 3] for k in range(3)) for j in range(d)] for i in range(d)]
    G = [[sum(unit[k][i % 3] * KT[3 * (i // 3) + k][j] for k in range(3)) for j in range(d)] for i in range(d)]
    order = SR.block_order(d // 6).tolist()
    return [[G[i][j] for j in order] for i in order]


def shell_stress_fr(xe, ue):
    """NMQ [6] = D B u_e: the local-frame B applied to the element's global rows of u as they are; for s4 B is summed
    over the four points with the factors rounded to fp32 (shell_ref.b_factors)."""
    import shell_ref as SR
    _, local = shell_frame_fr(xe)
    npe = len(xe)
    pts = [None] if npe == 3 else SR.b_factors()
    eps = [[Fr(0)] * 3, [Fr(0)] * 3]
    for f in pts:
        _, _, g = shell_point_fr(local, f)
        for n in range(npe):
            for c_, (h, v) in _shell_cols(g[n]).items():
                for r in range(3):
                    eps[h][r] += v[r] * ue[n][c_]
    out = []
    for (D0, D1, D2), e in zip(shell_D_fr(), eps):
        out += [D0 * e[0] + D1 * e[1], D1 * e[0] + D0 * e[1], D2 * e[2]]
    return out


def shell_apply_fr(K, unit, conn, u):
    """(y [N,6], mag [N,6]) of y = sum_e R_e^T K_e R_e u with the local matrices K [M,d,d] and frames unit [M,3,3]
    taken as the fp64 inputs they are; mag = sum_e |R_e^T| (|K_e| |R_e u|)."""
    N = u.shape[0]
    Kr, Ur, U = _rows(K), _rows(unit), _rows(u)
    y = [[Fr(0)] * 6 for _ in range(N)]
    mg = [[Fr(0)] * 6 for _ in range(N)]
    for Ke, Un, el in zip(Kr, Ur, conn.tolist()):
        npe = len(el)
        ul = [sum(Un[k % 3][j] * U[n][3 * (k // 3) + j] for j in range(3)) for n in el for k in range(6)]
        live = [j for j in range(6 * npe) if ul[j] != 0]
        for a, n in enumerate(el):
            fl = [sum(Ke[6 * a + k][j] * ul[j] for j in live if Ke[6 * a + k][j] != 0) for k in range(6)]
            fm = [sum(abs(Ke[6 * a + k][j] * ul[j]) for j in live if Ke[6 * a + k][j] != 0) for k in range(6)]
            for j in range(6):
                y[n][j] += sum(Un[k][j % 3] * fl[3 * (j // 3) + k] for k in range(3))
                mg[n][j] += sum(abs(Un[k][j % 3]) * fm[3 * (j // 3) + k] for k in range(3))
    return to_tensor(y), to_tensor(mg)


# ----------------------------------------------------------------------------- shells: per case
@functools.lru_cache(maxsize=None)
def shell_apply_inputs(etype, case):
    """(K [M,d,d], unit [M,3,3]) given to the operator: shell_ref's local matrices and frames of the case, fp64 values
    that the kernel and the exact product both take as they are."""
    import shell_ref as SR
    c, conn = shell_case(etype, case)
    return SR.shell_K(c, conn, *shell_params()).contiguous(), SR.frame(c, conn).contiguous()


@functools.lru_cache(maxsize=None)
def shell_exact(etype, case, quantity):
    """Exact reference of one quantity of one shell case. Whole patch: "geom" (unit [M,3,3], local [M,npe,3], J [M,2,2],
    gradients [M,npe,2] at shell_geom_factors), "stress" NMQ [M,6] for shell_u, "apply" (y, mag) for
    shell_apply_inputs and shell_u. On SHELL_SAMPLE: "K" (local K [8,d,d], the points' terms [8,d,d,4] (None for s3),
    global-frame K [8,d,d] in block order)."""
    c, conn = shell_case(etype, case)
    Xr = _rows(c)
    if quantity == "geom":
        f = None if etype == "s3" else shell_geom_factors()
        units, locs, Js, gs = [], [], [], []
        for el in conn.tolist():
            unit, local = shell_frame_fr([Xr[n] for n in el])
            J, _, g = shell_point_fr(local, f)
            units.append(unit), locs.append(local), Js.append(J), gs.append(g)
        return to_tensor(units), to_tensor(locs), to_tensor(Js), to_tensor(gs)
    if quantity == "stress":
        U = _rows(shell_u())
        return to_tensor([shell_stress_fr([Xr[n] for n in el], [U[n] for n in el]) for el in conn.tolist()])
    if quantity == "apply":
        K, unit = shell_apply_inputs(etype, case)
        return shell_apply_fr(K, unit, conn, shell_u())
    if quantity == "K":
        Ks, Ps, Gs = [], [], []
        for e in SHELL_SAMPLE[etype]:
            terms, unit = shell_K_terms_fr([Xr[n] for n in conn[e].tolist()])
            K = _sum_terms(terms)
            Ks.append(K), Gs.append(shell_global_fr(K, unit))
            d = len(K)
            Ps.append([[[T[i][j] for T in terms] for j in range(d)] for i in range(d)])
        return to_tensor(Ks), (to_tensor(Ps) if etype == "s4" else None), to_tensor(Gs)
    raise KeyError(quantity)


@functools.lru_cache(maxsize=None)
def shell_calibration(etype, case, quantity):
    """tests/shell_ref.py's values of shell_exact's quantities, as it is (it differences from node 0)."""
    import shell_ref as SR
    c, conn = shell_case(etype, case)
    mem, ben = shell_params()
    if quantity == "geom":
        unit, loc = SR.geometry(c, conn)
        f = None if etype == "s3" else shell_geom_factors()
        return unit, loc, SR.jacobian(loc, f), SR.gradients(loc, f)
    if quantity == "stress":
        return SR.stress(c, conn, mem, ben, shell_u())
    if quantity == "apply":
        K, unit = shell_apply_inputs(etype, case)
        return SR.nodal_forces(K, conn, shell_u(), unit)
    if quantity == "K":
        s = conn[torch.tensor(SHELL_SAMPLE[etype])]
        order = SR.block_order(conn.shape[1])
        K = SR.shell_K(c, s, mem, ben)
        Kg = SR.global_K(K, SR.frame(c, s))[:, order][:, :, order]
        return K, (SR.s4_K_points(c, s, mem, ben) if etype == "s4" else None), Kg
    raise KeyError(quantity)


SHELL_GEOM_PARTS = ("unit", "local", "J", "grads")
SHELL_K_PARTS = ("K", "points", "global")


def shell_calibration_err(etype, case, quantity, part=None):
    """Error of shell_ref against exact in the tests' measure: per element relative (exact_ref.elem_err) for the
    geometry (part: one of SHELL_GEOM_PARTS), K (one of SHELL_K_PARTS) and NMQ; per dof against the magnitude sum for
    the operator."""
    ex, cal = shell_exact(etype, case, quantity), shell_calibration(etype, case, quantity)
    if quantity == "geom":
        i = SHELL_GEOM_PARTS.index(part)
        return X.elem_err(cal[i], ex[i])
    if quantity == "K":
        i = SHELL_K_PARTS.index(part)
        return X.elem_err(cal[i], ex[i])
    if quantity == "apply":
        return X.dof_err(cal, ex[0], ex[1])
    return X.elem_err(cal, ex)
