"""Exact-rational references of the element layer, the hard-geometry cases built on them, and the comparison the
hard-geometry tests use (tests/test_exact_ref_cpu.py, tests/test_gpu_hard_geometry.py). A plain helper module.

Every input is an fp64 value taken as the exact rational it is (`Fraction(float(v))`): coordinates, E, nu, rho and the
entries of the rule tables `R.DN[etype](...)`, `R.POINTS[etype]()`, `element._N[etype]`. All arithmetic is
`fractions.Fraction`; a result is rounded once, when it is turned into an fp64 tensor. (von Mises needs a square
root: it is taken to 2^-128 relative before that one rounding.)

c3d4 closed forms, with the P1 gradients g_a = c_a / det (c_1 = e_2 x e_3, c_2 = e_3 x e_1, c_3 = e_1 x e_2,
c_0 = -(c_1 + c_2 + c_3), e_b = x_b - x_0, det = e_1 . c_1) and V = |det| / 6:
    elastic  K_ab = V (lambda g_a g_b^T + mu g_b g_a^T + mu (g_a . g_b) I)
    Poisson  K_ab = kappa V g_a . g_b
    mass     M_ab = rho V (1 + delta_ab) / 20  (x) I3
Isoparametric families (c3d8, c3d6, c3d10) follow the rules the oracle's docstrings state (`oracle/ref_cpu.py`
iso_K / iso_mass / iso_stress): signed detJ in the stiffness, |detJ| in the mass, c3d6 single=True = B at
(1/3, 1/3, 0) times the sum of the three |sub-tet| volumes, single=False of c3d8 / c3d10 = the unweighted per-point
stack.

`tet4_K_edges_fp64` is a torch fp64 restatement of the edge-difference closed form: the calibration reference of the
c3d4 tolerances (CPU code, not the code under test). The isoparametric tolerances are calibrated by the oracle, which
forms J from absolute coordinates like the kernels.

Cost: c3d4 K_e ~1 s per 162 elements, c3d8 ~0.25 s and c3d10 ~0.5 s per element; everything is memoised per
(case, quantity) and the isoparametric samples hold 8 elements.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction as Fr

import torch

from oracle import ref_cpu as R

F64 = torch.float64
E, NU, RHO, KAPPA = 113.8e9, 0.342, 4430.0, 2.5
EPS = 2.2e-16
MARGIN = 8.0


# ----------------------------------------------------------------------------- rational helpers
def _rows(t):
    """Tensor -> nested lists of exact Fractions."""
    def conv(v):
        return [conv(w) for w in v] if isinstance(v, list) else Fr(float(v))
    return conv(t.detach().to("cpu", F64).tolist())


def to_tensor(v):
    """Nested lists of Fractions -> fp64 tensor (the one rounding)."""
    def conv(w):
        return [conv(x) for x in w] if isinstance(w, (list, tuple)) else float(w)
    return torch.tensor(conv(v), dtype=F64)


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _sqrt(q):
    """sqrt of a non-negative Fraction to 2^-128 relative."""
    if q == 0:
        return Fr(0)
    p, d = q.numerator, q.denominator
    return Fr(math.isqrt((p * d) << 256), d << 128)


def _lame(E_, nu_):
    """(cc, a, b) with lambda = cc a, mu = cc b: cc = E / ((1 + nu)(1 - 2 nu)), a = nu, b = (1 - 2 nu) / 2."""
    E_, nu_ = Fr(float(E_)), Fr(float(nu_))
    return E_ / ((1 + nu_) * (1 - 2 * nu_)), nu_, (1 - 2 * nu_) / 2


def _block_K(C, a, b, factor):
    """[3n][3n] of factor * (a c_p c_q^T + b c_q c_p^T + b (c_p . c_q) I) over the node vectors C [n][3]."""
    n = len(C)
    K = [[None] * (3 * n) for _ in range(3 * n)]
    for p in range(n):
        cp = C[p]
        for q in range(n):
            cq = C[q]
            bd = b * _dot(cp, cq)
            for i in range(3):
                for j in range(3):
                    s = a * cp[i] * cq[j] + b * cp[j] * cq[i]
                    if i == j:
                        s += bd
                    K[3 * p + i][3 * q + j] = s * factor
    return K


def _stress(G, ue, cc, a, b):
    """(sigma [3][3], von Mises) from node gradients G [n][3] and node displacements ue [n][3]: sigma = lambda tr(eps)
    I + 2 mu eps, the reference's D with engineering shears (`solver/element.py:282-353`)."""
    H = [[sum(ue[n][i] * G[n][j] for n in range(len(G))) for j in range(3)] for i in range(3)]
    tr = H[0][0] + H[1][1] + H[2][2]
    s = [[cc * (b * (H[i][j] + H[j][i]) + (a * tr if i == j else 0)) for j in range(3)] for i in range(3)]
    vm2 = ((s[0][0] - s[1][1]) ** 2 + (s[1][1] - s[2][2]) ** 2 + (s[2][2] - s[0][0]) ** 2
           + 6 * (s[0][1] ** 2 + s[1][2] ** 2 + s[0][2] ** 2)) / 2
    return s, _sqrt(vm2)


# ----------------------------------------------------------------------------- c3d4
def tet4_geom(c, t):
    """Per element (det, cofactor vectors c_a [4][3]); the gradients are c_a / det."""
    X = _rows(c)
    out = []
    for el in t.tolist():
        p = [X[n] for n in el]
        e1, e2, e3 = _sub(p[1], p[0]), _sub(p[2], p[0]), _sub(p[3], p[0])
        c1, c2, c3 = _cross(e2, e3), _cross(e3, e1), _cross(e1, e2)
        out.append((_dot(e1, c1), [[-(c1[k] + c2[k] + c3[k]) for k in range(3)], c1, c2, c3]))
    return out


def tet4_volumes(c, t):
    return to_tensor([abs(det) / 6 for det, _ in tet4_geom(c, t)])


def tet4_gradients(c, t):
    """[M, 4, 3]"""
    return to_tensor([[[v / det for v in ca] for ca in C] for det, C in tet4_geom(c, t)])


def tet4_B(c, t):
    """[M, 6, 12], Voigt rows xx, yy, zz, xy, yz, xz."""
    return R._voigt_B(tet4_gradients(c, t))


def tet4_K_fr(c, t, kind="elastic", E_=E, nu_=NU):
    """Element matrices as nested Fractions; kind "elastic" (E, nu), "poisson" (kappa = E_), "mass" (rho = E_)."""
    out = []
    if kind == "elastic":
        cc, a, b = _lame(E_, nu_)
    else:
        cc = Fr(float(E_))
    for det, C in tet4_geom(c, t):
        V = abs(det) / 6
        if kind == "elastic":
            out.append(_block_K(C, a, b, cc * V / (det * det)))
        elif kind == "poisson":
            f = cc * V / (det * det)
            out.append([[f * _dot(C[p], C[q]) for q in range(4)] for p in range(4)])
        else:
            out.append([[(cc * V * (2 if p == q else 1) / 20 if i == j else Fr(0)) for q in range(4) for j in range(3)]
                        for p in range(4) for i in range(3)])
    return out


def tet4_stress(c, t, u, E_=E, nu_=NU):
    """(sigma [M, 3, 3], von Mises [M])"""
    cc, a, b = _lame(E_, nu_)
    U = _rows(u)
    sig, vm = [], []
    for (det, C), el in zip(tet4_geom(c, t), t.tolist()):
        s, v = _stress([[x / det for x in ca] for ca in C], [U[n] for n in el], cc, a, b)
        sig.append(s)
        vm.append(v)
    return to_tensor(sig), to_tensor(vm)


def ebe_products(K_fr, t, x):
    """(y, diag, mag, 1 / diag) per dof of the element-by-element sums y = sum_e K_e x_e, diag = sum_e diag(K_e),
    mag = sum_e |K_e| |x_e|, all exact, rounded once. x [N, dpn]."""
    N, dpn = x.shape
    Xr = _rows(x.reshape(-1))
    y, dg, mg = [Fr(0)] * (N * dpn), [Fr(0)] * (N * dpn), [Fr(0)] * (N * dpn)
    for K, el in zip(K_fr, t.tolist()):
        dofs = [n * dpn + k for n in el for k in range(dpn)]
        xe = [Xr[d] for d in dofs]
        for i, di in enumerate(dofs):
            row = K[i]
            y[di] += sum(row[j] * xe[j] for j in range(len(dofs)))
            mg[di] += sum(abs(row[j] * xe[j]) for j in range(len(dofs)))
            dg[di] += row[i]
    return to_tensor(y), to_tensor(dg), to_tensor(mg), to_tensor([1 / v if v else Fr(0) for v in dg])


def tet4_geom_edges_fp64(c, t):
    """(det [M], gradients [M, 4, 3]) in plain fp64 from the edge differences."""
    cof, det = R.tet4_cofactors(c, t)
    return det, cof / det.view(-1, 1, 1)


def tet4_K_edges_fp64(c, t, E_, nu_, kind="elastic"):
    """fp64 restatement of the edge-difference closed form (module docstring): the calibration reference."""
    det, g = tet4_geom_edges_fp64(c, t)
    V = (det.abs() / 6.0).view(-1, 1, 1, 1, 1)
    if kind == "mass":
        m = (torch.ones(4, 4, dtype=F64) + torch.eye(4, dtype=F64)) / 20.0
        return torch.kron(E_ * V.view(-1, 1, 1) * m, torch.eye(3, dtype=F64))
    gg = torch.einsum("mak,mbk->mab", g, g)
    if kind == "poisson":
        return E_ * gg * V.view(-1, 1, 1)
    lam, mu = R._lame(E_, nu_)
    K = lam * torch.einsum("mai,mbj->maibj", g, g) + mu * torch.einsum("maj,mbi->maibj", g, g) \
        + mu * gg[:, :, None, :, None] * torch.eye(3, dtype=F64)[None, None, :, None, :]
    return (K * V).reshape(-1, 12, 12)


# ----------------------------------------------------------------------------- isoparametric families
def _el():
    import fem355  # noqa: F401
    from fem355 import element
    return element


def _dn(etype, pt):
    return _rows(R.DN[etype](*[float(v) for v in pt]))


def _point(xe, dN):
    """(J [3][3], det, C [n][3]) at one point: J[i][k] = sum_j dN[j][i] x[j][k]; the gradients are C / det."""
    n = len(xe)
    J = [[sum(dN[j][i] * xe[j][k] for j in range(n)) for k in range(3)] for i in range(3)]
    adj = [_cross(J[1], J[2]), _cross(J[2], J[0]), _cross(J[0], J[1])]   # column j of det * J^-1
    det = _dot(J[0], adj[0])
    C = [[adj[0][i] * dN[m][0] + adj[1][i] * dN[m][1] + adj[2][i] * dN[m][2] for i in range(3)] for m in range(n)]
    return J, det, C


def iso_point(c, e, etype, pt):
    """(J [M, 3, 3], global shape gradients [M, npe, 3]) at the natural point pt."""
    X, dN = _rows(c), _dn(etype, pt)
    Js, Gs = [], []
    for el in e.tolist():
        J, det, C = _point([X[n] for n in el], dN)
        Js.append(J)
        Gs.append([[v / det for v in cm] for cm in C])
    return to_tensor(Js), to_tensor(Gs)


def _wedge_volume(xe):
    v = Fr(0)
    for (p, q, r, s) in ((0, 1, 2, 3), (1, 2, 4, 3), (2, 4, 5, 3)):
        v += abs(_dot(_cross(_sub(xe[q], xe[p]), _sub(xe[r], xe[p])), _sub(xe[s], xe[p]))) / 6
    return v


def iso_K(c, e, etype, E_=E, nu_=NU):
    """(K single=True [M, d, d], K single=False) by the oracle's rules: c3d8 / c3d10 single=False is the unweighted
    per-point stack [n_ip, M, d, d]; c3d6 single=True is B at (1/3, 1/3, 0) times the wedge volume and single=False
    the weighted 6-point sum."""
    cc, a, b = _lame(E_, nu_)
    X = _rows(c)
    pts, wts = R.POINTS[etype]()
    dNs = [_dn(etype, p) for p in pts]
    W = _rows(wts)
    dNc = _rows(R.wedge6_dN(1.0 / 3.0, 1.0 / 3.0, 0.0)) if etype == "c3d6" else None
    single, multi = [], []
    for el in e.tolist():
        xe = [X[n] for n in el]
        per = []
        for dN in dNs:
            _, det, C = _point(xe, dN)
            per.append(_block_K(C, a, b, cc / det))          # detJ B^T D B
        d = len(per[0])
        wsum = [[sum(W[q] * per[q][i][j] for q in range(len(per))) for j in range(d)] for i in range(d)]
        if etype == "c3d6":
            _, det, C = _point(xe, dNc)
            single.append(_block_K(C, a, b, cc * _wedge_volume(xe) / (det * det)))
            multi.append(wsum)
        else:
            single.append(wsum)
            multi.append(per)
    Ks = to_tensor(single)
    Km = to_tensor(multi)
    return Ks, (Km if etype == "c3d6" else Km.transpose(0, 1).contiguous())


def iso_mass(c, e, etype, rho=RHO):
    """rho sum_q w_q |detJ_q| N N^T (x) I3 with element.mass_integration_points and element._N -> [M, 3 npe, 3 npe]."""
    el_ = _el()
    X = _rows(c)
    pts, wts = el_.mass_integration_points(etype)
    dNs = [_dn(etype, p) for p in pts]
    Ns = [_rows(torch.tensor(el_._N[etype](*[float(v) for v in p]), dtype=F64)) for p in pts]
    W, rho = _rows(wts), Fr(float(rho))
    out = []
    for el in e.tolist():
        xe = [X[n] for n in el]
        n = len(xe)
        coef = [rho * W[q] * abs(_point(xe, dNs[q])[1]) for q in range(len(dNs))]
        m = [[sum(coef[q] * Ns[q][p] * Ns[q][r] for q in range(len(dNs))) for r in range(n)] for p in range(n)]
        out.append([[(m[p][r] if i == j else Fr(0)) for r in range(n) for j in range(3)]
                    for p in range(n) for i in range(3)])
    return to_tensor(out)


def iso_stress(c, e, u, etype, E_=E, nu_=NU):
    """single=True: sum_q w_q (sigma_q, von Mises_q) -> ([M, 3, 3], [M])."""
    cc, a, b = _lame(E_, nu_)
    X, U = _rows(c), _rows(u)
    pts, wts = R.POINTS[etype]()
    dNs, W = [_dn(etype, p) for p in pts], _rows(wts)
    sig, vm = [], []
    for el in e.tolist():
        xe, ue = [X[n] for n in el], [U[n] for n in el]
        S, V = [[Fr(0)] * 3 for _ in range(3)], Fr(0)
        for q, dN in enumerate(dNs):
            _, det, C = _point(xe, dN)
            s, v = _stress([[x / det for x in cm] for cm in C], ue, cc, a, b)
            S = [[S[i][j] + W[q] * s[i][j] for j in range(3)] for i in range(3)]
            V += W[q] * v
        sig.append(S)
        vm.append(V)
    return to_tensor(sig), to_tensor(vm)


# ----------------------------------------------------------------------------- comparison
def elem_err(a, b):
    """Per-element relative error max|a - b| / max|b| over the element's entries (dim 0 = element), max over
    elements."""
    a = a.detach().to("cpu", F64).reshape(a.shape[0], -1)
    b = b.detach().to("cpu", F64).reshape(b.shape[0], -1)
    return float(((a - b).abs().max(1).values / b.abs().max(1).values.clamp_min(1e-300)).max())


def dof_err(y, y_exact, mag):
    """Per-dof error of an assembled product relative to the magnitude sum: max_dof |y - y_exact| / mag_dof."""
    y = y.detach().to("cpu", F64).reshape(-1)
    return float(((y - y_exact.reshape(-1)).abs() / mag.reshape(-1).clamp_min(1e-300)).max())


def tolerance(calibration_err):
    """Margin 8 over the calibration reference's own error (floored at one fp64 epsilon): another summation order,
    FMA contraction and a 1-ulp reciprocal."""
    return MARGIN * max(calibration_err, EPS)


def check(name, err, calibration_err):
    """The assertion of every measured comparison; prints the figures first (pytest -s shows them)."""
    tol = tolerance(calibration_err)
    print(f"HARDGEOM {name}: err {err:.2e} calib {calibration_err:.2e} ratio {err / max(calibration_err, EPS):.2f} "
          f"tol {tol:.2e}")
    assert err <= tol, f"{name}: error {err:.3e} > {tol:.3e} (8 x calibration error {calibration_err:.3e})"
    return err


# ----------------------------------------------------------------------------- cases
TET4_CASES = ("flipped", "shift1e4", "shift1e6", "scale1e-3", "scale1e3", "squash1e-4", "squash1e-4_rot")
ISO_CASES = ("plain", "shift1e3", "shift1e6", "squash1e-4")
ISO_TYPES = ("c3d8", "c3d6", "c3d10")
SHIFT_DIR = (1.0, -0.7, 0.3)
_ISO_REORDER = {"c3d8": [4, 5, 6, 7, 0, 1, 2, 3], "c3d6": [3, 4, 5, 0, 1, 2]}


def _mesh():
    import fem355  # noqa: F401
    from fem355 import mesh
    return mesh


def _orthogonal(seed=7):
    q, r = torch.linalg.qr(torch.randn(3, 3, dtype=F64, generator=torch.Generator().manual_seed(seed)))
    return q * torch.sign(torch.diagonal(r))


def _transform(c, case):
    if case in ("plain", "flipped", "unflipped"):
        return c.clone()
    if case.startswith("shift"):
        return c + float(case[5:]) * torch.tensor(SHIFT_DIR, dtype=F64)
    if case.startswith("scale"):
        return c * float(case[5:])
    if case.startswith("squash"):
        c = c * torch.tensor([1.0, 1.0, 1e-4], dtype=F64)
        return c @ _orthogonal().T if case.endswith("_rot") else c
    raise KeyError(case)


def linear_map(case):
    """The 3 x 3 matrix L of `_transform`: transformed = c @ L.T (+ the shift). Fields that must not depend on the
    absolute coordinates are defined on the unit mesh and pushed through L (u @ L.T)."""
    if case in ("plain", "flipped", "unflipped") or case.startswith("shift"):
        return torch.eye(3, dtype=F64)
    if case.startswith("scale"):
        return float(case[5:]) * torch.eye(3, dtype=F64)
    if case.startswith("squash"):
        L = torch.diag(torch.tensor([1.0, 1.0, 1e-4], dtype=F64))
        return _orthogonal() @ L if case.endswith("_rot") else L
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def tet4_case(case):
    """(coords [64, 3], tets [162, 4]): kuhn_cube(3, jitter 0.15), every second element's local order [1, 0, 2, 3]
    (81 negative dets) unless case == "unflipped"; then the case's transform."""
    c, t = _mesh().kuhn_cube(3, jitter=0.15)
    t = t.clone()
    if case != "unflipped":
        t[1::2] = t[1::2][:, [1, 0, 2, 3]]
    return _transform(c, case).contiguous(), t.contiguous()


def tet4_h(case):
    c, _ = tet4_case(case)
    return float((c.max(0).values - c.min(0).values).max()) / 3.0


@functools.lru_cache(maxsize=None)
def tet4_u(case):
    """Seeded displacement of magnitude 1e-6 h."""
    c, _ = tet4_case(case)
    return 1e-6 * tet4_h(case) * torch.randn(c.shape[0], 3, dtype=F64, generator=torch.Generator().manual_seed(21))


@functools.lru_cache(maxsize=None)
def tet4_x(case, kind):
    c, _ = tet4_case(case)
    return torch.randn(c.shape[0], 3 if kind == "elastic" else 1, dtype=F64,
                       generator=torch.Generator().manual_seed(22))


_TET4_PAR = {"elastic": (E, NU), "poisson": (KAPPA, 0.0), "mass": (RHO, 0.0)}


@functools.lru_cache(maxsize=None)
def _tet4_K_fr(case, kind):
    c, t = tet4_case(case)
    return tet4_K_fr(c, t, kind, *_TET4_PAR[kind])


@functools.lru_cache(maxsize=None)
def tet4_exact(case, quantity):
    """Exact reference of one quantity of one c3d4 case: "vol", "B", "K_elastic", "K_poisson", "K_mass", "stress"
    (sigma, vm), "ebe_elastic" / "ebe_poisson" (y, diag, mag, 1 / diag for tet4_x)."""
    c, t = tet4_case(case)
    if quantity == "vol":
        return tet4_volumes(c, t)
    if quantity == "B":
        return tet4_B(c, t)
    if quantity.startswith("K_"):
        return to_tensor(_tet4_K_fr(case, quantity[2:]))
    if quantity == "stress":
        return tet4_stress(c, t, tet4_u(case))
    if quantity.startswith("ebe_"):
        kind = quantity[4:]
        return ebe_products(_tet4_K_fr(case, kind), t, tet4_x(case, kind))
    raise KeyError(quantity)


@functools.lru_cache(maxsize=None)
def tet4_calibration(case, quantity):
    """The fp64 edge-difference form's value of the same quantity (tet4_exact's keys)."""
    c, t = tet4_case(case)
    if quantity == "vol":
        return tet4_geom_edges_fp64(c, t)[0].abs() / 6.0
    if quantity == "B":
        return R._voigt_B(tet4_geom_edges_fp64(c, t)[1])
    if quantity.startswith("K_"):
        kind = quantity[2:]
        return tet4_K_edges_fp64(c, t, *_TET4_PAR[kind], kind=kind)
    if quantity == "stress":
        B = R._voigt_B(tet4_geom_edges_fp64(c, t)[1])
        return R._point_stress(B, tet4_u(case)[t].reshape(t.shape[0], -1), R.elasticity_matrix(E, NU))
    if quantity.startswith("ebe_"):
        kind = quantity[4:]
        K = tet4_calibration(case, "K_" + kind)
        x = tet4_x(case, kind)
        dpn = x.shape[1]
        y = R.nodal_forces(K, t, x).reshape(-1)
        d = torch.zeros(x.numel(), dtype=F64).index_add_(0, R.dof_map(t, dpn).reshape(-1),
                                                         torch.diagonal(K, dim1=1, dim2=2).reshape(-1))
        return y, d
    raise KeyError(quantity)


def tet4_calibration_err(case, quantity, part=None):
    """Error of the calibration form against the exact value, in the measure the tests use for that quantity.
    part: "sigma" / "vm" of "stress"; "y" / "diag" of "ebe_*"."""
    ex, cal = tet4_exact(case, quantity), tet4_calibration(case, quantity)
    if quantity == "stress":
        i = ("sigma", "vm").index(part)
        return elem_err(cal[i], ex[i])
    if quantity.startswith("ebe_"):
        y, d, mag, dinv = ex
        return dof_err(cal[0], y, mag) if part == "y" else dof_err(1.0 / cal[1], dinv, dinv.abs())
    return elem_err(cal, ex)


def _iso_sign(c, e, etype):
    p, _ = R.POINTS[etype]()
    dets = torch.stack([torch.det(R.iso_jacobian(c, e, R.DN[etype](*[float(v) for v in q]))) for q in p], 1)
    assert bool(((dets > 0).all(1) | (dets < 0).all(1)).all()), "detJ changes sign inside an element"
    return dets[:, 0] > 0


@functools.lru_cache(maxsize=None)
def iso_case(etype, case):
    """(coords, elements, positive [M] bool (detJ > 0 at every rule point), sample [8] element ids, 4 of each sign).
    c3d8: hex_box(3, jitter 0.1), every second hex reordered [4, 5, 6, 7, 0, 1, 2, 3]; c3d6: wedge_box(3, jitter 0.1),
    every second wedge [3, 4, 5, 0, 1, 2]; c3d10: tet10_cube(2, jitter 0.1) followed by a z-mirrored copy on nodes of
    its own. case "unflipped": the generator's mesh as it comes (sample: the first 8 elements)."""
    m = _mesh()
    if etype == "c3d10":
        c, e = m.tet10_cube(2, jitter=0.1)
        if case != "unflipped":
            e = torch.cat([e, e + c.shape[0]], 0)
            c = torch.cat([c, c * torch.tensor([1.0, 1.0, -1.0], dtype=F64)], 0)
    else:
        c, e = (m.hex_box if etype == "c3d8" else m.wedge_box)(3, jitter=0.1)
        e = e.clone()
        if case != "unflipped":
            e[1::2] = e[1::2][:, _ISO_REORDER[etype]]
    c = _transform(c, case).contiguous()
    pos = _iso_sign(c, e, etype)
    if case == "unflipped":
        sample = torch.arange(8)
    else:
        sample = torch.cat([torch.nonzero(pos).view(-1)[:4], torch.nonzero(~pos).view(-1)[:4]]).sort().values
        assert sample.numel() == 8
    return c, e.contiguous(), pos, sample


def iso_h(etype, case):
    c = iso_case(etype, case)[0]
    return float((c.max(0).values - c.min(0).values).max()) / 3.0


@functools.lru_cache(maxsize=None)
def iso_u(etype, case):
    c = iso_case(etype, case)[0]
    return 1e-6 * iso_h(etype, case) * torch.randn(c.shape[0], 3, dtype=F64,
                                                    generator=torch.Generator().manual_seed(23))


def iso_geom_point(etype):
    """The rule point at which J and the gradients are compared (the rule's second point: off-centre)."""
    return R.POINTS[etype]()[0][1]


@functools.lru_cache(maxsize=None)
def iso_exact(etype, case, quantity):
    """Exact reference on the case's 8-element sample: "K" (single=True, single=False), "mass", "stress" (sigma, vm),
    "geom" (J, gradients at iso_geom_point)."""
    c, e, _, s = iso_case(etype, case)
    if quantity == "K":
        return iso_K(c, e[s], etype)
    if quantity == "mass":
        return iso_mass(c, e[s], etype)
    if quantity == "stress":
        return iso_stress(c, e[s], iso_u(etype, case), etype)
    if quantity == "geom":
        return iso_point(c, e[s], etype, iso_geom_point(etype))
    raise KeyError(quantity)


@functools.lru_cache(maxsize=None)
def iso_calibration(etype, case, quantity):
    """The oracle's value of the same quantity on the same sample."""
    c, e, _, s = iso_case(etype, case)
    if quantity == "K":
        return R.iso_K(c, e[s], etype, E, NU), R.iso_K(c, e[s], etype, E, NU, single=False)
    if quantity == "mass":
        el_ = _el()
        p, w = el_.mass_integration_points(etype)
        return R.iso_mass(c, e[s], el_._N[etype], R.DN[etype], p, w, RHO)
    if quantity == "stress":
        return R.iso_stress(c, e[s], iso_u(etype, case), etype, E, NU, single=True)
    if quantity == "geom":
        dN = R.DN[etype](*[float(v) for v in iso_geom_point(etype)])
        return R.iso_jacobian(c, e[s], dN), R.iso_gradients(c, e[s], dN)
    raise KeyError(quantity)


def stack_first(K, etype):
    """single=False result with the element axis first (c3d8 / c3d10 come point-major)."""
    return K if etype == "c3d6" else K.transpose(0, 1)


def iso_calibration_err(etype, case, quantity, part=0):
    ex, cal = iso_exact(etype, case, quantity), iso_calibration(etype, case, quantity)
    if quantity == "mass":
        return elem_err(cal, ex)
    a, b = cal[part], ex[part]
    if quantity == "K" and part == 1:
        a, b = stack_first(a, etype), stack_first(b, etype)
    return elem_err(a, b)


# ----------------------------------------------------------------------------- singular threshold
@functools.lru_cache(maxsize=None)
def threshold_case(with_singular):
    """The flipped c3d4 mesh scaled so that min|det| = 4e-12 (above the reference's absolute |det| < 1e-12 test,
    `solver/element.py:857`); with_singular: one tet on 4 nodes of its own with |det| = 2.5e-13 inserted at element
    index 140."""
    c, t = tet4_case("flipped")
    det = R.tet4_cofactors(c, t)[1].abs().min()
    c = c * float((4e-12 / det) ** (1.0 / 3.0))
    if with_singular:
        a = 2.5e-13 ** (1.0 / 3.0)
        extra = c.mean(0) + a * torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F64)
        n = c.shape[0]
        c = torch.cat([c, extra], 0)
        t = torch.cat([t[:140], torch.arange(n, n + 4).view(1, 4), t[140:]], 0)
    return c.contiguous(), t.contiguous()
