"""Dense CPU reference for linear buckling (torch fp64 only), written from the formulas of DESIGN §8r -- the reference
project has no buckling analysis.

  * geo_scalar: Gs_e[a][b] = sum_q w_q |detJ_q| grad N_a(q)^T sigma_q grad N_b(q) by plain einsum over the quadrature
    tables of element.geometric_integration_points, sigma_q = D(E, nu) B_q u_e (+ the element's constant sigma0);
  * elem_K / dense: the stiffness the buckling solver assembles (|detJ|, rules that sum to the reference volume);
  * dense_pairs: the pencil G phi = theta K phi on the free dofs through a Cholesky factor of K and eigh,
    |theta| descending, lambda = -1 / theta;
  * subspace_ref: the block subspace iteration of SellMatrix.buckling_lowest with Cholesky solves in the place of PCG.

Columns: a fem355.mesh box scaled by (1, 1.5, 8), the z = 0 face clamped, a unit axial compression spread over the
top face's nodes, E = 1000, nu = 0.3."""
import functools

import torch

from oracle import ref_cpu as R

F64 = torch.float64
E, NU = 1000.0, 0.3
SCALE = torch.tensor([1.0, 1.5, 8.0], dtype=F64)
NPE = {"c3d4": 4, "c3d6": 6, "c3d8": 8, "c3d10": 10}
CONVERGED, MAXITER, BREAKDOWN = 1, 2, 3   # _capi.PCG_*
COND, THETA_FLOOR = 1e12, 1e-12           # system.MODAL_COND / MODAL_THETA_FLOOR


def tables(et):
    """(dN [n, npe, 3], w [n]) of the geometric stiffness' rule."""
    from fem355 import element
    return element.geometric_integration_points(et)


def jacobians(coords, el, et):
    """(J [M, n, 3, 3], det [M, n]) at the rule's points: J[i][k] = sum_j dN[j][i] x_j[k]."""
    dN, _ = tables(et)
    J = torch.einsum("qji,mjk->mqik", dN, coords.to(F64)[el])
    return J, torch.linalg.det(J)


def lame(E_, nu):
    c = E_ / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return c * nu, c * (1.0 - 2.0 * nu) / 2.0


def point_stress(coords, el, et, u=None, E_=None, nu=None, sigma0=None):
    """sigma [M, n, 3, 3] at the rule's points and the global gradients g [M, n, npe, 3]."""
    dN, _ = tables(et)
    J, _ = jacobians(coords, el, et)
    g = torch.einsum("mqil,qnl->mqni", torch.linalg.inv(J), dN)
    M, n = J.shape[:2]
    sig = torch.zeros((M, n, 3, 3), dtype=F64)
    if u is not None:
        lam, mu = lame(E_, nu)
        H = torch.einsum("mnc,mqnk->mqck", u.to(F64)[el], g)
        eps = 0.5 * (H + H.transpose(-1, -2))
        tr = eps.diagonal(dim1=-2, dim2=-1).sum(-1)
        sig = sig + lam * tr[..., None, None] * torch.eye(3, dtype=F64) + 2.0 * mu * eps
    if sigma0 is not None:
        s = sigma0.to(F64)
        s = s.triu() + s.triu(1).transpose(-1, -2)        # the upper triangle is what counts
        sig = sig + s[:, None]
    return sig, g


def geo_scalar(coords, el, et, u=None, E_=None, nu=None, sigma0=None):
    """Gs [M, npe, npe] of the formula above."""
    if u is None and sigma0 is None:
        raise ValueError("geo_scalar: a displacement, a prestress or both")
    _, w = tables(et)
    _, det = jacobians(coords, el, et)
    sig, g = point_stress(coords, el, et, u, E_, nu, sigma0)
    return torch.einsum("q,mq,mqai,mqik,mqbk->mab", w, det.abs(), g, sig, g)


def elem_K(coords, el, et, E_=E, nu=NU):
    """Element stiffness of solver._buckling_ke from the oracle's restatements: |detJ| and volume-true weights."""
    from fem355 import element
    if et == "c3d4":
        return R.tet4_K(coords, el, E_, nu)
    if et == "c3d8":
        K = R.iso_K(coords, el, "c3d8", E_, nu)
    else:
        p, w = element.mass_integration_points(et)
        K = R.iso_K(coords, el, et, E_, nu, points=p, weights=w, single=(et == "c3d10"))
    centre = {"c3d8": (0.0, 0.0, 0.0), "c3d6": (1 / 3, 1 / 3, 0.0), "c3d10": (0.25, 0.25, 0.25)}[et]
    sign = torch.sign(torch.det(R.iso_jacobian(coords, el, R.DN[et](*centre))))
    return K * sign.view(-1, 1, 1)


def dense(Ke, el, N, dpn):
    """Dense [N dpn, N dpn] sum of P_e^T K_e P_e."""
    dofs = (el.unsqueeze(-1) * dpn + torch.arange(dpn).view(1, 1, dpn)).reshape(el.shape[0], -1)
    n, d = N * dpn, dofs.shape[1]
    A = torch.zeros(n * n, dtype=F64)
    A.index_add_(0, (dofs.unsqueeze(2) * n + dofs.unsqueeze(1)).reshape(-1), Ke.reshape(-1, d * d).reshape(-1))
    return A.view(n, n)


def kron3(Gs):
    return torch.kron(Gs, torch.eye(3, dtype=F64).view(1, 3, 3))


def dense_pairs(K, G, free):
    """(theta [nf] by |theta| descending, U [n, nf] K-orthonormal with zero rows on the fixed dofs) of G phi = theta K phi."""
    L = torch.linalg.cholesky(K[free][:, free])
    T = torch.linalg.solve_triangular(L, G[free][:, free], upper=False)
    T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)
    th, Z = torch.linalg.eigh(0.5 * (T + T.T))
    order = torch.argsort(th.abs(), descending=True, stable=True)
    U = torch.zeros((K.shape[0], th.numel()), dtype=F64)
    U[free] = torch.linalg.solve_triangular(L.T.contiguous(), Z[:, order].contiguous(), upper=True)
    return th[order], U


def _ritz(GG, GK, m):
    """system.rayleigh_ritz on (X^T G X, X^T K X), restated, with the pairs reordered by |theta| descending."""
    d = GK.diagonal()
    if not bool(torch.isfinite(GG).all() and torch.isfinite(GK).all()) or bool((d <= 0).any()):
        return None
    s = d.rsqrt()
    A, B = s[:, None] * GG * s[None, :], s[:, None] * GK * s[None, :]
    ev = torch.linalg.eigvalsh(B)
    if not float(ev[0]) > 0.0 or float(ev[-1] / ev[0]) > COND:
        return None
    L, info = torch.linalg.cholesky_ex(B)
    if int(info) != 0:
        return None
    T = torch.linalg.solve_triangular(L, A, upper=False)
    T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)
    th, Z = torch.linalg.eigh(0.5 * (T + T.T))
    if not bool(torch.isfinite(th).all()):
        return None
    C = s[:, None] * torch.linalg.solve_triangular(L.T.contiguous(), Z[:, :m].contiguous(), upper=True)
    order = torch.argsort(th[:m].abs(), descending=True, stable=True)
    return th[:m][order], C[:, order]


def subspace_ref(K, G, free, k, m, tol=1e-8, max_iter=200, seed=0):
    """Dense restatement of SellMatrix.buckling_lowest with exact K-solves on the free dofs.
    Returns (factors [k], theta [k], X [n, k], iterations, status, residuals [k])."""
    n = K.shape[0]
    Lf = torch.linalg.cholesky(K[free][:, free])
    X = torch.randn((n, m), dtype=F64, generator=torch.Generator().manual_seed(seed)) * free[:, None]
    nan = torch.full((k,), float("nan"), dtype=F64)

    def products(X):
        KX, GX = K @ X, G @ X
        GG, GK = X.T @ GX, X.T @ KX
        return KX, GX, GG.triu() + GG.triu(1).T, GK.triu() + GK.triu(1).T   # upper triangle mirrored, as the kernel

    KX, GX, GG, GK = products(X)
    rr = _ritz(GG, GK, m)
    if rr is None or not float(rr[0].abs().max()) > 0.0:
        return nan, torch.zeros(k, dtype=F64), X[:, :k], 0, BREAKDOWN, nan
    theta, C = rr
    ref = float(theta.abs().max())
    X, KX, GX = X @ C, KX @ C, GX @ C
    status, rel = MAXITER, nan
    for it in range(max_iter + 1):
        Rr = (GX - KX * theta)[free]
        rel = (Rr.norm(dim=0) / (theta.abs() * KX[free].norm(dim=0)))[:k]
        if not bool(torch.isfinite(rel).all()):
            status = BREAKDOWN
            break
        if bool((rel <= tol).all()):
            status = CONVERGED
            break
        if it == max_iter:
            break
        Y = torch.zeros_like(X)
        Y[free] = torch.cholesky_solve(-GX[free], Lf)
        X = Y
        KX, GX, GG, GK = products(X)
        rr = _ritz(GG, GK, m)
        if rr is None or float(rr[0].abs().max()) <= THETA_FLOOR * ref:
            status = BREAKDOWN
            break
        theta, C = rr
        X, KX, GX = X @ C, KX @ C, GX @ C
    th = theta[:k].clone()
    return -1.0 / th, th, X[:, :k].clone(), it, status, rel


# ---------------------------------------------------------------- the column cases
def column_mesh(kind, n, jitter=0.0):
    """(coords scaled to the column, connectivity, element type) of a fem355.mesh box."""
    from fem355 import mesh
    gen, et = {"tet": (mesh.kuhn_cube, "c3d4"), "hex": (mesh.hex_box, "c3d8"), "wedge": (mesh.wedge_box, "c3d6"),
               "tet10": (mesh.tet10_cube, "c3d10")}[kind]
    c, el = gen(n, jitter=jitter)
    return c * SCALE, el, et


def top_load(coords, total=-1.0):
    """[N, 3]: `total` in z spread evenly over the nodes of the top face (negative: compression)."""
    top = torch.nonzero((coords[:, 2] - coords[:, 2].max()).abs() <= 1e-12, as_tuple=True)[0]
    F = torch.zeros((coords.shape[0], 3), dtype=F64)
    F[top, 2] = total / top.numel()
    return F


def hex_column(nx, ny, nz, dims):
    """A structured nx x ny x nz c3d8 box of size dims, node (i, j, k) at (i * (ny + 1) + j) * (nz + 1) + k, corners in
    fem355.mesh.HEX_CORNERS order -> (coords, connectivity)."""
    from fem355 import mesh
    ax = [torch.arange(m + 1, dtype=F64) * (d / m) for m, d in zip((nx, ny, nz), dims)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    coords = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1)
    I, J, K_ = (t.reshape(-1) for t in torch.meshgrid(torch.arange(nx), torch.arange(ny), torch.arange(nz),
                                                      indexing="ij"))
    cols = [((I + di) * (ny + 1) + (J + dj)) * (nz + 1) + (K_ + dk) for (di, dj, dk) in mesh.HEX_CORNERS]
    return coords, torch.stack(cols, dim=1).to(torch.long)


def top_pressure(coords, el, p=1.0):
    """[N, 3]: the consistent nodal loads of a pressure p on the top faces (local nodes 4..7) of a structured c3d8
    column with flat rectangular faces: a quarter of the face's area times -p to each of its nodes."""
    zmax = coords[:, 2].max()
    F = torch.zeros((coords.shape[0], 3), dtype=F64)
    for e in range(el.shape[0]):
        q = el[e, 4:8]
        if bool((coords[q, 2] - zmax).abs().max() <= 1e-12):
            a = coords[q]
            area = float((a[:, 0].max() - a[:, 0].min()) * (a[:, 1].max() - a[:, 1].min()))
            F[q, 2] -= p * area / 4.0
    return F


class Column:
    """One column clamped at z = 0 (or at the nodes `fixed`) under a load F: dense K, the reference state, dense G and
    the free dofs. fams: [(element type, connectivity)]."""

    def __init__(self, coords, fams, F, fixed=None):
        self.c, self.fams, self.F = coords, fams, F
        self.et, self.el = fams[0]
        self.N = self.c.shape[0]
        self.n = 3 * self.N
        self.fixed = torch.nonzero(self.c[:, 2].abs() <= 1e-12, as_tuple=True)[0] if fixed is None else fixed
        free = torch.ones((self.N, 3), dtype=torch.bool)
        free[self.fixed] = False
        self.free = free.view(-1)
        self.K = sum(dense(elem_K(self.c, el, et), el, self.N, 3) for et, el in self.fams)
        self.u = self.solve(self.F)
        self.G = self.geometric(self.u)

    def solve(self, F):
        u = torch.zeros(self.n, dtype=F64)
        f = self.free
        u[f] = torch.linalg.solve(self.K[f][:, f], F.reshape(-1)[f])
        return u.view(self.N, 3)

    def geometric(self, u=None, sigma0=None):
        """Dense K_g = G_s (x) I3 of a displacement and / or per-family prestress {type: [M, 3, 3]}."""
        s0 = sigma0 or {}
        return sum(dense(kron3(geo_scalar(self.c, el, et, u, E, NU, s0.get(et))), el, self.N, 3)
                   for et, el in self.fams)

    @functools.cached_property
    def pairs(self):
        return dense_pairs(self.K, self.G, self.free)

    def residuals(self, theta, X, G=None):
        """||G x - theta K x|| / (|theta| ||K x||) over the free dofs with the dense matrices."""
        G = self.G if G is None else G
        X, theta = X.cpu().to(F64), theta.cpu().to(F64)
        KX = (self.K @ X)[self.free]
        return ((G @ X)[self.free] - KX * theta).norm(dim=0) / (theta.abs() * KX.norm(dim=0))


@functools.lru_cache(maxsize=None)
def column(kind, n, total=-1.0):
    """The box column of column_mesh(kind, n) under `total` spread over its top nodes."""
    c, el, et = column_mesh(kind, n)
    return Column(c, [(et, el)], top_load(c, total))


@functools.lru_cache(maxsize=None)
def slender_hex_column(total=1.0):
    """The 2 x 3 x 8-hex column of 1 x 1.5 x 10 under an axial compression of `total` (negative: tension), applied as
    the consistent nodal loads of a uniform pressure on the top face."""
    c, el = hex_column(2, 3, 8, (1.0, 1.5, 10.0))
    return Column(c, [("c3d8", el)], top_pressure(c, el, total / 1.5))
