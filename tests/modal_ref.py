"""Dense CPU reference for the modal solver (torch only): K and M of the test meshes from the oracle's element
matrices, the generalised eigensolve on the free dofs via Cholesky, and a plain dense restatement of the block LOBPCG
that SellMatrix.eig_lowest runs on the device ("the reference LOBPCG").

Meshes: mesh.kuhn_cube(n, jitter=0.15) / mesh.hex_box(n) scaled by (1, 0.7, 2) so that no two low modes coincide, the
z = 0 face clamped, E = 113.8e9, nu = 0.342, rho = 4430. The consistent P1 mass is rho V (1 + delta_ab) / 20 per
component; the hex mass is the oracle's `R.iso_mass`; the lumped mass is the reference's sum of the element matrices'
diagonals clamped at 1e-12 (`solver/solver.py:1126-1134`)."""
import functools

import torch

from oracle import ref_cpu as R

F64 = torch.float64
E, NU, RHO = 113.8e9, 0.342, 4430.0
SCALE = torch.tensor([1.0, 0.7, 2.0], dtype=F64)
CONVERGED, MAXITER, BREAKDOWN = 1, 2, 3   # _capi.PCG_*
COND, THETA_FLOOR = 1e12, 1e-12           # system.MODAL_COND / MODAL_THETA_FLOOR

# name -> (mesh, n, operator, mass, k, m)
CASES = {
    "elastic4": ("tet", 4, "elastic", "consistent", 4, 8),
    "elastic6": ("tet", 6, "elastic", "consistent", 6, 8),
    "elastic8": ("tet", 8, "elastic", "consistent", 3, 4),
    "lumped5": ("tet", 5, "elastic", "lumped", 6, 8),
    "poisson6": ("tet", 6, "poisson", "consistent", 6, 8),
    "hex4": ("hex", 4, "elastic", "consistent", 4, 8),
}


def tet_scalar_mass(coords, tets, rho=RHO):
    """Scalar factor [M, 4, 4] of the consistent P1 mass: rho V (1 + delta_ab) / 20."""
    V = R.tet_volumes(coords, tets)
    return (rho * V / 20.0).view(-1, 1, 1) * (torch.ones((4, 4), dtype=F64) + torch.eye(4, dtype=F64))


def hex_scalar_mass(coords, hexes, rho=RHO):
    from fem355 import element as el
    pts, wts = el.mass_integration_points("c3d8")
    return R.iso_mass(coords, hexes, el._N["c3d8"], el._ISO["c3d8"][1], pts, wts, rho)[:, ::3, ::3].contiguous()


def dense(Ke, elements, N, dpn):
    """Dense [N dpn, N dpn] sum of P_e^T K_e P_e."""
    dofs = (elements.unsqueeze(-1) * dpn + torch.arange(dpn).view(1, 1, dpn)).reshape(elements.shape[0], -1)
    n, d = N * dpn, dofs.shape[1]
    A = torch.zeros(n * n, dtype=F64)
    idx = (dofs.unsqueeze(2) * n + dofs.unsqueeze(1)).reshape(-1)
    A.index_add_(0, idx, Ke.reshape(-1, d * d).reshape(-1))
    return A.view(n, n)


def lumped_diag(Me, elements, N, dpn=3):
    """`solver/solver.py:1126-1134`: the element matrices' diagonals summed per dof, clamped at 1e-12."""
    dofs = (elements.unsqueeze(-1) * dpn + torch.arange(dpn).view(1, 1, dpn)).reshape(-1)
    d = torch.zeros(N * dpn, dtype=F64)
    d.index_add_(0, dofs, Me.diagonal(dim1=1, dim2=2).reshape(-1))
    return d.clamp(min=1e-12)


class Case:
    """One mesh: element matrices, dense K and M, the clamped nodes, the Jacobi weights and the free dofs."""

    def __init__(self, name, clamp=True):
        from fem355 import mesh
        kind, n, op, mass, self.k, self.m = CASES[name]
        self.name, self.op, self.mass = name, op, mass
        c, el = (mesh.kuhn_cube(n, jitter=0.15) if kind == "tet" else mesh.hex_box(n))
        self.fixed = mesh.face_nodes(c, 2, 0.0) if clamp else torch.zeros(0, dtype=torch.long)
        self.c, self.el = c * SCALE, el
        self.N = c.shape[0]
        self.dpn = 1 if op == "poisson" else 3
        self.n = self.N * self.dpn
        if kind == "hex":
            self.Ke = R.iso_K(self.c, el, "c3d8", E, NU)
            self.Ms = hex_scalar_mass(self.c, el)
        else:
            self.Ke = R.tet4_K(self.c, el, E, NU) if op == "elastic" else R.tet4_poisson_K(self.c, el)
            self.Ms = tet_scalar_mass(self.c, el)
        # the full element mass M_s (x) I_dpn
        self.Me = torch.kron(self.Ms, torch.eye(self.dpn, dtype=F64).view(1, self.dpn, self.dpn))
        self.K = dense(self.Ke, el, self.N, self.dpn)
        if mass == "lumped":
            self.mdiag = lumped_diag(self.Me, el, self.N, self.dpn)
            self.M = torch.diag(self.mdiag)
        else:
            self.M = dense(self.Me, el, self.N, self.dpn)
        free = torch.ones((self.N, self.dpn), dtype=torch.bool)
        free[self.fixed] = False
        self.free = free.view(-1)
        self.w = torch.where(self.free, 1.0 / self.K.diagonal(), torch.zeros(self.n, dtype=F64))

    @functools.cached_property
    def eig(self):
        """(lam [nf] ascending, U [n, nf] M-orthonormal, zero rows on the fixed dofs) of the dense pencil."""
        f = self.free
        L = torch.linalg.cholesky(self.M[f][:, f])
        T = torch.linalg.solve_triangular(L, self.K[f][:, f], upper=False)
        T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)
        lam, Z = torch.linalg.eigh(0.5 * (T + T.T))
        U = torch.zeros((self.n, lam.numel()), dtype=F64)
        U[f] = torch.linalg.solve_triangular(L.T.contiguous(), Z, upper=True)
        return lam, U

    @functools.cached_property
    def lobpcg(self):
        """The reference LOBPCG at tol 1e-8 on this case: (lam, X, iterations, status, residuals, restarts)."""
        return lobpcg_ref(self.K, self.M, self.w, self.k, self.m, tol=1e-8)

    def eig_error(self, lam):
        """Worst relative error of lam [k] against the dense eigenvalues."""
        ref = self.eig[0][: lam.numel()]
        return float(((lam.cpu() - ref).abs() / ref).max())

    def residuals(self, lam, X):
        """||K x - lam M x|| / (lam ||M x||) over the free dofs, recomputed with the dense matrices."""
        X, lam = X.cpu().to(F64), lam.cpu().to(F64)
        MX = (self.M @ X)[self.free]
        Rr = (self.K @ X)[self.free] - MX * lam
        return Rr.norm(dim=0) / (lam * MX.norm(dim=0))


@functools.lru_cache(maxsize=None)
def case(name, clamp=True):
    return Case(name, clamp)


def _ritz(GK, GM, m):
    """Rayleigh-Ritz of the issue's recipe: scale by diag(GM)^(-1/2), Cholesky, eigh; None when GM is unsafe."""
    d = GM.diagonal()
    if not bool(torch.isfinite(GK).all() and torch.isfinite(GM).all()) or bool((d <= 0).any()):
        return None
    s = d.rsqrt()
    A, B = s[:, None] * GK * s[None, :], s[:, None] * GM * s[None, :]
    ev = torch.linalg.eigvalsh(B)
    if not float(ev[0]) > 0.0 or float(ev[-1] / ev[0]) > COND:
        return None
    L, info = torch.linalg.cholesky_ex(B)
    if int(info) != 0:
        return None
    T = torch.linalg.solve_triangular(L, A, upper=False)
    T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)
    lam, Z = torch.linalg.eigh(0.5 * (T + T.T))
    return lam[:m], s[:, None] * torch.linalg.solve_triangular(L.T.contiguous(), Z[:, :m].contiguous(), upper=True)


def lobpcg_ref(K, M, w, k, m, tol=1e-8, max_iter=2000, seed=0, X0=None):
    """Dense restatement of SellMatrix.eig_lowest: X, W, P and their K- and M-products carried, only W multiplied by
    the matrices per iteration, Rayleigh-Ritz on [X W P] (restart without P when the Gram matrix is unsafe), rotation
    of the nine blocks. `w` [n]: Jacobi weights, zero on the fixed dofs."""
    n = K.shape[0]
    free = w != 0
    X = torch.randn((n, m), dtype=F64, generator=torch.Generator().manual_seed(seed))
    if X0 is not None:
        X[:, : X0.shape[1]] = X0
    X = X * free[:, None]
    KX, MX = K @ X, M @ X
    rr = _ritz(X.T @ KX, X.T @ MX, m)
    nan = torch.full((k,), float("nan"), dtype=F64)
    if rr is None or bool((rr[0] <= THETA_FLOOR * rr[0].abs().max()).any()):
        return torch.zeros(k, dtype=F64), X[:, :k], 0, BREAKDOWN, nan, 0
    theta, C = rr
    ref = float(theta.max())
    X, KX, MX = X @ C, KX @ C, MX @ C
    P = KP = MP = None
    restarts, status, rel = 0, MAXITER, nan
    for it in range(max_iter + 1):
        Rr = KX - MX * theta
        W = w[:, None] * Rr
        rel = (Rr[free].norm(dim=0) / (theta * MX[free].norm(dim=0)))[:k]
        if not bool(torch.isfinite(rel).all()):
            status = BREAKDOWN
            break
        if bool((rel <= tol).all()):
            status = CONVERGED
            break
        if it == max_iter:
            break
        KW, MW = K @ W, M @ W
        S = [X, W] + ([P] if P is not None else [])
        KS = [KX, KW] + ([KP] if P is not None else [])
        MS = [MX, MW] + ([MP] if P is not None else [])
        Sc, KSc, MSc = torch.cat(S, 1), torch.cat(KS, 1), torch.cat(MS, 1)
        GK, GM = Sc.T @ KSc, Sc.T @ MSc
        GK, GM = GK.triu() + GK.triu(1).T, GM.triu() + GM.triu(1).T   # upper triangle mirrored, as the kernel
        a = len(S)
        rr = _ritz(GK, GM, m)
        if rr is None and a == 3:
            restarts += 1
            a = 2
            rr = _ritz(GK[: 2 * m, : 2 * m], GM[: 2 * m, : 2 * m], m)
        if rr is None or not bool(torch.isfinite(rr[0]).all()) or bool((rr[0] <= THETA_FLOOR * ref).any()):
            status = BREAKDOWN
            break
        theta, C = rr
        CX, CW = C[:m], C[m: 2 * m]
        P, KP, MP = W @ CW, KW @ CW, MW @ CW
        if a == 3:
            CP = C[2 * m:]
            P, KP, MP = P + S[2] @ CP, KP + KS[2] @ CP, MP + MS[2] @ CP
        X, KX, MX = X @ CX + P, KX @ CX + KP, MX @ CX + MP
    return theta[:k].clone(), X[:, :k].clone(), it, status, rel, restarts
