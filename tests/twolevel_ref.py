"""Dense restatement of the two-level preconditioner M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T (torch on the host, fp64)
on `oracle.ref_cpu`'s element matrices: Z, E, T and the dropped count, Einv, the preconditioner as an operator, PCG
with the device context's semantics, and a dense direct solve. Nothing here is shared with the package's code except
`dist.rcb_partition` (the aggregation both sides are given) and the Kuhn split tables of `mesh`.

`descending=True` evaluates everything under the reversed node numbering (so every sum over an aggregate's nodes runs
through its list in descending order) and maps results back: the spread between the two is what summation order
alone does to a result, the unit of the device tests' tolerances."""
import numpy as np
import torch

import fem355  # noqa: F401
from fem355 import dist
from fem355.mesh import HEX_CORNERS, KUHN_TETS
from oracle import ref_cpu as R

F64 = torch.float64
EPS = 2.0 ** -52
E_MOD, NU = 113.8e9, 0.342   # tests/modal_ref.py's material
DROP = 1e-10


def kuhn_box(nx, ny, nz, size=(1.0, 1.0, 1.0), jitter=0.0, seed=1234):
    """Box of 6 nx ny nz Kuhn tets over [0, size]; nodes lexicographic ((i (ny + 1) + j) (nz + 1) + k); interior nodes
    moved by up to +-jitter h per axis."""
    ax = [torch.arange(n + 1, dtype=F64) * (s / n) for n, s in zip((nx, ny, nz), size)]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    coords = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], 1)
    if jitter:
        rng = np.random.default_rng(seed)
        d = torch.from_numpy(rng.uniform(-jitter, jitter, size=tuple(coords.shape)))
        h = torch.tensor([s / n for n, s in zip((nx, ny, nz), size)], dtype=F64)
        inner = torch.ones(coords.shape[0], dtype=torch.bool)
        for a, s in enumerate(size):
            inner &= (coords[:, a] > 1e-12) & (coords[:, a] < s - 1e-12)
        coords[inner] += (d * h)[inner]
    I, J, K = (t.reshape(-1) for t in torch.meshgrid(torch.arange(nx), torch.arange(ny), torch.arange(nz),
                                                     indexing="ij"))
    hexes = torch.stack([((I + di) * (ny + 1) + (J + dj)) * (nz + 1) + (K + dk) for di, dj, dk in HEX_CORNERS], 1)
    tets = torch.stack([hexes[:, list(t)] for t in KUHN_TETS], 1).reshape(-1, 4).contiguous()
    return coords, tets.long()


def beam_case(nx=3, ny=3, nz=24, size=(1.0, 1.0, 8.0), jitter=0.15):
    """The issue's beam: z = 0 face clamped, lateral (x) load over the far face. -> coords, tets, F [N, 3], fixed."""
    coords, tets = kuhn_box(nx, ny, nz, size, jitter)
    fixed = torch.nonzero(coords[:, 2].abs() <= 1e-12).view(-1)
    far = torch.nonzero((coords[:, 2] - size[2]).abs() <= 1e-12).view(-1)
    F = torch.zeros((coords.shape[0], 3), dtype=F64)
    F[far, 0] = 1e6 / far.numel()
    return coords, tets, F, fixed


def dense_matrix(families, N):
    """families [(K_e [M, d, d], connectivity [M, npe])] -> A [3N, 3N], sum of |K_e| entries, contributions per
    entry (the last two feed the rounding bounds)."""
    n = 3 * N
    A, Aabs, Cnt = (torch.zeros(n * n, dtype=F64) for _ in range(3))
    for K, el in families:
        dm = R.dof_map(el.long(), 3)
        idx = (dm[:, :, None] * n + dm[:, None, :]).reshape(-1)
        v = K.to(F64).reshape(-1)
        A.index_add_(0, idx, v)
        Aabs.index_add_(0, idx, v.abs())
        Cnt.index_add_(0, idx, torch.ones_like(v))
    return A.view(n, n), Aabs.view(n, n), Cnt.view(n, n)


def jacobi_weights(A, fixed):
    w = 1.0 / A.diagonal().clone()
    w = torch.where(torch.isfinite(w), w, torch.zeros_like(w)).view(-1, 3)
    w[fixed] = 0.0
    return w.reshape(-1)


def rcb_aggregates(coords, w, k):
    """`dist.rcb_partition` over the free nodes -> ids [N], -1 elsewhere."""
    free = (w.view(-1, 3) != 0).any(1)
    ids = torch.nonzero(free).view(-1)
    agg = torch.full((coords.shape[0],), -1, dtype=torch.long)
    agg[ids] = dist.rcb_partition(coords[ids], k)
    return agg


class TwoLevelRef:
    def __init__(self, A, coords, w, agg, descending=False, shift=None, Aabs=None, Cnt=None):
        N = coords.shape[0]
        self.N, self.n = N, 3 * N
        perm = torch.arange(N).flip(0) if descending else torch.arange(N)
        self.dp = (3 * perm[:, None] + torch.arange(3)[None, :]).reshape(-1)   # permuted dof -> natural dof
        self.idp = torch.empty_like(self.dp)
        self.idp[self.dp] = torch.arange(self.n)
        A, w = A.to(F64), w.to(F64).reshape(-1)
        self.A = A[self.dp][:, self.dp].contiguous()
        self.w = w[self.dp].contiguous()
        coords, agg = coords.to(F64)[perm], agg.clone().long()[perm]
        free = (self.w.view(N, 3) != 0)
        agg[~free.any(1)] = -1
        sel = agg >= 0
        uniq, inv = torch.unique(agg[sel], return_inverse=True)
        agg[sel] = inv
        self.agg, self.k = agg, int(uniq.numel())
        self.m = 6 * self.k
        k = self.k
        onehot = torch.zeros((N, k), dtype=F64)
        onehot[sel, agg[sel]] = 1.0
        cnt = onehot.sum(0)
        centre = ((onehot.T @ coords) / cnt[:, None]).float().double()   # fp32-rounded, as the package stores them
        ai = agg.clamp(min=0)
        d = torch.where(sel[:, None], coords - centre[ai], torch.zeros_like(coords))
        rho = ((onehot.T @ (d * d)).sum(1) / cnt).sqrt().float().double()
        rho = torch.where(rho > 0, rho, torch.ones_like(rho))
        if shift is not None:   # another centre per aggregate: the same space, another basis of it
            d = torch.where(sel[:, None], coords - (centre + shift.to(F64))[ai], torch.zeros_like(coords))
        rel = d / rho[ai][:, None]
        self.centre, self.rho, self.rel = centre, rho, rel
        x, y, z = rel[:, 0], rel[:, 1], rel[:, 2]
        o, l = torch.zeros_like(x), torch.ones_like(x)
        Rn = torch.stack([torch.stack([l, o, o, o, z, -y], 1), torch.stack([o, l, o, -z, o, x], 1),
                          torch.stack([o, o, l, y, -x, o], 1)], 1)   # [N, 3, 6] = [I | -[rel]x]
        Rn = Rn * (free.to(F64) * sel[:, None].to(F64))[:, :, None]
        Z = torch.zeros((N, 3, k, 6), dtype=F64)
        Z[sel, :, agg[sel], :] = Rn[sel]
        self.Z = Z.reshape(self.n, self.m)
        self.E = self.Z.T @ (self.A @ self.Z)
        G = (self.Z.T @ self.Z).view(k, 6, k, 6)[torch.arange(k), :, torch.arange(k), :]
        lam, V = torch.linalg.eigh(G)
        keep = lam > DROP * lam[:, -1:]
        a_of, q_of = torch.nonzero(keep, as_tuple=True)
        mk = int(a_of.numel())
        T = torch.zeros((self.m, mk), dtype=F64)
        T[(6 * a_of)[:, None] + torch.arange(6)[None, :], torch.arange(mk)[:, None]] = V[a_of, :, q_of]
        self.T, self.dropped = T, self.m - mk
        Es = 0.5 * (self.E + self.E.T)
        Ek = T.T @ Es @ T
        Ik = torch.linalg.inv(0.5 * (Ek + Ek.T))
        Einv = T @ (0.5 * (Ik + Ik.T)) @ T.T
        self.Einv = 0.5 * (Einv + Einv.T)
        self.Aabs = None if Aabs is None else Aabs[self.dp][:, self.dp]
        self.Cnt = None if Cnt is None else Cnt[self.dp][:, self.dp]

    # ------------------------------------------------------------ natural numbering in and out
    def _in(self, v):
        return v.to(F64).reshape(-1)[self.dp]

    def _out(self, v):
        return v[self.idp]

    def restrict(self, r):
        return self.Z.T @ self._in(r)

    def restrict_bound(self, r):
        """terms 2^-52 sum |terms| per entry of Z^T r."""
        nz = (self.Z != 0).to(F64)
        return nz.sum(0) * EPS * (self.Z.abs().T @ self._in(r).abs())

    def E_bound(self):
        """terms 2^-52 sum |terms| per entry of Z^T A Z, the element contributions to A counted as terms."""
        nz = (self.Z != 0).to(F64)
        terms = nz.T @ (self.Cnt @ nz)
        return terms * EPS * (self.Z.abs().T @ (self.Aabs @ self.Z.abs()))

    def _apply(self, r):
        return self.w * r + self.Z @ (self.Einv @ (self.Z.T @ r))

    def apply(self, r):
        return self._out(self._apply(self._in(r)))

    def dense_preconditioner(self):
        """M^-1 on the free dofs (natural numbering) -> [nf, nf]."""
        M = torch.diag(self.w) + self.Z @ self.Einv @ self.Z.T
        f = torch.nonzero(self.w[self.idp] != 0).view(-1)
        return M[self.idp][:, self.idp][f][:, f]

    def pcg(self, b, tol=1e-8, rtol=None, max_iter=1000, jacobi=False, true_rtol=None):
        """The device context's iteration: stop on sqrt(r.z) < tol (rtol: times sqrt(r0.z0)), history of sqrt(r.z),
        p.Ap <= 0 or non-finite -> breakdown. jacobi=True: z = w o r. true_rtol: stop on ||r|| < true_rtol ||b|| over the
        free dofs instead. -> (x natural, iterations, history, status)."""
        prec = (lambda r: self.w * r) if jacobi else self._apply
        b = self._in(b)
        free = (self.w != 0).to(F64)
        x = torch.zeros_like(b)
        r = b.clone()
        z = prec(r)
        p = z.clone()
        rz = float(r @ z)
        if rtol is not None:
            tol = rtol * rz ** 0.5
        hist, status, it = [], "maxiter", 0
        for it in range(1, max_iter + 1):
            q = self.A @ p
            pq = float(p @ q)
            if not pq > 0.0 or pq == float("inf"):
                status = "breakdown"
                break
            al = rz / pq
            x += al * p
            r -= al * q
            z = prec(r)
            rz_new = float(r @ z)
            hist.append(rz_new ** 0.5 if rz_new >= 0 else float("nan"))
            if true_rtol is not None:
                if float((free * r).norm()) < true_rtol * float((free * b).norm()):
                    status = "converged"
                    break
            elif hist[-1] < tol:
                status = "converged"
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
        return self._out(x), it, torch.tensor(hist, dtype=F64), status

    def direct(self, b):
        """Dense direct solve on the free dofs (zeros elsewhere), natural numbering."""
        wn = self.w[self.idp]
        f = torch.nonzero(wn != 0).view(-1)
        An = self.A[self.idp][:, self.idp]
        u = torch.zeros(self.n, dtype=F64)
        u[f] = torch.linalg.solve(An[f][:, f], b.to(F64).reshape(-1)[f])
        return u

    def masked_residual(self, b, x):
        """||b - A x|| over the free dofs, natural numbering."""
        wn = self.w[self.idp]
        An = self.A[self.idp][:, self.idp]
        return float(((b.to(F64).reshape(-1) - An @ x.to(F64).reshape(-1)) * (wn != 0)).norm())
