"""Restatement of the geometric multigrid PCG (host, fp64) on `oracle.ref_cpu`'s element matrices: uniform refinement
of c3d4 meshes with `parents`, the prolongation P from `parents`, the Chebyshev-Jacobi smoother, the V-cycle, PCG with
the device context's semantics and a direct solve. Nothing here is shared with the package's code. Vectors go in and
out as torch tensors; the level matrices and P are scipy CSR (the pattern of twolevel_ref.py is dense torch, which at
the 16-cube's 14,739 dofs would take 1.7 GB and minutes), `.toarray()` gives the dense forms the small tests need.

`descending=True` evaluates everything under the reversed node numbering of every level (so every row sum, every
restriction sum and the assembly's sums run in the opposite order) and maps results back: the spread between the two
is what summation order alone does to a result, the unit of the device tests' tolerances."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import ref_cpu as R

F64 = torch.float64
EPS = 2.0 ** -52
E_MOD, NU = 113.8e9, 0.342   # tests/modal_ref.py's material
WALK = [(0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3)]   # the edges of c3d10 nodes 4 .. 9
CHILDREN = [[0, 4, 6, 7], [4, 1, 5, 8], [6, 5, 2, 9], [7, 8, 9, 3], [4, 6, 7, 5], [6, 7, 9, 5], [4, 7, 8, 5],
            [5, 8, 7, 9]]   # corner tets, then the octahedron cut along mid(1,2) - mid(0,3) (nodes 5 and 7)


def split_table():
    """CHILDREN with every child oriented like the parent (checked on the unit tet; last two nodes swapped if not)."""
    c = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    x = np.concatenate([c, np.array([0.5 * (c[a] + c[b]) for a, b in WALK])])
    tab = [list(r) for r in CHILDREN]
    for row in tab:
        p = x[row]
        if np.linalg.det(p[1:] - p[0]) < 0:
            row[2], row[3] = row[3], row[2]
    return tab


def tet_volumes(coords, tets):
    """Signed volumes det[x1 - x0, x2 - x0, x3 - x0] / 6."""
    p = coords.to(F64)[tets.long()]
    return torch.linalg.det(p[:, 1:] - p[:, :1]) / 6.0


def elevate_ref(coords, tets, first_encounter):
    """c3d4 -> c3d10: (coords [N + E, 3], c3d10 connectivity [M, 10], unique edges [E, 2], mid_id [E]). Mid nodes follow
    the corners in the order of the sorted unique edges, or of the first slot 6 e + k (WALK) that names the edge."""
    X, t = coords.to(F64), tets.long()
    N, M = X.shape[0], t.shape[0]
    ea = torch.stack([t[:, a] for a, _ in WALK], 1).reshape(-1)
    eb = torch.stack([t[:, b] for _, b in WALK], 1).reshape(-1)
    lo, hi = torch.minimum(ea, eb), torch.maximum(ea, eb)
    key = lo * N + hi
    uniq, inv = torch.unique(key, return_inverse=True)
    E = uniq.numel()
    ue = torch.stack([uniq // N, uniq % N], 1)
    mid_id = torch.arange(E)
    if first_encounter:
        first = torch.full((E,), 6 * M, dtype=torch.long)
        first.scatter_reduce_(0, inv, torch.arange(6 * M), reduce="amin")
        mid_id = torch.empty(E, dtype=torch.long)
        mid_id[torch.argsort(first)] = torch.arange(E)
    Xo = torch.empty((N + E, 3), dtype=F64)
    Xo[:N] = X
    Xo[N + mid_id] = 0.5 * (X[ue[:, 0]] + X[ue[:, 1]])
    el10 = torch.cat([t, (N + mid_id[inv]).view(M, 6)], 1)
    return Xo, el10, ue, mid_id


def refine_ref(coords, tets):
    """One uniform refinement in the numbering of reorder=None: (coords, tets [8 M, 4], parents [N + E, 2])."""
    N = coords.shape[0]
    Xo, el10, ue, _ = elevate_ref(coords, tets, False)
    fine = el10[:, torch.tensor(split_table())].reshape(-1, 4)
    parents = torch.cat([torch.arange(N)[:, None].expand(N, 2), ue], 0)
    return Xo, fine.contiguous(), parents.contiguous()


def hierarchy_ref(coords, tets, levels):
    """[(coords, tets, parents or None)] for `levels` refinements, numbering of reorder=None."""
    out = [(coords.to(F64), tets.long(), None)]
    for _ in range(levels):
        c, t, p = refine_ref(out[-1][0], out[-1][1])
        out.append((c, t, p))
    return out


def carry_ref(ids, hier, level):
    inside = torch.zeros(hier[0][0].shape[0], dtype=torch.bool)
    inside[ids] = True
    for _, _, p in hier[1:level + 1]:
        inside = inside[p[:, 0].long()] & inside[p[:, 1].long()]
    return torch.nonzero(inside).view(-1)


def element_matrices(coords, tets, kind, E, nu):
    return R.tet4_K(coords, tets, E, nu) if kind == "elastic" else R.tet4_poisson_K(coords, tets, E)


def sparse_matrix(K, tets, N, bs, absolute=False):
    """CSR [bs N, bs N] of the element matrices (duplicates summed by scipy in a fixed order)."""
    dm = R.dof_map(tets.long(), bs).numpy()
    rows = np.repeat(dm[:, :, None], dm.shape[1], 2).reshape(-1)
    cols = np.repeat(dm[:, None, :], dm.shape[1], 1).reshape(-1)
    v = K.to(F64).reshape(-1).numpy()
    return sp.coo_matrix((np.abs(v) if absolute else v, (rows, cols)), shape=(bs * N, bs * N)).tocsr()


def prolongation(parents, Nc, bs):
    """CSR P [bs Nf, bs Nc]: x_f[i] = 0.5 (x_c[a] + x_c[b]) per component."""
    p = parents.long().numpy()
    Nf = p.shape[0]
    i = np.repeat(np.arange(Nf), 2)
    P1 = sp.coo_matrix((np.full(2 * Nf, 0.5), (i, p.reshape(-1))), shape=(Nf, Nc)).tocsr()
    return sp.kron(P1, sp.identity(bs), format="csr") if bs > 1 else P1


def power_start(n):
    i = np.arange(n, dtype=np.int64)
    return ((i * 2654435761) % 4294967296).astype(np.float64) / 4294967296.0 - 0.5


def chebyshev_scalars(lmax, degree, boost, ratio):
    hi = lmax * boost
    lo = hi / ratio
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [0.0], [1.0 / theta]
    for _ in range(1, degree):
        rn = 1.0 / (2.0 * sigma - rho)
        c1.append(rn * rho)
        c2.append(2.0 * rn / delta)
        rho = rn
    return c1, c2


class MultigridRef:
    """levels: [(coords, tets, parents or None)] coarsest first; fixed: bool mask [N_fine] of the finest level's fixed
    nodes. lmax_scale multiplies every level's power-iteration estimate (0.5: the deliberately halved lmax)."""

    def __init__(self, levels, kind="elastic", E=E_MOD, nu=NU, fixed=None, degree=2, eig_iters=10, boost=1.1,
                 ratio=30.0, descending=False, lmax_scale=1.0, matrices=None):
        self.bs = bs = 1 if kind == "poisson" else 3
        self.degree, self.descending = degree, descending
        L = len(levels)
        self.N = [int(c.shape[0]) for c, _, _ in levels]
        Nf = self.N[-1]
        fixed = torch.zeros(Nf, dtype=torch.bool) if fixed is None else fixed.bool().clone()
        masks = [None] * L
        masks[-1] = fixed
        for l in range(L - 1, 0, -1):
            p = levels[l][2].long()
            carried = p[:, 0] == p[:, 1]
            m = torch.zeros(self.N[l - 1], dtype=torch.bool)
            m[p[carried, 0]] = masks[l][carried]
            masks[l - 1] = m
        self.A, self.w, self.free, self.P, self.lmax, self.c1, self.c2 = [], [], [], [None], [None], [None], [None]
        self.child = [None]
        for l, (c, t, p) in enumerate(levels):
            N = self.N[l]
            t = t.long()
            fx = masks[l]
            if descending:   # node i -> N - 1 - i on every level; the element order stays
                c, t, fx = c.flip(0), N - 1 - t, fx.flip(0)
                if p is not None:
                    p = (self.N[l - 1] - 1 - p.long()).flip(0)
            K = matrices[l] if matrices is not None else element_matrices(levels[l][0], levels[l][1], kind, E, nu)
            A = sparse_matrix(K, t, N, bs)
            d = A.diagonal()
            with np.errstate(divide="ignore"):
                w = np.where(d != 0, 1.0 / d, 0.0)
            w = np.where(np.isfinite(w), w, 0.0).reshape(N, bs)
            w[fx.numpy()] = 0.0
            self.A.append(A)
            self.w.append(w.reshape(-1))
            self.free.append(self.w[-1] != 0)
            if l > 0:
                self.P.append(prolongation(p, self.N[l - 1], bs))
                self.child.append(self._child_table(p, self.N[l - 1]))
                lm = self._lmax(l, eig_iters) * lmax_scale
                self.lmax.append(lm)
                a, b = chebyshev_scalars(lm, degree, boost, ratio)
                self.c1.append(a)
                self.c2.append(b)
        f = np.nonzero(self.free[0])[0]
        A0 = self.A[0].toarray()
        Aff = A0[np.ix_(f, f)]
        I = np.linalg.inv(0.5 * (Aff + Aff.T))
        self.Einv = np.zeros_like(A0)
        self.Einv[np.ix_(f, f)] = 0.5 * (I + I.T)
        self.masks = masks

    # ------------------------------------------------------------ natural numbering in and out (finest level)
    def _flip(self, v, l):
        return v.reshape(self.N[l], self.bs)[::-1].reshape(-1).copy() if self.descending else v

    def _in(self, v, l=-1):
        l = l % len(self.N)
        return self._flip(v.to(F64).reshape(-1).numpy().copy(), l)

    def _out(self, v, l=-1):
        l = l % len(self.N)
        return torch.from_numpy(self._flip(np.asarray(v, dtype=np.float64), l).copy())

    def _lmax(self, l, iters):
        A, w = self.A[l], self.w[l]
        x = self._flip(power_start(A.shape[0]), l) * self.free[l]
        x = x / np.sqrt((x * x).sum())
        lam = 0.0
        for _ in range(iters):
            y = w * (A @ x)
            lam = float((x * y).sum())
            x = y / np.sqrt((y * y).sum())
        return lam

    # ------------------------------------------------------------ transfers (level l - 1 <-> l), natural numbering
    def prolong(self, l, xc, xf=None):
        e = self.free[l] * (self.P[l] @ self._in(xc, l - 1))
        return self._out(e if xf is None else self._in(xf, l) + e, l)

    def _child_table(self, p, Nc):
        """[Nc, K] the nodes of the fine level that name coarse node c, ascending, once per occurrence (a carried node
        twice), padded with -1: the order in which the restriction sums."""
        flat = p.long().numpy().reshape(-1)
        order = np.argsort(flat, kind="stable")
        counts = np.bincount(flat, minlength=Nc)
        start = np.concatenate([[0], np.cumsum(counts)])[:-1]
        sc = flat[order]
        tab = np.full((Nc, int(counts.max())), -1, dtype=np.int64)
        tab[sc, np.arange(flat.size) - start[sc]] = order // 2
        return tab

    def _restrict(self, l, r):
        """P^T (mask o r): every coarse node adds 0.5 r_f over its child list in list order, one term per occurrence --
        the sum as the kernel forms it (a merged P^T would add a carried node's two halves as one term)."""
        tab, bs = self.child[l], self.bs
        mr = (self.free[l] * r).reshape(-1, bs)
        s = np.zeros((tab.shape[0], bs))
        for k in range(tab.shape[1]):
            c = tab[:, k]
            ok = c >= 0
            s[ok] = s[ok] + 0.5 * mr[c[ok]]
        return s.reshape(-1)

    def restrict(self, l, rf):
        return self._out(self._restrict(l, self._in(rf, l)), l - 1)

    def restrict_bound(self, l, rf):
        """2^-52 sum |terms| per entry of P^T (mask o r)."""
        return self._out(EPS * (abs(self.P[l]).T @ (self.free[l] * np.abs(self._in(rf, l)))), l - 1)

    # ------------------------------------------------------------ the cycle
    def _v(self, l, r):
        if l == 0:
            return self.Einv @ r
        A, w, c1, c2, deg = self.A[l], self.w[l], self.c1[l], self.c2[l], self.degree
        r = r.copy()
        d = c2[0] * (w * r)
        x = d.copy()
        for k in range(1, deg):
            r = r - A @ d
            d = c1[k] * d + c2[k] * (w * r)
            x = x + d
        r = r - A @ d
        xc = self._v(l - 1, self._restrict(l, r))
        d = self.free[l] * (self.P[l] @ xc)
        x = x + d
        for k in range(deg):
            r = r - A @ d
            d = c1[k] * d + c2[k] * (w * r)
            x = x + d
        return x

    def _apply(self, r):
        return self._v(len(self.N) - 1, r)

    def apply(self, r):
        return self._out(self._apply(self._in(r)))

    def dense_preconditioner(self):
        """M^-1 on the free dofs of the finest level (natural numbering) -> [nf, nf] torch."""
        n = self.A[-1].shape[0]
        fr = torch.nonzero(self._out(self.free[-1].astype(np.float64)) != 0).view(-1)
        cols = []
        for j in fr.tolist():
            e = torch.zeros(n, dtype=F64)
            e[j] = 1.0
            cols.append(self.apply(e)[fr])
        return torch.stack(cols, 1)

    def pcg(self, b, tol=1e-8, rtol=None, max_iter=1000, jacobi=False):
        """The device context's iteration: stop on sqrt(r.z) < tol (rtol: times sqrt(r0.z0)), history of sqrt(r.z),
        breakdown on p.Ap <= 0 or non-finite and on r.z <= 0 or non-finite. -> (x natural, iterations, history,
        status)."""
        A, w = self.A[-1], self.w[-1]
        prec = (lambda r: w * r) if jacobi else self._apply
        b = self._in(b)
        x = np.zeros_like(b)
        r = b.copy()
        z = prec(r)
        p = z.copy()
        rz = float(r @ z)
        if not rz >= 0.0 or rz == float("inf"):
            return self._out(x), 1, torch.zeros(0, dtype=F64), "breakdown"   # iteration 1 cannot start
        if rz == 0.0:   # nothing to do (b = A x0 on the free dofs): converged before the first iteration
            return self._out(x), 0, torch.zeros(0, dtype=F64), "converged"
        if rtol is not None:
            tol = rtol * rz ** 0.5
        hist, status, it = [], "maxiter", 0
        for it in range(1, max_iter + 1):
            q = A @ p
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
            if rz_new >= 0 and hist[-1] < tol:
                status = "converged"
                break
            if not rz_new > 0.0 or rz_new == float("inf"):
                status = "breakdown"
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
        return self._out(x), it, torch.tensor(hist, dtype=F64), status

    def direct(self, b):
        """Sparse direct solve on the free dofs of the finest level (zeros elsewhere), natural numbering."""
        f = np.nonzero(self.free[-1])[0]
        u = np.zeros(self.A[-1].shape[0])
        u[f] = spla.spsolve(self.A[-1][f][:, f].tocsc(), self._in(b)[f])
        return self._out(u)

    def masked_residual(self, b, x):
        r = (self._in(b) - self.A[-1] @ self._in(x)) * self.free[-1]
        return float(np.sqrt((r * r).sum()))
