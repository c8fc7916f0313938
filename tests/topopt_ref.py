"""CPU fp64 restatement of the topology-optimisation path (torch only, dense), written from the formulation of DESIGN
§8t, not from any kernel text: per-element modulus scale, unit strain energy, the node-average density filter and its
adjoint, the SIMP scale and the optimality-criteria update with its geometric bisection.

With the gradients g_a and volume V_e of the reference configuration, lam1 / mu1 the Lame constants at E = 1:
    K(s) = sum_e s_e K_e(E, nu),  K_e = V_e B^T D B
    ce_e = u_e^T K_e(1, nu) u_e = V_e (lam1 tr(eps)^2 + 2 mu1 eps:eps),  eps = sym(sum_a u_a (x) g_a)
    filter   rho_n = (sum_{e at n} V_e rho_e) / Vn_n,  Vn_n = sum_{e at n} V_e,  rho_t_e = 1/4 sum_a rho_n[e_a]
    adjoint  t_n = (1/4 sum_{e at n} g_e) / Vn_n,  out_e = V_e sum_a t[e_a]
    s_e = s_min + (1 - s_min) rho_t_e^p,  c = sum_e s_e E ce_e = u^T K(s) u,
    dc = filter^T (-p (1 - s_min) rho_t^(p-1) E ce)
    OC: b_e = max(0, -dc_e) / V_e, lo_e = max(rho_min, rho_e - move), hi_e = min(1, rho_e + move),
        rho_new_e(l) = min(hi_e, max(lo_e, rho_e sqrt(b_e / l))); bracket [rho_min^2 min_{b>0} b, max b / rho_min^2] over
        the free elements, 60 steps at l_mid = sqrt(l_lo) sqrt(l_hi) (volume above the target: l_lo = l_mid, else
        l_hi = l_mid), the result taken at l_hi; passive elements pinned (1: solid -> 1, -1: void -> rho_min).
The design loop solves K u = F on the free dofs directly, or by its own Jacobi-PCG started from the previous u and
stopped at sqrt(r.z) <= rtol sqrt(F.w F) (the device's rule)."""
import math

import torch

import hyperelastic_ref as HR
from oracle import ref_cpu as R

F64 = torch.float64
N_BISECT = 60


def lame1(nu):
    c = 1.0 / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return c * nu, c * (1.0 - 2.0 * nu) / 2.0


def apex_mesh():
    """kuhn_cube(3, jitter=0.15) plus one node at (0.5, 0.5, 1.5) joined to the 18 triangles of the z = 1 face: the apex
    row has 17 columns, so a bs = 1 pattern leaves the 16-column accumulator configuration."""
    from fem355 import mesh
    c, t = mesh.kuhn_cube(3, jitter=0.15)
    c = c.to(F64)
    top = set(torch.nonzero(c[:, 2] > 1.0 - 1e-9).view(-1).tolist())
    apex = c.shape[0]
    new = []
    for tet in t.tolist():
        on = [n for n in tet if n in top]
        if len(on) == 3:
            new.append(on + [apex])
    assert len(new) == 18, len(new)
    return torch.cat([c, torch.tensor([[0.5, 0.5, 1.5]], dtype=F64)]), torch.cat([t, torch.tensor(new, dtype=t.dtype)])


class Model:
    def __init__(self, coords, tets, E=1.0, nu=0.3):
        self.coords, self.tets = coords.to(F64), tets
        self.N, self.M = coords.shape[0], tets.shape[0]
        self.E, self.nu = float(E), float(nu)
        self.g, self.V = HR.geometry(self.coords, tets)
        self.Vn = torch.zeros(self.N, dtype=F64).index_add_(0, tets.reshape(-1), self.V.repeat_interleave(4))
        self._Ke = {}

    # ------------------------------------------------------------ stiffness
    def element_matrices(self, kind="elastic"):
        """K_e(E, nu) [M,12,12] or the Poisson K_e(kappa = E) [M,4,4], formed once."""
        if kind not in self._Ke:
            if kind == "elastic":
                self._Ke[kind] = R.tet4_K(self.coords, self.tets, self.E, self.nu)
            else:
                self._Ke[kind] = self.E * self.V.view(-1, 1, 1) * torch.einsum("mai,mbi->mab", self.g, self.g)
        return self._Ke[kind]

    def dense(self, s, kind="elastic"):
        """sum_e s_e K_e as a dense [n, n] matrix, n = dpn N."""
        Ke = self.element_matrices(kind) * s.to(F64).view(-1, 1, 1)
        dpn = 3 if kind == "elastic" else 1
        dofs = (self.tets.view(-1, 4, 1) * dpn + torch.arange(dpn)).reshape(self.M, 4 * dpn)
        n = dpn * self.N
        K = torch.zeros(n * n, dtype=F64)
        K.index_add_(0, (dofs.view(self.M, -1, 1) * n + dofs.view(self.M, 1, -1)).reshape(-1), Ke.reshape(-1))
        return K.view(n, n)

    # ------------------------------------------------------------ energy
    def unit_energy(self, u):
        lam, mu = lame1(self.nu)
        H = torch.einsum("mai,maj->mij", u.to(F64).view(self.N, 3)[self.tets], self.g)
        eps = 0.5 * (H + H.transpose(1, 2))
        tr = eps.diagonal(dim1=1, dim2=2).sum(1)
        return self.V * (lam * tr * tr + 2.0 * mu * (eps * eps).sum((1, 2)))

    # ------------------------------------------------------------ filter
    def filter(self, x, passes=1):
        x = x.to(F64).clone()
        for _ in range(passes):
            xn = torch.zeros(self.N, dtype=F64).index_add_(0, self.tets.reshape(-1), (self.V * x).repeat_interleave(4))
            x = 0.25 * (xn / self.Vn)[self.tets].sum(1)
        return x

    def filter_adjoint(self, g, passes=1):
        g = g.to(F64).clone()
        for _ in range(passes):
            t = torch.zeros(self.N, dtype=F64).index_add_(0, self.tets.reshape(-1), g.repeat_interleave(4))
            g = self.V * (0.25 * t / self.Vn)[self.tets].sum(1)
        return g


def simp(rho_t, penal, s_min):
    return s_min + (1.0 - s_min) * rho_t ** penal


def oc_bounds(rho, move, rho_min):
    return torch.clamp(rho - move, min=rho_min), torch.clamp(rho + move, max=1.0)


def oc_density(rho, b, l, move, rho_min, passive=None):
    lo, hi = oc_bounds(rho, move, rho_min)
    new = torch.minimum(hi, torch.maximum(lo, rho * torch.sqrt(b / l)))
    if passive is not None:
        new = torch.where(passive > 0, torch.ones_like(new), new)
        new = torch.where(passive < 0, torch.full_like(new, rho_min), new)
    return new


def oc_bracket(b, rho_min, passive=None):
    """(l_lo, l_hi) over the free elements, or None when no free b_e > 0."""
    bf = b if passive is None else b[passive == 0]
    if bf.numel() == 0 or not bool((bf > 0).any()):
        return None
    return rho_min * rho_min * float(bf[bf > 0].min()), float(bf.max()) / (rho_min * rho_min)


def oc_update(rho, dc, V, volfrac, move, rho_min, passive=None, n_bisect=N_BISECT):
    """-> (rho_new, max |rho_new - rho|, reached volume fraction, (l_lo, l_hi))."""
    rho, V = rho.to(F64), V.to(F64)
    b = torch.clamp(-dc.to(F64), min=0.0) / V
    vtot = float(V.sum())
    br = oc_bracket(b, rho_min, passive)
    if br is None:
        return rho.clone(), 0.0, float((V * rho).sum()) / vtot, None
    lo, hi = br
    target = volfrac * vtot
    for _ in range(n_bisect):
        mid = math.sqrt(lo) * math.sqrt(hi)
        if float((V * oc_density(rho, b, mid, move, rho_min, passive)).sum()) > target:
            lo = mid
        else:
            hi = mid
    new = oc_density(rho, b, hi, move, rho_min, passive)
    return new, float((new - rho).abs().max()), float((V * new).sum()) / vtot, (lo, hi)


def jacobi_pcg(K, b, w, x0, tol, max_iter):
    """Jacobi-PCG from x0, stopped at sqrt(r.z) <= tol -> (x, iterations, converged)."""
    x = x0.clone()
    r = b - K @ x
    z = w * r
    p = z.clone()
    rz = float(r @ z)
    if math.sqrt(max(rz, 0.0)) <= tol:
        return x, 0, True
    for i in range(max_iter):
        Ap = K @ p
        alpha = rz / float(p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = w * r
        rz_new = float(r @ z)
        if math.sqrt(max(rz_new, 0.0)) <= tol:
            return x, i + 1, True
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_iter, False


class Design:
    """The design loop on a Model: compliance, sensitivities and the OC step, with a direct or a PCG linear solve."""

    def __init__(self, model, F, mask, volfrac, penal=3.0, s_min=1e-3, rho_min=1e-3, passes=1, move=0.2, passive=None,
                 linear="direct", linear_rtol=1e-8, linear_max_iter=10000):
        self.m, self.F = model, F.to(F64).reshape(-1)
        self.free = ~mask.reshape(-1)
        self.volfrac, self.penal, self.s_min, self.rho_min = volfrac, penal, s_min, rho_min
        self.passes, self.move, self.passive = passes, move, passive
        self.linear, self.rtol, self.max_it = linear, linear_rtol, linear_max_iter
        self.x = torch.zeros(3 * model.N, dtype=F64)
        self.pcg_iterations = []

    def solve(self, s):
        K = self.m.dense(s)
        if self.linear == "direct":
            u = torch.zeros(3 * self.m.N, dtype=F64)
            u[self.free] = torch.linalg.solve(K[self.free][:, self.free], self.F[self.free])
            return u
        w = torch.where(self.free, 1.0 / K.diagonal(), torch.zeros(1, dtype=F64))
        bn = math.sqrt(float(self.F @ (w * self.F)))
        self.x, it, ok = jacobi_pcg(K, self.F, w, self.x, self.rtol * bn, self.max_it)
        self.pcg_iterations.append(it)
        if not ok:
            raise RuntimeError("topopt_ref: the PCG did not converge")
        return self.x.clone()

    def compliance(self, rho):
        """(c, dc, rho_t, s, u) at the design rho."""
        rho_t = self.m.filter(rho, self.passes)
        s = simp(rho_t, self.penal, self.s_min)
        u = self.solve(s)
        ce = self.m.unit_energy(u)
        c = float((s * self.m.E * ce).sum())
        dct = -self.penal * (1.0 - self.s_min) * rho_t ** (self.penal - 1.0) * self.m.E * ce
        return c, self.m.filter_adjoint(dct, self.passes), rho_t, s, u

    def run(self, rho, iterations):
        """`iterations` design steps from rho -> dict of the histories and the final density."""
        rho = rho.to(F64).clone()
        h = {"compliance": [], "load_work": [], "volume_fraction": [], "change": [], "density": None}
        for _ in range(iterations):
            c, dc, _, _, u = self.compliance(rho)
            rho, ch, vf, _ = oc_update(rho, dc, self.m.V, self.volfrac, self.move, self.rho_min, self.passive)
            h["compliance"].append(c)
            h["load_work"].append(float(self.F @ u))
            h["volume_fraction"].append(vf)
            h["change"].append(ch)
        h["density"] = rho
        return h


def cantilever(coords):
    """The optimisation case: x = 0 face fixed ([N,3] bool mask), a unit load in -z spread over the nodes of the edge
    x = 1, z = 0 -> (F [N,3], mask)."""
    c = coords.to(F64)
    mask = torch.zeros(c.shape[0], 3, dtype=torch.bool)
    mask[c[:, 0] < 1e-9] = True
    edge = (c[:, 0] > 1.0 - 1e-9) & (c[:, 2] < 1e-9)
    F = torch.zeros(c.shape[0], 3, dtype=F64)
    F[edge, 2] = -1.0 / int(edge.sum())
    return F, mask
