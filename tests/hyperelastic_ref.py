"""CPU fp64 oracle of the nonlinear c3d4 path (torch only), written from the formulation, not from any kernel text:
total-Lagrangian c3d4 with constant F = I + sum_a u_a (x) g_a per element and the strain energies
    svk          W = lam/2 (tr E)^2 + mu E:E,  E = (F^T F - I)/2
    neo_hookean  W = mu/2 (F:F - 3) - mu ln J + lam/2 (ln J)^2
Everything else is derived from the energy by autograd: the internal force is the gradient of the total energy, the
element tangent the Hessian of the element energy in its 12 dofs, the global tangent the sum of the element Hessians
(the Hessian of the total energy), the Cauchy stress J^-1 (dW/dF) F^T. The energies are evaluated from H = F - I
(E = (H + H^T + H^T H)/2, F:F - 3 = 2 tr H + H:H): the same functions, without the cancellation at small strains.

A dense Newton with the load stepping, stop rule and line search of solver.nonlinear_static_solver, with a direct
linear solve on the free dofs or with a Jacobi-PCG (oracle.ref_cpu.pcg on the dense tangent) at the same linear_rtol."""
import torch

import modal_ref as MR
from oracle import ref_cpu as R

F64 = torch.float64
MATERIALS = ("svk", "neo_hookean")
LS_HALVINGS, LS_C1 = 10, 1e-4


def lame(E, nu):
    c = E / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return c * nu, c * ((1.0 - 2.0 * nu) / 2.0)


def geometry(coords, tets):
    """(gradients [M,4,3], volumes [M]) of the reference configuration."""
    return R.tet4_gradients(coords.to(F64), tets), R.tet_volumes(coords.to(F64), tets)


def density_from_H(H, lam, mu, material):
    """W [M] from H = F - I [M,3,3]."""
    if material == "svk":
        Eg = 0.5 * (H + H.transpose(1, 2) + H.transpose(1, 2) @ H)
        tr = Eg.diagonal(dim1=1, dim2=2).sum(1)
        return 0.5 * lam * tr * tr + mu * (Eg * Eg).sum((1, 2))
    if material == "neo_hookean":
        Fm = torch.eye(3, dtype=F64) + H
        lnJ = torch.log(torch.det(Fm))
        return 0.5 * mu * (2.0 * H.diagonal(dim1=1, dim2=2).sum(1) + (H * H).sum((1, 2))) - mu * lnJ + 0.5 * lam * lnJ * lnJ
    raise ValueError(material)


def element_energy(ue, g, V, lam, mu, material):
    """V W [M] from the element displacements ue [M,4,3]."""
    return V * density_from_H(torch.einsum("mai,maj->mij", ue, g), lam, mu, material)


class Model:
    """One mesh + material: energies, forces, tangents, stresses at a displacement u [N,3]."""

    def __init__(self, coords, tets, E, nu, material):
        self.coords, self.tets, self.material = coords.to(F64), tets, material
        self.N, self.M = coords.shape[0], tets.shape[0]
        self.lam, self.mu = lame(E, nu)
        self.g, self.V = geometry(coords, tets)

    def deformation(self, u):
        Fm = torch.eye(3, dtype=F64) + torch.einsum("mai,maj->mij", u.to(F64)[self.tets], self.g)
        return Fm, torch.det(Fm)

    def energies(self, u):
        return element_energy(u.to(F64)[self.tets], self.g, self.V, self.lam, self.mu, self.material)

    def f_int(self, u):
        u = u.detach().to(F64).clone().requires_grad_(True)
        return torch.autograd.grad(self.energies(u).sum(), u)[0]

    def element_forces_tangents(self, u):
        """(fe [M,4,3], Kt [M,12,12]) = gradient and Hessian of every element's energy in its own 12 dofs."""
        ue = u.detach().to(F64)[self.tets].clone().requires_grad_(True)
        w = element_energy(ue, self.g, self.V, self.lam, self.mu, self.material)
        fe = torch.autograd.grad(w.sum(), ue, create_graph=True)[0]
        flat = fe.reshape(self.M, 12)
        rows = [torch.autograd.grad(flat[:, j].sum(), ue, retain_graph=True)[0].reshape(self.M, 12) for j in range(12)]
        return fe.detach(), torch.stack(rows, dim=1)

    def dense_tangent(self, u):
        return MR.dense(self.element_forces_tangents(u)[1], self.tets, self.N, 3)

    def cauchy(self, u):
        """Voigt [M,6] (xx, yy, zz, xy, yz, xz) of J^-1 (dW/dF) F^T."""
        H = torch.einsum("mai,maj->mij", u.detach().to(F64)[self.tets], self.g).clone().requires_grad_(True)
        P = torch.autograd.grad(density_from_H(H, self.lam, self.mu, self.material).sum(), H)[0]
        Fm = torch.eye(3, dtype=F64) + H.detach()
        s = P @ Fm.transpose(1, 2) / torch.det(Fm).view(-1, 1, 1)
        return torch.stack((s[:, 0, 0], s[:, 1, 1], s[:, 2, 2], s[:, 0, 1], s[:, 1, 2], s[:, 0, 2]), dim=1)


def closed_form_tangent(model, u):
    """The closed-form blocks of the formulation, evaluated in torch -> [M,12,12]."""
    g, V, lam, mu = model.g, model.V, model.lam, model.mu
    Fm, J = model.deformation(u)
    I3 = torch.eye(3, dtype=F64)
    gg = torch.einsum("maj,mbj->mab", g, g)
    if model.material == "svk":
        Eg = 0.5 * (Fm.transpose(1, 2) @ Fm - I3)
        S = lam * Eg.diagonal(dim1=1, dim2=2).sum(1).view(-1, 1, 1) * I3 + 2.0 * mu * Eg
        Fg = torch.einsum("mij,maj->mai", Fm, g)
        c = torch.einsum("mai,mij,mbj->mab", g, S, g)
        FFt = Fm @ Fm.transpose(1, 2)
        K = (torch.einsum("mab,ik->maibk", c, I3) + lam * torch.einsum("mai,mbk->maibk", Fg, Fg)
             + mu * torch.einsum("mbi,mak->maibk", Fg, Fg) + mu * torch.einsum("mab,mik->maibk", gg, FFt))
    else:
        h = torch.einsum("mji,maj->mai", torch.linalg.inv(Fm), g)   # F^-T g_a
        lnJ = torch.log(J).view(-1, 1, 1, 1, 1)
        K = (mu * torch.einsum("mab,ik->maibk", gg, I3) + (mu - lam * lnJ) * torch.einsum("mbi,mak->maibk", h, h)
             + lam * torch.einsum("mai,mbk->maibk", h, h))
    return (K * V.view(-1, 1, 1, 1, 1)).reshape(model.M, 12, 12)


# ---------------------------------------------------------------- displacement fields and load cases of the tests
def rotation(angle=0.7):
    ax = torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    ax = ax / ax.norm()
    Kx = torch.tensor([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]], dtype=F64)
    return torch.eye(3, dtype=F64) + torch.sin(torch.tensor(angle, dtype=F64)) * Kx + \
        (1.0 - torch.cos(torch.tensor(angle, dtype=F64))) * (Kx @ Kx)


def field(name, coords, n):
    """The displacement fields of the element tests on a mesh of n cells per edge."""
    c = coords.to(F64)
    if name == "zero":
        return torch.zeros_like(c)
    if name == "random":
        return (0.1 / n) * (2.0 * torch.rand(c.shape, dtype=F64, generator=torch.Generator().manual_seed(7)) - 1.0)
    if name == "rigid":
        return c @ rotation().T - c + torch.tensor([0.3, -0.2, 0.1], dtype=F64) * c.abs().max()
    if name == "stretch":
        return torch.stack((0.2 * c[:, 0], -0.05 * c[:, 1], torch.zeros_like(c[:, 2])), dim=1)
    raise ValueError(name)


SOLVER_CASES = {"pull": (0.0, 0.0, 0.15), "shear": (0.04, 0.0, 0.0), "push": (0.0, 0.0, -0.08)}


def solver_case(coords, name, scale=1.0):
    """(F [N,3], fixed node ids): the z = 0 face fixed, the total top-face force spread evenly over the top nodes."""
    c = coords.to(F64)
    z = c[:, 2]
    fixed = torch.nonzero(z == z.min()).reshape(-1)
    top = torch.nonzero(z == z.max()).reshape(-1)
    F = torch.zeros_like(c)
    F[top] = scale * torch.tensor(SOLVER_CASES[name], dtype=F64) / top.numel()
    return F, fixed


# ---------------------------------------------------------------- dense Newton restatement
def newton(model, F, fixed, load_steps=1, tol=1e-8, atol=0.0, max_iter=25, linear="direct", linear_rtol=1e-6,
           linear_max_iter=10000, u_init=None):
    """Load-stepped Newton with the stop rule and line search of nonlinear_static_solver. linear: "direct" or "pcg".
    Returns (u [N,3], info) with info = dict(converged, iterations [per step: linear solves], alphas, min_detF, peak)."""
    N = model.N
    free = torch.ones(3 * N, dtype=torch.bool)
    free.view(N, 3)[fixed] = False
    Fv = F.to(F64).reshape(-1)
    stop = max(tol * float(Fv[free].norm()), atol)
    u = torch.zeros(3 * N, dtype=F64) if u_init is None else u_init.to(F64).reshape(-1).clone()
    u[~free] = 0.0
    info = {"converged": False, "iterations": [], "alphas": [], "min_detF": float("inf"), "pcg_iterations": []}

    def evaluate(v, lf):
        r = lf * Fv - model.f_int(v.view(N, 3)).reshape(-1)
        r[~free] = 0.0
        detF = model.deformation(v.view(N, 3))[1]
        inverted = bool((detF <= 0).any())
        en = float("inf") if inverted else float(model.energies(v.view(N, 3)).sum())
        return r, en - lf * float(Fv @ v), float(r.norm()), inverted, float(detF.min())

    for s in range(1, load_steps + 1):
        lf = s / load_steps
        its, done = 0, False
        for k in range(1, max_iter + 1):
            r, pot, rn, _, dmin = evaluate(u, lf)
            if rn <= stop:
                done = True
                info["min_detF"] = min(info["min_detF"], dmin)
                break
            K = model.dense_tangent(u.view(N, 3))
            w = torch.where(free, 1.0 / K.diagonal(), torch.zeros(3 * N, dtype=F64))
            w[torch.isinf(w)] = 0.0
            delta = torch.zeros(3 * N, dtype=F64)
            if linear == "direct":
                delta[free] = torch.linalg.solve(K[free][:, free], r[free])
            else:
                bn = float(torch.sqrt(r @ (w * r)))
                delta, pit, _ = R.pcg(None, None, r, w, tol=linear_rtol * bn, max_iter=linear_max_iter,
                                      matvec=lambda v: K @ v)
                info["pcg_iterations"].append(pit)
            slope = float(r @ delta)
            if not slope > 0.0:
                delta = w * r
                slope = float(r @ delta)
            alpha, ok = 1.0, False
            for _ in range(LS_HALVINGS + 1):
                ut = u + alpha * delta
                _, pot_t, rn_t, inv_t, _ = evaluate(ut, lf)
                if not inv_t and (pot_t <= pot - LS_C1 * alpha * slope or rn_t < rn):
                    ok = True
                    break
                alpha *= 0.5
            if not ok:
                info["iterations"].append(its)
                return u.view(N, 3), info
            u = ut
            its += 1
            info["alphas"].append(alpha)
        info["iterations"].append(its)
        if not done:
            return u.view(N, 3), info
    info["converged"] = True
    info["peak"] = float(u.abs().max())
    return u.view(N, 3), info
