"""CPU fp64 restatement of the elastoplastic c3d4 path (torch only), written from the formulation, not from any kernel
text: small-strain von Mises (J2) plasticity with linear isotropic hardening, one integration point per tet.

With the gradients g_a and volume V of the reference configuration, eps = sym(sum_a u_a (x) g_a), mu = E / (2 (1 + nu)),
kappa = E / (3 (1 - 2 nu)); tensors are 3x3 here and (xx, yy, zz, xy, yz, xz) tensor components where they are stored:
    e = dev eps, s_tr = 2 mu (e - ep_n), q_tr = sqrt(3/2) |s_tr|, f_tr = q_tr - (sigma_y + H alpha_n)
    f_tr <= 0: s = s_tr, state kept;  f_tr > 0: dgamma = f_tr / (3 mu + H), n = s_tr / |s_tr|,
    beta = 1 - 3 mu dgamma / q_tr, s = beta s_tr, ep_n+1 = ep_n + sqrt(3/2) dgamma n, alpha_n+1 = alpha_n + dgamma
    sigma = kappa tr(eps) 1 + s;  C = kappa 1(x)1 + 2 mu beta P_dev - 2 mu (3 mu / (3 mu + H) - (1 - beta)) n(x)n
    we = V [kappa/2 tr(eps)^2 + mu |e - ep_n+1|^2 + H/2 alpha_n+1^2 + sigma_y dgamma]
The update is written once on the strain (`update`), so that the stress, the closed-form tangent and the potential can
be differentiated against each other (tests/test_plasticity_cpu.py). A dense Newton over a load path with the stop rule
and line search of solver.elastoplastic_static_solver follows, with a direct linear solve on the free dofs or a
Jacobi-PCG (oracle.ref_cpu.pcg on the dense tangent) at the device's linear_rtol."""
import math

import torch

import hyperelastic_ref as HR
import modal_ref as MR
from oracle import ref_cpu as R

F64 = torch.float64
LS_HALVINGS, LS_C1, LS_POT_ROUND = 10, 1e-4, 1e-13
I3 = torch.eye(3, dtype=F64)
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))


def to_voigt(T):
    """[M,3,3] symmetric -> [M,6] tensor components (xx, yy, zz, xy, yz, xz)."""
    return torch.stack([T[:, i, j] for i, j in VOIGT], dim=1)


def from_voigt(v):
    T = torch.zeros(v.shape[0], 3, 3, dtype=F64)
    for t, (i, j) in enumerate(VOIGT):
        T[:, i, j] = v[:, t]
        T[:, j, i] = v[:, t]
    return T


def moduli(E, nu):
    return E / (2.0 * (1.0 + nu)), E / (3.0 * (1.0 - 2.0 * nu))


def virgin(M):
    return torch.zeros(M, 6, dtype=F64), torch.zeros(M, dtype=F64)


def update(eps, ep_n, alpha_n, mu, kappa, sigma_y, H):
    """The radial return on strains eps [M,3,3] from the committed (ep_n [M,3,3], alpha_n [M]) -> dict of sigma, s, ep,
    alpha, dgamma, n, beta, f_tr, plastic and the potential density w (all per element; differentiable in eps)."""
    tr = eps.diagonal(dim1=1, dim2=2).sum(1)
    e = eps - (tr / 3.0).view(-1, 1, 1) * I3
    s_tr = 2.0 * mu * (e - ep_n)
    sn = torch.sqrt((s_tr * s_tr).sum((1, 2)))
    q_tr = math.sqrt(1.5) * sn
    f_tr = q_tr - (sigma_y + H * alpha_n)
    plastic = f_tr > 0
    safe_sn = torch.where(plastic, sn, torch.ones_like(sn))
    safe_q = torch.where(plastic, q_tr, torch.ones_like(q_tr))
    dgamma = torch.where(plastic, f_tr / (3.0 * mu + H), torch.zeros_like(f_tr))
    n = torch.where(plastic.view(-1, 1, 1), s_tr / safe_sn.view(-1, 1, 1), torch.zeros_like(s_tr))
    beta = 1.0 - 3.0 * mu * dgamma / safe_q
    s = beta.view(-1, 1, 1) * s_tr
    ep = ep_n + math.sqrt(1.5) * dgamma.view(-1, 1, 1) * n
    alpha = alpha_n + dgamma
    sigma = (kappa * tr).view(-1, 1, 1) * I3 + s
    d = e - ep
    w = 0.5 * kappa * tr * tr + mu * (d * d).sum((1, 2)) + 0.5 * H * alpha * alpha + sigma_y * dgamma
    return dict(sigma=sigma, s=s, ep=ep, alpha=alpha, dgamma=dgamma, n=n, beta=beta, f_tr=f_tr, plastic=plastic, w=w)


def tangent_moduli(out, mu, kappa, H):
    """The consistent tangent C [M,3,3,3,3] of an `update` result."""
    M = out["beta"].shape[0]
    dd = torch.einsum("ij,kl->ijkl", I3, I3)
    sym = 0.5 * (torch.einsum("ik,jl->ijkl", I3, I3) + torch.einsum("il,jk->ijkl", I3, I3))
    pdev = sym - dd / 3.0
    beta = out["beta"].view(M, 1, 1, 1, 1)
    cn = torch.where(out["plastic"], 2.0 * mu * (3.0 * mu / (3.0 * mu + H) - (1.0 - out["beta"])),
                     torch.zeros(M, dtype=F64)).view(M, 1, 1, 1, 1)
    return kappa * dd + 2.0 * mu * beta * pdev - cn * torch.einsum("mij,mkl->mijkl", out["n"], out["n"])


class Model:
    """One mesh + material: the element update, forces, tangents and potentials at a displacement u [N,3] from a
    committed state (ep [M,6], alpha [M]); None is the virgin state."""

    def __init__(self, coords, tets, E, nu, sigma_y, H):
        self.coords, self.tets = coords.to(F64), tets
        self.N, self.M = coords.shape[0], tets.shape[0]
        self.E, self.nu, self.sigma_y, self.H = float(E), float(nu), float(sigma_y), float(H)
        self.mu, self.kappa = moduli(self.E, self.nu)
        self.g, self.V = HR.geometry(coords, tets)

    def strain_of(self, ue):
        Hm = torch.einsum("mai,maj->mij", ue, self.g)
        return 0.5 * (Hm + Hm.transpose(1, 2))

    def strain(self, u):
        return self.strain_of(u.to(F64)[self.tets])

    def _state(self, state):
        ep, al = virgin(self.M) if state is None else state
        return from_voigt(ep.to(F64)), al.to(F64)

    def update(self, u, state=None):
        ep_n, al_n = self._state(state)
        return update(self.strain(u), ep_n, al_n, self.mu, self.kappa, self.sigma_y, self.H)

    def element(self, u, state=None, tangent=True):
        """dict of Kt [M,12,12] (closed form), fe [M,4,3], we [M], sigma [M,6], ep [M,6], alpha [M], plastic [M] bool,
        f_tr [M]: the outputs of one fem_tet4_j2 launch."""
        o = self.update(u, state)
        V = self.V
        res = dict(fe=V.view(-1, 1, 1) * torch.einsum("mij,maj->mai", o["sigma"], self.g), we=V * o["w"],
                   sigma=to_voigt(o["sigma"]), ep=to_voigt(o["ep"]), alpha=o["alpha"], plastic=o["plastic"],
                   f_tr=o["f_tr"], Kt=None)
        if tangent:
            Cm = tangent_moduli(o, self.mu, self.kappa, self.H)
            K = torch.einsum("maj,mijkl,mbl->maibk", self.g, Cm, self.g) * V.view(-1, 1, 1, 1, 1)
            res["Kt"] = K.reshape(self.M, 12, 12)
        return res

    def element_potential(self, ue, state=None):
        """we [M] from the element displacements ue [M,4,3] (differentiable)."""
        ep_n, al_n = self._state(state)
        return self.V * update(self.strain_of(ue), ep_n, al_n, self.mu, self.kappa, self.sigma_y, self.H)["w"]

    def next_state(self, u, state=None):
        o = self.update(u, state)
        return to_voigt(o["ep"]), o["alpha"]

    def f_int(self, u, state=None, fe=None):
        fe = self.element(u, state, tangent=False)["fe"] if fe is None else fe
        out = torch.zeros(self.N, 3, dtype=F64)
        out.index_add_(0, self.tets.reshape(-1), fe.reshape(-1, 3))
        return out

    def dense_tangent(self, u, state=None):
        return MR.dense(self.element(u, state)["Kt"], self.tets, self.N, 3)


# ---------------------------------------------------------------- materials, displacement fields, load cases
def material(scale):
    """(E, nu, sigma_y, H) of the two test materials."""
    if scale == "bench":
        return MR.E, MR.NU, 1e-3 * MR.E, 0.1 * MR.E
    return 1.0, 0.3, 0.01, 0.1


def yield_strain(E, nu, sigma_y):
    return sigma_y / (2.0 * moduli(E, nu)[0])


def field(name, coords, n, ey, seed=7):
    """The displacement fields of the element tests on a mesh of n cells per edge; ey = sigma_y / (2 mu) is the size of
    the deviatoric strain at first yield. The amplitudes were picked on the CPU (test_plasticity_cpu checks them): every
    element of `small` is elastic, every element of `large` yields, `graded` yields in 25-75 % of the elements, and
    |f_tr| >= 1e-6 sigma_y everywhere, from the virgin and from the hardened state."""
    c = coords.to(F64)
    if name == "zero":
        return torch.zeros_like(c)
    rnd = 2.0 * torch.rand(c.shape, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 1.0
    size = c.abs().amax(0)
    if name == "small":
        return (0.02 * ey / n) * rnd * size
    if name == "large":
        return (40.0 * ey / n) * rnd * size
    if name == "graded":
        x = c[:, 0] / size[0]
        return torch.stack((GRADED_A * ey * size[0] * x * x, torch.zeros_like(x), torch.zeros_like(x)), dim=1)
    if name == "harden":    # produces the hardened input state of the element tests (the single tet needs more)
        z = c[:, 2] / size[2]
        return torch.stack((torch.zeros_like(z), torch.zeros_like(z), (HARDEN_AMP if c.shape[0] > 4 else 1.6 * HARDEN_AMP) * ey * size[2] * z * z), dim=1)
    raise ValueError(name)


GRADED_A = 1.3
HARDEN_AMP = 0.9
FIELDS = ("zero", "small", "large", "graded")


def hardened_state(model, n):
    """The state the reference reaches from the virgin one on the `harden` field."""
    ey = yield_strain(model.E, model.nu, model.sigma_y)
    return model.next_state(field("harden", model.coords, n, ey))


def x_face_traction(coords, tets, t):
    """Consistent nodal loads [N,3] of the uniform traction (t, 0, 0) on the face x = max x (A/3 per node of a
    boundary triangle)."""
    c = coords.to(F64)
    xmax = float(c[:, 0].max())
    F = torch.zeros_like(c)
    for f in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        tri = tets[:, list(f)]
        on = (c[tri][:, :, 0] == xmax).all(1)
        p = c[tri[on]]
        area = 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1)
        for a in range(3):
            F[:, 0].index_add_(0, tri[on][:, a], area * t / 3.0)
    return F


def roller_mask(coords):
    """[N,3] bool: u_x = 0 on x = 0, u_y = 0 on y = 0, u_z = 0 on z = 0."""
    return coords.to(F64) == 0.0


def uniaxial_case(coords, tets):
    """The uniaxial case on a unit cube of the unit material: (model, F at the full traction t_max = 2 sigma_y on
    x = 1, roller mask, exact u [N,3] after each load factor of the path 0.5, 1.0, 0.0, exact alpha after the second
    step). Linear tets reproduce the homogeneous state: sigma_xx = t alone, eps_xx = t/E + (t - sigma_y)/H once
    t > sigma_y, the plastic part isochoric (lateral strain -1/2 of it)."""
    m = Model(coords, tets, *material("unit"))
    E, nu, sy, H = m.E, m.nu, m.sigma_y, m.H
    tmax = 2.0 * sy
    F = x_face_traction(m.coords, m.tets, tmax)
    x = m.coords

    def u_of(exx, eyy):
        return torch.stack((exx * x[:, 0], eyy * x[:, 1], eyy * x[:, 2]), dim=1)

    pl = (tmax - sy) / H
    exact = [u_of(0.5 * tmax / E, -nu * 0.5 * tmax / E), u_of(tmax / E + pl, -nu * tmax / E - 0.5 * pl),
             u_of(pl, -0.5 * pl)]
    return m, F, roller_mask(m.coords), exact, pl


SOLVER_CASES = {"pull": (0.0, 0.0, 0.0112), "shear": (0.00455, 0.0, 0.0)}
LOAD_PATH = (0.5, 1.0, 0.3)


def solver_case(coords, name):
    """(F [N,3], fixed node ids): the z = 0 face fixed, the total top-face force spread evenly over the top nodes.
    For the unit material (sigma_y = 0.01) on the unit cube; sized on the CPU so that 30-90 % of the elements end
    plastic at full load."""
    c = coords.to(F64)
    z = c[:, 2]
    fixed = torch.nonzero(z == z.min()).reshape(-1)
    top = torch.nonzero(z == z.max()).reshape(-1)
    F = torch.zeros_like(c)
    F[top] = torch.tensor(SOLVER_CASES[name], dtype=F64) / top.numel()
    return F, fixed


# ---------------------------------------------------------------- dense Newton restatement over a load path
def newton(model, F, mask, load_path, state=None, tol=1e-8, atol=0.0, max_iter=25, linear="direct", linear_rtol=1e-6,
           linear_max_iter=10000, u_init=None, verbose=False):
    """Newton per load factor from the previous u, the state committed after every converged step; the stop rule
    (scale max |lambda| ||F_free||) and line search of solver.elastoplastic_static_solver (a trial taken for its
    smaller residual must not raise the potential by more than its rounding: the potential is convex but only
    piecewise smooth, and full Newton steps accepted on the residual alone can cycle between two sets of yielding
    elements). mask: [N,3] bool, True on
    the dofs held at zero. linear: "direct" or "pcg". Returns (u [N,3], state, info) with info = dict(converged,
    iterations [per step], plastic_fraction [per step], u_steps, states, pcg_iterations, failed_step)."""
    N = model.N
    free = ~mask.reshape(-1)
    Fv = F.to(F64).reshape(-1)
    lmax = max(abs(float(l)) for l in load_path)
    stop = max(tol * lmax * float(Fv[free].norm()), atol)
    u = torch.zeros(3 * N, dtype=F64) if u_init is None else u_init.to(F64).reshape(-1).clone()
    u[~free] = 0.0
    state = virgin(model.M) if state is None else (state[0].clone(), state[1].clone())
    info = {"converged": False, "iterations": [], "plastic_fraction": [], "u_steps": [], "states": [],
            "pcg_iterations": [], "failed_step": None}

    K_el = model.dense_tangent(torch.zeros(N, 3, dtype=F64))

    def evaluate(v, lf):
        el = model.element(v.view(N, 3), state, tangent=False)
        r = lf * Fv - model.f_int(None, fe=el["fe"]).reshape(-1)
        r[~free] = 0.0
        en, work = float(el["we"].sum()), lf * float(Fv @ v)
        return r, en - work, float(r.norm()), el, abs(en) + abs(work)

    for s, lf in enumerate(load_path, 1):
        lf = float(lf)
        its, done = 0, False
        for k in range(1, max_iter + 1):
            r, pot, rn, el, _ = evaluate(u, lf)
            if verbose:
                print(f"step {s} iteration {k}: residual {rn:.3e} potential {pot:.16e} plastic {int(el['plastic'].sum())}")
            if rn <= stop:
                done = True
                break
            # the first iteration of a step takes the elastic tangent: at the u just committed every yielded element
            # has f_tr = 0 up to rounding, and which branch its tangent would take is noise
            K = K_el if k == 1 else model.dense_tangent(u.view(N, 3), state)
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
                _, pot_t, rn_t, _, mag = evaluate(ut, lf)
                if pot_t <= pot - LS_C1 * alpha * slope or (rn_t < rn and pot_t <= pot + LS_POT_ROUND * mag):
                    ok = True
                    break
                alpha *= 0.5
            if not ok:
                break
            u = ut
            its += 1
        info["iterations"].append(its)
        if not done:
            info["failed_step"] = s
            return u.view(N, 3), state, info
        state = (el["ep"], el["alpha"])
        info["plastic_fraction"].append(float(el["plastic"].to(F64).mean()))
        info["u_steps"].append(u.view(N, 3).clone())
        info["states"].append(state)
    info["converged"] = True
    return u.view(N, 3), state, info
