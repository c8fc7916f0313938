"""CPU fp64 restatement of the explicit dynamics (torch only), written from the formulation, not from kernel text:
    lumped mass       m_i = sum over the elements at node i of rho V_e / 4
    element step      dt_e = 1 / (c_d sqrt(sum_a |g_a|^2)), c_d^2 = (max(lam, 0) + 2 mu) / rho (= (lam + 2 mu) / rho for nu >= 0)
    internal force    linear: the dense oracle.ref_cpu tet4 K times u; svk / neo_hookean: hyperelastic_ref.Model.f_int
    strain energy     linear: u.K u / 2; svk / neo_hookean: hyperelastic_ref.Model.energies
    leapfrog          a_n = (amp_n F - f_int(u_n)) / m - alpha v_n,
                      v_{1/2} = v_0 + (dt/2) a_0, else v_{n+1/2} = ((1 - alpha dt/2) v_{n-1/2} + dt r_n / m) / (1 + alpha dt/2),
                      u_{n+1} = u_n + dt v_{n+1/2},  v_n = (v_{n-1/2} + v_{n+1/2}) / 2
Fixed dofs and nodes of zero mass stay at u = v = a = 0."""
import math

import torch

import hyperelastic_ref as HR
import modal_ref as MR
from oracle import ref_cpu as R

F64 = torch.float64
MATERIALS = ("linear", "svk", "neo_hookean")


def lumped_mass(coords, tets, rho):
    N = coords.shape[0]
    m = torch.zeros(N, dtype=F64)
    if tets.shape[0]:
        q = rho * R.tet_volumes(coords.to(F64), tets) / 4.0
        m.index_add_(0, tets.reshape(-1), q.repeat_interleave(4))
    return m


def element_dt(coords, tets, E, nu, rho):
    """(dt, dt_e [M])."""
    if tets.shape[0] == 0:
        return float("inf"), torch.zeros(0, dtype=F64)
    g = R.tet4_gradients(coords.to(F64), tets)
    lam, mu = HR.lame(E, nu)
    cd = math.sqrt((max(lam, 0.0) + 2.0 * mu) / rho)
    dte = 1.0 / (cd * torch.sqrt((g * g).sum((1, 2))))
    return float(dte.min()), dte


def dense_K(coords, tets, E, nu):
    return MR.dense(R.tet4_K(coords.to(F64), tets, E, nu), tets, coords.shape[0], 3)


def omega_max(coords, tets, E, nu, rho, free=None):
    """Largest omega of K x = omega^2 M_lumped x on the free dofs (all dofs when free is None)."""
    K = dense_K(coords, tets, E, nu)
    m = lumped_mass(coords, tets, rho).repeat_interleave(3)
    if free is None:
        free = torch.ones_like(m, dtype=torch.bool)
    s = 1.0 / torch.sqrt(m[free])
    A = K[free][:, free] * s.view(-1, 1) * s.view(1, -1)
    return math.sqrt(float(torch.linalg.eigvalsh(0.5 * (A + A.T))[-1]))


def modes(coords, tets, E, nu, rho, free):
    """(omega [nf] ascending, Phi [3N, nf] with zero rows on the fixed dofs) of the lumped-mass pencil."""
    K = dense_K(coords, tets, E, nu)
    m = lumped_mass(coords, tets, rho).repeat_interleave(3)
    s = 1.0 / torch.sqrt(m[free])
    A = K[free][:, free] * s.view(-1, 1) * s.view(1, -1)
    lam, Z = torch.linalg.eigh(0.5 * (A + A.T))
    Phi = torch.zeros((m.numel(), lam.numel()), dtype=F64)
    Phi[free] = Z * s.view(-1, 1)
    return torch.sqrt(lam), Phi


class Model:
    """f_int and strain energy of one mesh + material at u [3N]."""

    def __init__(self, coords, tets, E, nu, material):
        self.N, self.material = coords.shape[0], material
        if material == "linear":
            self.K = dense_K(coords, tets, E, nu)
        else:
            self.hr = HR.Model(coords, tets, E, nu, material)

    def f_int(self, u):
        if self.material == "linear":
            return self.K @ u
        return self.hr.f_int(u.view(self.N, 3)).reshape(-1)

    def energy(self, u):
        if self.material == "linear":
            return float(u @ (self.K @ u)) * 0.5
        return float(self.hr.energies(u.view(self.N, 3)).sum())


def leapfrog(model, m, free, dt, steps, F=None, amps=None, u0=None, v0=None, alpha=0.0, energy_every=0):
    """`steps` leapfrog steps. m [N], free [3N] bool. Returns a dict: U [steps + 1, 3N] (u_0 .. u_steps), V, A [steps + 1,
    3N] (v_n, a_n; the last row as the device forms the state reached), energy rows (steps n < steps with
    n % energy_every == 0): t, kinetic, strain, ext_power, ext_work."""
    n = 3 * model.N
    md = m.repeat_interleave(3)
    free = free & (md > 0)
    mi = torch.where(free, 1.0 / md.clamp(min=1e-300), torch.zeros(n, dtype=F64))
    z = lambda: torch.zeros(n, dtype=F64)
    Fv = z() if F is None else F.to(F64).reshape(-1)
    amps = [1.0] * (steps + 1) if amps is None else [float(a) for a in amps]
    u = (z() if u0 is None else u0.to(F64).reshape(-1).clone()) * free
    v = (z() if v0 is None else v0.to(F64).reshape(-1).clone()) * free
    U, V, A = [u.clone()], [], []
    en = {k: [] for k in ("t", "kinetic", "strain", "ext_power", "ext_work")}
    c1, c2 = 1.0 - 0.5 * alpha * dt, 1.0 / (1.0 + 0.5 * alpha * dt)
    vh = None
    for k in range(steps + 1):
        rm = (amps[k] * Fv - model.f_int(u)) * mi
        if vh is None:
            vn = v
            an = (rm - alpha * vn) * free
            vhn = vn + 0.5 * dt * an
        else:
            vhn = (c1 * vh + dt * rm) * c2
            vn = 0.5 * (vh + vhn)
            an = (rm - alpha * vn) * free
        V.append(vn.clone())
        A.append(an.clone())
        if k == steps:
            break
        if energy_every and k % energy_every == 0:
            en["t"].append(k * dt)
            en["kinetic"].append(float(0.5 * (md * vn * vn).sum()))
            en["strain"].append(model.energy(u))
            en["ext_power"].append(float(amps[k] * (Fv @ vn)))
            en["ext_work"].append(float(amps[k] * (Fv @ u)))
        u = u + dt * vhn
        vh = vhn
        U.append(u.clone())
    out = dict(U=torch.stack(U), V=torch.stack(V), A=torch.stack(A))
    out.update({k: torch.tensor(x, dtype=F64) for k, x in en.items()})
    return out
