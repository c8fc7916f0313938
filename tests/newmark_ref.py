"""Dense CPU reference for the transient solver (torch fp64 only): Newmark-beta with Rayleigh damping restated on the
free dofs of a modal_ref.Case, with two linear solvers -- a Cholesky solve ("direct") and a Jacobi-PCG with the device's
stop rule (sqrt(r.z) < rtol sqrt(b.(w o b)) tested after every iteration, never before the first) and warm start
("pcg"), i.e. what system.NewmarkIntegrator runs.

    K_eff = (1 + a1 beta_R) K + (a0 + a1 alpha) M
    b     = f_{n+1} + M ((a0 + alpha a1) u + (a2 + alpha a4) v + (a3 + alpha a5) a) + K beta_R (a1 u + a4 v + a5 a)
    a_new = a0 (u_new - u) - a2 v - a3 a,   v_new = v + dt ((1 - gamma) a + gamma a_new)
"""
import functools
import math

import torch

import modal_ref as MR

F64 = torch.float64
STEPS = 64
CASES = ("elastic4", "poisson6", "hex4", "lumped5")
DAMPED = dict(gamma=0.6, beta=0.3025)   # with alpha = 0.05 omega_j, beta_R = 0.02 / omega_j


def constants(dt, beta, gamma, alpha, beta_r):
    a0, a1, a2 = 1.0 / (beta * dt * dt), gamma / (beta * dt), 1.0 / (beta * dt)
    a3, a4, a5 = 1.0 / (2.0 * beta) - 1.0, gamma / beta - 1.0, 0.5 * dt * (gamma / beta - 2.0)
    return a0, a1, a2, a3, a4, a5


class Run:
    """u, v, a [steps + 1, n] (zeros on the fixed dofs), energy [steps + 1], PCG iterations per step."""

    def __init__(self, u, v, a, energy, iters):
        self.u, self.v, self.a, self.energy, self.iters = u, v, a, energy, iters

    def drift(self):
        """max |E_n - E_0| / E_0"""
        return float((self.energy - self.energy[0]).abs().max() / self.energy[0])


def _pcg(A, b, w, x0, tol, max_iter):
    x = x0.clone()
    r = b - A @ x
    z = w * r
    p = z.clone()
    rz = torch.dot(r, z)
    for i in range(max_iter):
        q = A @ p
        al = rz / torch.dot(p, q)
        x += al * p
        r -= al * q
        z = w * r
        rz_new = torch.dot(r, z)
        if float(torch.sqrt(rz_new)) < tol:
            return x, i + 1
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise AssertionError(f"reference PCG: no convergence in {max_iter} iterations")


def newmark(cs, dt, steps=STEPS, u0=None, v0=None, load=None, beta=0.25, gamma=0.5, alpha=0.0, beta_r=0.0,
            solver="direct", rtol=1e-8, predictor=False, max_iter=5000):
    """Integrate the case `cs` from (u0, v0) [n] under load(k) -> f [n] at step k = 0..steps (None: no load)."""
    f = cs.free
    K, M = cs.K[f][:, f], cs.M[f][:, f]
    nf = K.shape[0]
    a0, a1, a2, a3, a4, a5 = constants(dt, beta, gamma, alpha, beta_r)
    Keff = (1.0 + a1 * beta_r) * K + (a0 + a1 * alpha) * M
    zero = torch.zeros(nf, dtype=F64)
    ld = (lambda k: zero) if load is None else (lambda k: load(k)[f])
    u = zero.clone() if u0 is None else u0[f].clone()
    v = zero.clone() if v0 is None else v0[f].clone()
    LM = torch.linalg.cholesky(M)
    a = torch.cholesky_solve((ld(0) - alpha * (M @ v) - K @ (u + beta_r * v)).unsqueeze(1), LM).squeeze(1)
    if solver == "direct":
        L = torch.linalg.cholesky(Keff)
    w = 1.0 / Keff.diagonal()
    U, V, Acc, its = [u], [v], [a], []
    for k in range(1, steps + 1):
        yM = (a0 + alpha * a1) * u + (a2 + alpha * a4) * v + (a3 + alpha * a5) * a
        yK = beta_r * (a1 * u + a4 * v + a5 * a)
        b = ld(k) + M @ yM + K @ yK
        if solver == "direct":
            un = torch.cholesky_solve(b.unsqueeze(1), L).squeeze(1)
        else:
            tol = rtol * math.sqrt(float(torch.dot(b, w * b)))
            un, it = _pcg(Keff, b, w, u + dt * v if predictor else u, tol, max_iter)
            its.append(it)
        an = a0 * (un - u) - a2 * v - a3 * a
        v = v + dt * ((1.0 - gamma) * a + gamma * an)
        u, a = un, an
        U.append(u)
        V.append(v)
        Acc.append(a)

    def full(rows):
        out = torch.zeros((len(rows), cs.n), dtype=F64)
        out[:, f] = torch.stack(rows)
        return out

    U, V, Acc = full(U), full(V), full(Acc)
    E = 0.5 * ((U @ cs.K) * U).sum(1) + 0.5 * ((V @ cs.M) * V).sum(1)
    return Run(U, V, Acc, E, its)


# ---------------------------------------------------------------- the standard scenarios of the tests
def mode(cs, j=1):
    """(omega_j, phi_j [n]) of the dense pencil (j = 1: the lowest mode)."""
    lam, Uv = cs.eig
    return math.sqrt(float(lam[j - 1])), Uv[:, j - 1].clone()


def step_size(cs, j=1):
    """dt = T_j / 20"""
    return 2.0 * math.pi / mode(cs, j)[0] / 20.0


def six_mode_start(cs):
    """A start displacement with the six lowest modes in it (weights 1, 1/2, ... 1/6)."""
    _, Uv = cs.eig
    return (Uv[:, :6] / torch.arange(1, 7, dtype=F64)).sum(1)


def load_vector(cs):
    """A fixed pseudo-random nodal load, zero on the clamped dofs, of the size that deflects the structure by about
    the magnitude of its first mode shape."""
    g = torch.Generator().manual_seed(7)
    F = torch.randn(cs.n, dtype=F64, generator=g) * cs.free
    return F * float(cs.eig[0][0])


def scenario(cs, name):
    """kwargs of `newmark` (without solver / rtol) for the named scenario."""
    om, phi = mode(cs)
    dt = step_size(cs)
    F = load_vector(cs)
    if name == "mode":
        return dict(dt=dt, u0=phi)
    if name == "damped":
        return dict(dt=dt, u0=six_mode_start(cs), alpha=0.05 * om, beta_r=0.02 / om, **DAMPED)
    if name == "step_load":
        return dict(dt=dt, load=lambda k: F)
    if name == "sine_load":
        return dict(dt=dt, load=lambda k: math.sin(0.7 * om * k * dt) * F)
    if name == "predictor":
        return dict(dt=dt, u0=phi, predictor=True)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(case_name, scen, solver):
    cs = MR.case(case_name)
    return newmark(cs, solver=solver, **scenario(cs, scen))
