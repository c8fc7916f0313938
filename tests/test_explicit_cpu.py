"""CPU tier of the explicit dynamics: every argument check of the public entry points (ValueError before any device
work), and the properties of the fp64 restatement tests/explicit_ref.py that the device tests lean on.

  total lumped mass     == rho x volume, rel <= 1e-14
  step bound            dt_est <= 2 / omega_max of the dense M_lumped^-1 K on kuhn_cube(2 / 3 / 6, jitter 0.15), E = 1,
                        nu = 0.3, rho = 1 -- and dt_est >= 0.3 x 2 / omega_max, a guard against a uselessly small
                        bound (the restatement gives 0.555, 0.480 and 0.384 of 2 / omega_max)
  discrete dispersion   linear material, kuhn3 clamped at z = 0, u0 = phi_j, v0 = 0, no load: the leapfrog iterate is
                        exactly phi_j cos(omega_h n dt) with sin(omega_h dt / 2) = omega_j dt / 2 (u_1 = phi (1 -
                        omega^2 dt^2 / 2) and the three-term recurrence holds); 200 steps at dt = 0.9 dt_est, j = 1 and
                        the highest mode, bound 4 n^2 1e-12 max|u| (the bound of the device test)."""
import functools
import math

import pytest
import torch

import explicit_ref as XR
import fem355  # noqa: F401
from fem355 import element, mesh, solver, system

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def cube(n):
    c, t = mesh.kuhn_cube(n, jitter=0.15)
    return c.to(F64), t


# ---------------------------------------------------------------- argument checks
def _args(**kw):
    c, t = cube(2)
    N = c.shape[0]
    a = dict(coords=c, elements=t, F=torch.zeros(N, 3, dtype=F64), fixed=[0, 1], rho=1.0, E=1.0, nu=0.3, steps=4,
             device="cpu")
    a.update(kw)
    return a


BAD = {
    "coords shape": dict(coords=torch.zeros(5, 2, dtype=F64)),
    "elements shape": dict(elements=torch.zeros(3, 5, dtype=torch.long)),
    "node out of range": dict(elements=torch.tensor([[0, 1, 2, 999]])),
    "F shape": dict(F=torch.zeros(3, 3, dtype=F64)),
    "rho zero": dict(rho=0.0),
    "rho negative": dict(rho=-1.0),
    "dt zero": dict(dt=0.0),
    "dt negative": dict(dt=-1e-3),
    "steps negative": dict(steps=-1),
    "unknown material": dict(material="mooney"),
    "amplitude length": dict(amplitude=torch.ones(4, dtype=F64)),
    "amplitude type": dict(amplitude=3.0),
    "record low": dict(record=[-1]),
    "record high": dict(record=[27]),
    "damping negative": dict(damping=-0.1),
    "nu high": dict(nu=0.5),
    "nu low": dict(nu=-1.0),
    "u0 shape": dict(u0=torch.zeros(4, 3, dtype=F64)),
    "v0 shape": dict(v0=torch.zeros(27, 2, dtype=F64)),
    "fixed out of range": dict(fixed=[27]),
    "fixed mask shape": dict(fixed=torch.zeros(5, 3, dtype=torch.bool)),
    "energy_every negative": dict(energy_every=-1),
    "safety": dict(safety=1.5),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_solver_argument_checks(name):
    with pytest.raises(ValueError):
        solver.explicit_dynamics_solver(**_args(**BAD[name]))


def test_element_argument_checks():
    c, t = cube(2)
    for kw in (dict(rho=0.0), dict(rho=-2.0)):
        with pytest.raises(ValueError):
            element.compute_c3d4_lumped_mass(c, t, device="cpu", **kw)
    for E, nu, rho in ((1.0, 0.5, 1.0), (1.0, -1.0, 1.0), (1.0, 0.3, 0.0), (0.0, 0.3, 1.0)):
        with pytest.raises(ValueError):
            element.compute_c3d4_stable_time_step(c, t, E, nu, rho, device="cpu")
    with pytest.raises(ValueError):
        element.compute_c3d4_lumped_mass(c[:, :2], t, 1.0, device="cpu")
    with pytest.raises(ValueError):
        element.compute_c3d4_stable_time_step(c, t[:, :3], 1.0, 0.3, 1.0, device="cpu")


def test_integrator_argument_checks():
    c, t = cube(2)
    for kw in (dict(material="mooney"), dict(damping=-1.0), dict(fixed_mask=torch.zeros(5, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            system.ExplicitDynamics(c, t, 1.0, 1.0, 0.3, **kw)
    with pytest.raises(ValueError):
        system.ExplicitDynamics(c, t, 0.0, 1.0, 0.3)
    with pytest.raises(ValueError):
        system.ExplicitDynamics(c, t, 1.0, 1.0, 0.5)
    for steps, dt in ((-1, 1.0), (1.5, 1.0), (3, 0.0), (3, -1.0)):
        with pytest.raises(ValueError):
            system.check_explicit_run("run", steps, dt)
    assert system.ExplicitResult(0, system.XD_OK, -1, 1.0).status == "OK"
    assert (system.XD_INVERTED, system.XD_DIVERGED) == ("INVERTED", "DIVERGED")


# ---------------------------------------------------------------- the restatement's own properties
@pytest.mark.parametrize("n", [2, 3, 6])
def test_total_lumped_mass(n):
    c, t = cube(n)
    rho = 4430.0
    m = XR.lumped_mass(c, t, rho)
    vol = float(XR.R.tet_volumes(c, t).sum())
    assert abs(float(m.sum()) - rho * vol) <= 1e-14 * rho * vol
    assert abs(vol - 1.0) <= 1e-12 and bool((m > 0).all())


RATIO = {2: 0.555, 3: 0.480, 6: 0.384}


@pytest.mark.parametrize("n", [2, 3, 6])
def test_step_bound_is_stable_and_useful(n):
    c, t = cube(n)
    dt, dte = XR.element_dt(c, t, 1.0, 0.3, 1.0)
    crit = 2.0 / XR.omega_max(c, t, 1.0, 0.3, 1.0)
    print(f"kuhn{n}: dt_est {dt:.6e}  2/omega_max {crit:.6e}  ratio {dt / crit:.3f}")
    assert dte.shape == (t.shape[0],) and dt == float(dte.min())
    assert dt <= crit
    assert dt >= 0.3 * crit
    assert abs(dt / crit - RATIO[n]) <= 5e-4


def test_step_bound_scales():
    """dt_e scales with length and with sqrt(rho / E)."""
    c, t = cube(2)
    d0, _ = XR.element_dt(c, t, 1.0, 0.3, 1.0)
    d1, _ = XR.element_dt(2.0 * c, t, 4.0, 0.3, 9.0)
    assert abs(d1 - d0 * 2.0 * 1.5) <= 1e-13 * d1


@functools.lru_cache(maxsize=None)
def dispersion_case():
    c, t = cube(3)
    free = torch.ones((c.shape[0], 3), dtype=torch.bool)
    free[mesh.face_nodes(c, 2, 0.0)] = False
    free = free.view(-1)
    om, Phi = XR.modes(c, t, 1.0, 0.3, 1.0, free)
    dt = 0.9 * XR.element_dt(c, t, 1.0, 0.3, 1.0)[0]
    return c, t, free, om, Phi, dt


def dispersion_exact(om, phi, dt, steps):
    """phi cos(omega_h n dt), n = 0 .. steps."""
    wh = 2.0 * math.asin(0.5 * om * dt) / dt
    k = torch.arange(steps + 1, dtype=F64)
    return torch.cos(wh * k * dt).view(-1, 1) * phi.view(1, -1)


@pytest.mark.parametrize("j", [0, -1])
def test_exact_discrete_dispersion(j):
    c, t, free, om, Phi, dt = dispersion_case()
    steps = 200
    assert 0.5 * float(om[-1]) * dt < 1.0
    model = XR.Model(c, t, 1.0, 0.3, "linear")
    out = XR.leapfrog(model, XR.lumped_mass(c, t, 1.0), free, dt, steps, u0=Phi[:, j])
    ref = dispersion_exact(float(om[j]), Phi[:, j], dt, steps)
    dev = float((out["U"] - ref).abs().max())
    print(f"mode {j}: omega dt / 2 = {0.5 * float(om[j]) * dt:.4f}  max deviation {dev:.3e}")
    assert dev <= 4 * steps ** 2 * 1e-12 * float(ref.abs().max())
