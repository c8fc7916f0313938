"""CPU tier of the penalty contact of the explicit dynamics: every argument check (ValueError before any
device work) and the identities of the fp64 restatement tests/contact_ref.py that the device tests lean on, all on
kuhn_cube(3, jitter=0.15), E = 1, nu = 0.3, rho = 1, dt = 0.9 x the guaranteed bound, penalty 0.5:

  impulse        free body, no damping: sum_i m_i (v_N - v_0) = dt (R_0 / 2 + R_1 + ... + R_{N-1} + R_N / 2), R the total
                 contact force; exact up to rounding, asserted to 1e-12 of |sum m v_0|
  drop           frictionless, v0 = (0, 0, -0.05), plane 1e-3 below the cube, 400 steps: the cube leaves again with a
                 positive mean v_z and kinetic + strain + penalty energy stays within 2 % of its start
  friction       the friction power is never positive (beyond the rounding of a node the cap has just stopped: 1e-14 of
                 the largest power); kinetic + strain + penalty - F.u at the last sampled step is below its first
  per node       |f_t| <= mu |f_n| and f_t . vt <= 0 for every node, surface and step

Measured here: impulse identity 2.5e-14; drop energy range -1.06 % / +0.24 %, 30 steps in contact, rebound at 0.83 of
the approach speed, deepest penetration 8.3e-3 (0.025 of an edge); sliding block: the balance falls from 2.0e-4 to
3.2e-5 and never exceeds its start, friction power between -6.2e-5 and +5.0e-22."""
import functools

import pytest
import torch

import contact_ref as CR
import explicit_ref as XR
import fem355  # noqa: F401
from fem355 import mesh, solver, system

F64 = torch.float64
E, NU, RHO, KAPPA = 1.0, 0.3, 1.0, 0.5


@functools.lru_cache(maxsize=None)
def cube(n=3):
    c, t = mesh.kuhn_cube(n, jitter=0.15)
    c = c.to(F64)
    m = XR.lumped_mass(c, t, RHO)
    dt = 0.9 * XR.element_dt(c, t, E, NU, RHO)[0]
    return c, t, m, dt, XR.Model(c, t, E, NU, "linear")


# ---------------------------------------------------------------- argument checks
def plane(**kw):
    a = dict(kind="plane", point=[0.0, 0.0, 0.0], normal=[0.0, 0.0, 1.0])
    a.update(kw)
    return a


BAD_SURFACE = {
    "unknown kind": dict(kind="torus", point=[0, 0, 0], radius=1.0),
    "zero normal": plane(normal=[0.0, 0.0, 0.0]),
    "missing normal": plane(normal=None),
    "zero axis": dict(kind="cylinder", point=[0, 0, 0], axis=[0, 0, 0], radius=1.0),
    "missing axis": dict(kind="cylinder", point=[0, 0, 0], radius=1.0),
    "missing radius sphere": dict(kind="sphere", point=[0, 0, 0]),
    "zero radius sphere": dict(kind="sphere", point=[0, 0, 0], radius=0.0),
    "negative radius cylinder": dict(kind="cylinder", point=[0, 0, 0], axis=[0, 0, 1], radius=-1.0),
    "negative friction": plane(friction=-0.1),
    "point length": plane(point=[0.0, 0.0]),
    "velocity and displacement": plane(velocity=[0, 0, 1], displacement=lambda t: [0, 0, t]),
    "displacement not callable": plane(displacement=[0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(BAD_SURFACE))
def test_surface_argument_checks(name):
    with pytest.raises(ValueError):
        system.RigidSurface(**BAD_SURFACE[name])


def test_contact_set_argument_checks():
    ok = system.RigidSurface(**plane())
    assert system.check_contact("t", [ok] * 8, 0.5, 10) == [ok] * 8
    with pytest.raises(ValueError):
        system.check_contact("t", [ok] * 9, 0.5, 10)
    with pytest.raises(ValueError):
        system.check_contact("t", [ok, "plane"], 0.5, 10)
    for nodes in ([10], [-1], [0, 3, 11]):
        with pytest.raises(ValueError):
            system.check_contact("t", [system.RigidSurface(**plane(nodes=nodes))], 0.5, 10)
    system.check_contact("t", [system.RigidSurface(**plane(nodes=[0, 9]))], 0.5, 10)
    for penalty in (0.0, -0.5, 4.0, 5.0, float("nan")):
        with pytest.raises(ValueError):
            system.check_contact("t", [ok], penalty, 10)
    # the step bound: 4 (1 - 0.9^2) = 0.76
    system.check_contact("t", [ok], 0.76, 10, safety=0.9)
    with pytest.raises(ValueError):
        system.check_contact("t", [ok], 0.77, 10, safety=0.9)
    system.check_contact("t", [ok], 3.9, 10)             # set_contact itself only asks for (0, 4)
    s = system.RigidSurface("cylinder", [0, 0, 0], axis=[0, 3, 4], radius=2.0, inside=True, friction=0.2)
    assert s.direction == (0.0, 0.6, 0.8) and s.inside and s.radius == 2.0
    assert not system.RigidSurface(**plane(inside=True)).inside


def _solver_args(**kw):
    c, t = mesh.kuhn_cube(2, jitter=0.15)
    N = c.shape[0]
    a = dict(coords=c.to(F64), elements=t, F=torch.zeros(N, 3, dtype=F64), fixed=[], rho=1.0, E=1.0, nu=0.3, steps=4,
             device="cpu")
    a.update(kw)
    return a


def test_solver_contact_argument_checks():
    ok = system.RigidSurface(**plane())
    bad = [dict(contact=[ok] * 9), dict(contact=[ok], penalty=0.0), dict(contact=[ok], penalty=4.0),
           dict(contact=[ok], penalty=0.77),                       # dt = None, safety 0.9: beyond 0.76
           dict(contact=[ok], penalty=0.5, safety=0.95),           # 4 (1 - 0.95^2) = 0.39
           dict(contact=[system.RigidSurface(**plane(nodes=[27]))]), dict(contact=["plane"]),
           dict(contact=[ok], contact_every=-1), dict(contact_every=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            solver.explicit_dynamics_solver(**_solver_args(**kw))
    # a given dt lifts the safety bound (the caller answers for the step): tests/test_gpu_contact.py runs that call


# ---------------------------------------------------------------- the restatement's identities
def test_impulse_identity():
    c, t, m, dt, model = cube()
    N = c.shape[0]
    free = torch.ones(3 * N, dtype=torch.bool)
    v0 = torch.tensor([0.03, 0.0, -0.05], dtype=F64).repeat(N, 1)
    floor = CR.Surface("plane", [0.0, 0.0, float(c[:, 2].min()) - 1e-3], normal=[0, 0, 1], friction=0.3)
    steps = 120
    out = CR.leapfrog(model, c, m, free, dt, steps, [floor], KAPPA, v0=v0)
    R = out["FC"].view(steps + 1, N, 3).sum(1)
    assert float(R.abs().max()) > 0.0
    lhs = (m.view(-1, 1) * (out["V"][-1] - out["V"][0]).view(N, 3)).sum(0)
    rhs = dt * (0.5 * R[0] + R[1:-1].sum(0) + 0.5 * R[-1])
    p0 = float((m.view(-1, 1) * v0).sum(0).norm())
    dev = float((lhs - rhs).abs().max()) / p0
    print(f"impulse identity: {dev:.2e} of |sum m v0|")
    assert dev <= 1e-12


@functools.lru_cache(maxsize=None)
def drop():
    c, t, m, dt, model = cube()
    N = c.shape[0]
    free = torch.ones(3 * N, dtype=torch.bool)
    v0 = torch.tensor([0.0, 0.0, -0.05], dtype=F64).repeat(N, 1)
    floor = CR.Surface("plane", [0.0, 0.0, float(c[:, 2].min()) - 1e-3], normal=[0, 0, 1])
    return CR.leapfrog(model, c, m, free, dt, 400, [floor], KAPPA, v0=v0, energy_every=1, contact_every=1)


def test_frictionless_drop_rebounds_and_keeps_energy():
    c, t, m, dt, model = cube()
    out = drop()
    vz = float((m * out["V"][-1].view(-1, 3)[:, 2]).sum() / m.sum())
    tot = out["kinetic"] + out["strain"] + out["contact_energy"]
    lo, hi = float(tot.min() / tot[0]) - 1.0, float(tot.max() / tot[0]) - 1.0
    touching = int((out["in_contact"][:, 0] > 0).sum())
    print(f"drop: mean v_z at the end {vz:+.4f} (approach -0.05), energy range {100 * lo:+.2f} % / {100 * hi:+.2f} %, "
          f"{touching} steps in contact, deepest penetration {float(out['penetration'].max()):.3e}")
    assert touching > 0 and int(out["in_contact"][-1, 0]) == 0
    assert vz > 0.0
    assert -0.02 <= lo and hi <= 0.02
    assert float(out["friction_power"].abs().max()) == 0.0 and float(out["surface_power"].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def slide():
    c, t, m, dt, model = cube()
    N = c.shape[0]
    free = torch.ones(3 * N, dtype=torch.bool)
    v0 = torch.tensor([0.02, 0.0, 0.0], dtype=F64).repeat(N, 1)
    F = torch.zeros(N, 3, dtype=F64)
    F[:, 2] = -0.02 * m
    floor = CR.Surface("plane", [0.0, 0.0, float(c[:, 2].min())], normal=[0, 0, 1], friction=0.3)
    return CR.leapfrog(model, c, m, free, dt, 200, [floor], KAPPA, F=F, v0=v0, energy_every=1, contact_every=1,
                       keep=True)


def test_friction_dissipates():
    out = slide()
    # a node whose sliding the cap has just stopped keeps a tangential velocity at rounding level (1e-16 of its speed)
    # of either sign: measured +5.0e-22 at three sticking steps against -4e-5 while sliding
    fp = out["friction_power"]
    print(f"friction power: min {float(fp.min()):.3e}, max {float(fp.max()):.3e}")
    assert float(fp.max()) <= 1e-14 * float(fp.abs().max()) and float(fp.min()) < 0.0
    bal = out["kinetic"] + out["strain"] + out["contact_energy"] - out["ext_work"]
    print(f"sliding block: balance {float(bal[0]):.3e} -> {float(bal[-1]):.3e}, max {float(bal.max()):.3e}; "
          f"nodes in contact {int(out['in_contact'].min())} .. {int(out['in_contact'].max())}")
    assert float(bal[-1]) < float(bal[0])


def test_friction_is_bounded_and_opposes_sliding_per_node():
    out = slide()
    n = 0
    for recs in out["records"]:
        for r in recs:
            ft = sum(x * x for x in r["ft"]) ** 0.5
            assert ft <= r["mu"] * r["fn"] * (1.0 + 1e-14)
            assert sum(a * b for a, b in zip(r["ft"], r["vt"])) <= 0.0
            n += 1
    assert n > 1000


def test_order_of_surfaces_matters_only_through_friction():
    """Two frictionless surfaces at one node: the swapped list gives the same force; with friction the first surface's
    friction changes the sliding the second sees."""
    c, t, m, dt, model = cube()
    N = c.shape[0]
    free = torch.ones(3 * N, dtype=torch.bool)
    v0 = torch.tensor([0.02, 0.03, -0.01], dtype=F64).repeat(N, 1)
    lo = c.min(0).values
    for mu, same in ((0.0, True), (0.4, False)):
        a = CR.Surface("plane", [0.0, 0.0, float(lo[2]) + 1e-3], normal=[0, 0, 1], friction=mu)
        b = CR.Surface("plane", [float(lo[0]) + 1e-3, 0.0, 0.0], normal=[1, 0, 0], friction=mu)
        f1 = CR.leapfrog(model, c, m, free, dt, 1, [a, b], KAPPA, v0=v0)["FC"][0]
        f2 = CR.leapfrog(model, c, m, free, dt, 1, [b, a], KAPPA, v0=v0)["FC"][0]
        assert float(f1.abs().max()) > 0.0
        assert (float((f1 - f2).abs().max()) <= 1e-15 * float(f1.abs().max())) == same
