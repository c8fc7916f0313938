"""Penalty contact of the explicit dynamics on the device (csrc/explicit.hip k_xd_update_c / k_xd_csum,
system.RigidSurface, ExplicitDynamics.set_contact, solver.explicit_dynamics_solver(contact=...)) against the fp64
restatement tests/contact_ref.py. Helpers and conventions of tests/test_gpu_explicit.py: NaN-tailed device arrays, the
meshes tet1 / kuhn3 / kuhn6 in "unit" scale (E = 1, nu = 0.3, rho = 1), dt = 0.9 x the guaranteed bound, penalty 0.5.

Tolerances:
  force        the start's a_0 and the closing evaluation of a one-step run, as forces m a, per kind (plane, sphere,
               sphere cavity, cylinder, cylinder cavity; mu = 0.3, moving, random v0): <= 1e-12 max|m a_ref| (the
               operator tolerance of test_gpu_explicit.py)
  trajectory   max|u_dev - u_ref| <= 4 n^2 1e-12 max|u_ref| over the whole history, n = 200 steps on kuhn3, 20 on kuhn6:
               the bound of test_gpu_explicit.py, whose premises the contact term keeps (per-step force error at the
               operator tolerance; (omega dt)^2 <= 4 by kappa <= 4 (1 - 0.9^2))
  histories    reaction, penetration and the three contact energy values within the same 4 n^2 1e-12 of the
               restatement's largest; contact counts equal unless the restatement's |g| is below 1e-12 of the mesh size
  bitwise      two runs; run(200) == run(120) + run(80) with a moving surface; recorded rows == the states of a run(1)
               loop; held dofs exactly 0 under contact; surfaces never touched == the run without set_contact (u, v, a
               and the recorded rows; the energy rows are summed per node there, not per dof: 1e-13 relative)

Measured on the MI355X (the tests print them; bound 1.6e-7 for n = 200 steps):
  force, worst case over kinds and meshes: start 2.7e-16, closing evaluation 1.2e-15 of max|m a| (bound 1e-12)
  trajectory, max|u - u_ref| / max|u_ref| over the whole history: oblique 3.7e-14 (linear) / 1.5e-15 (neo_hookean),
      slide 1.0e-14 / 6.6e-15, indent 1.1e-14 / 1.2e-14, callable motion 1.9e-14 / 2.6e-14; closing v <= 2.8e-13,
      closing a <= 1.2e-12 of their largest
  kuhn_cube(6), 20 steps: 1.8e-15 (bound 1.6e-9)
  histories: reaction 4.9e-16 of 3.8e-2, penetration 3.3e-16 of 4.0e-3, contact energy 1.4e-18 of 3.8e-5, friction
      power 3.7e-19 of 3.4e-6, surface power 2.4e-18 of 1.0e-4; every contact count equal
All orders of magnitude below the bounds."""
import functools
import math

import pytest
import torch

import contact_ref as CR
import explicit_ref as XR
import test_gpu_explicit as TX

pytestmark = pytest.mark.gpu

F64 = torch.float64
KAPPA = 0.5
STEPS = 200
MATS = ("linear", "neo_hookean")


@functools.lru_cache(maxsize=None)
def base(name):
    """(coords, tets, m, dt)"""
    c, t, n, E, nu, rho = TX.mesh_of(name, "unit")
    return c, t, XR.lumped_mass(c, t, rho), 0.9 * XR.element_dt(c, t, E, nu, rho)[0]


def rigid(surfs):
    from fem355 import system
    return [system.RigidSurface(**s.kwargs()) for s in surfs]


def free_of(c, fixed):
    free = torch.ones((c.shape[0], 3), dtype=torch.bool)
    if fixed is not None:
        if fixed.dtype == torch.bool:
            free &= ~fixed
        else:
            free[fixed] = False
    return free.view(-1)


def device_run(dev, name, material, surfs, steps, F=None, v0=None, u0=None, fixed=None, chunks=None, energy_every=10,
               contact_every=10, contact=True, rec=None):
    """-> (results per run() call, u, v, a, a_0 of the start)"""
    c, t, m, dt = base(name)
    xd = TX.make(dev, name, "unit", material, fixed)
    try:
        if contact:
            xd.set_contact(rigid(surfs), KAPPA, dt=dt)
        Fd = None if F is None else TX.padded(F, dev)
        xd.start(u0=None if u0 is None else TX.padded(u0, dev), v0=None if v0 is None else TX.padded(v0, dev), F=Fd)
        a0 = xd.a.clone()
        rec = torch.arange(3 * c.shape[0]) if rec is None else rec
        res = [xd.run(k, dt, Fd, 1.0, record=rec, energy_every=energy_every,
                      contact_every=contact_every if contact else 0) for k in (chunks or [steps])]
        return res, xd.u.clone(), xd.v.clone(), xd.a.clone(), a0
    finally:
        xd.close()


def ref_run(name, material, surfs, steps, F=None, v0=None, u0=None, fixed=None, keep=False):
    c, t, m, dt = base(name)
    return CR.leapfrog(TX.model_of(name, "unit", material), c, m, free_of(c, fixed), dt, steps, surfs, KAPPA, F=F,
                       v0=v0, u0=u0, energy_every=10, contact_every=10, keep=keep)


def rand_v(c, scale, seed=5):
    return scale * (2.0 * torch.rand(c.shape, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 1.0)


# ---------------------------------------------------------------- 1. one force evaluation per kind
KINDS = ("plane", "sphere", "sphere_cavity", "cylinder", "cylinder_cavity")
PEN = 0.03


def kind_surface(kind, c):
    """A moving surface of `kind` with mu = 0.3 that a few nodes of the mesh penetrate by up to PEN."""
    mid = c.mean(0)
    top = c[int(c[:, 2].argmax())]
    mv = dict(friction=0.3, velocity=[0.01, 0.0, -0.02])
    if kind == "plane":
        return CR.Surface("plane", [0.0, 0.0, float(c[:, 2].min()) + PEN], normal=[0.1, 0.0, 1.0], **mv)
    if kind == "sphere":
        d = torch.tensor([0.1, 0.05, 0.5], dtype=F64)
        return CR.Surface("sphere", (top + d).tolist(), radius=float(d.norm()) + PEN, **mv)
    if kind == "sphere_cavity":
        return CR.Surface("sphere", mid.tolist(), radius=float((c - mid).norm(dim=1).max()) - PEN, inside=True, **mv)
    ax = torch.tensor([1.0, 0.2, 0.0], dtype=F64) if kind == "cylinder" else torch.tensor([0.1, 0.0, 1.0], dtype=F64)
    ax = ax / ax.norm()
    perp = lambda x: (x - (x @ ax).view(-1, 1) * ax).norm(dim=1)
    if kind == "cylinder":
        d = torch.tensor([0.0, 0.05, 0.5], dtype=F64)
        return CR.Surface("cylinder", (top + d).tolist(), axis=ax.tolist(), radius=float(perp(d.view(1, 3))) + PEN, **mv)
    return CR.Surface("cylinder", mid.tolist(), axis=ax.tolist(), radius=float(perp(c - mid).max()) - PEN, inside=True,
                      **mv)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["tet1", "kuhn3"])
def test_contact_force(gpu, name, kind):
    c, t, m, dt = base(name)
    s = kind_surface(kind, c)
    v0 = rand_v(c, 0.05)
    u0 = rand_v(c, 0.002, seed=6)
    ref = ref_run(name, "linear", [s], 1, v0=v0, u0=u0)
    assert int((ref["FC"][0].view(-1, 3).abs().sum(1) > 0).sum()) >= 1      # the case does touch
    res, u, v, a, a0 = device_run(gpu, name, "linear", [s], 1, v0=v0, u0=u0)
    md = m.repeat_interleave(3)
    for what, dev, r in (("start", a0, ref["A"][0]), ("closing", a, ref["A"][1])):
        assert bool(torch.isfinite(dev).all())
        sc = float((md * r).abs().max())
        d = float((md * (dev.cpu() - r)).abs().max()) / sc
        print(f"contact force {name} {kind} {what}: {d:.2e} of max|m a| = {sc:.3e} (bound {TX.OP_TOL:.0e}); contact "
              f"share of it {float(ref['FC'][0].abs().max()) / sc:.2f}")
        assert d <= TX.OP_TOL
    assert res[0].status == "OK"


# ---------------------------------------------------------------- 2. trajectories
@functools.lru_cache(maxsize=None)
def traj_case(case):
    """(surfaces, kwargs of the runs) on kuhn3"""
    from fem355 import mesh
    c, t, m, dt = base("kuhn3")
    N = c.shape[0]
    zlo = float(c[:, 2].min())
    if case == "oblique":
        v0 = torch.tensor([0.03, 0.0, -0.05], dtype=F64).repeat(N, 1)
        return [CR.Surface("plane", [0.0, 0.0, zlo - 1e-3], normal=[0, 0, 1], friction=0.3)], dict(v0=v0)
    if case == "slide":
        F = torch.zeros(N, 3, dtype=F64)
        F[:, 2] = -0.02 * m
        v0 = torch.tensor([0.02, 0.0, 0.0], dtype=F64).repeat(N, 1)
        return [CR.Surface("plane", [0.0, 0.0, zlo], normal=[0, 0, 1], friction=0.3)], dict(F=F, v0=v0)
    assert case == "indent"
    fixed = mesh.face_nodes(c, 2, 0.0)
    s = CR.Surface("sphere", [0.5, 0.5, float(c[:, 2].max()) + 0.6 + 1e-3], radius=0.6, friction=0.2,
                   velocity=[0.0, 0.0, -0.005])
    return [s], dict(fixed=fixed)


@functools.lru_cache(maxsize=None)
def traj_ref(case, material):
    """The restatement's run, formed once and shared (never modified)."""
    surfs, kw = traj_case(case)
    out = ref_run("kuhn3", material, surfs, STEPS, **kw)
    assert int(out["in_contact"].max()) >= 4                                # the case does touch
    return out


def check_history(res, u, ref, steps, tag):
    U = torch.cat([r.rec_u for r in res] + [u.view(1, -1)]).cpu()
    assert bool(torch.isfinite(U).all())
    um = float(ref["U"].abs().max())
    dev = float((U - ref["U"]).abs().max()) / um
    print(f"{tag}: max|u - u_ref| / max|u_ref| = {dev:.2e} (bound {TX.traj_bound(steps):.1e}), max|u| {um:.3e}")
    assert dev <= TX.traj_bound(steps)


@pytest.mark.parametrize("material", MATS)
@pytest.mark.parametrize("case", ["oblique", "slide", "indent"])
def test_trajectory_parity(gpu, case, material):
    surfs, kw = traj_case(case)
    ref = traj_ref(case, material)
    res, u, v, a, a0 = device_run(gpu, "kuhn3", material, surfs, STEPS, **kw)
    assert res[0].status == "OK" and res[0].steps_done == STEPS
    check_history(res, u, ref, STEPS, f"trajectory {case} {material}")
    for what, x, r in (("v", v, ref["V"][-1]), ("a", a, ref["A"][-1])):
        d = float((x.cpu() - r).abs().max()) / float(r.abs().max())
        print(f"  closing {what}: {d:.2e}")
        assert d <= TX.traj_bound(STEPS)


def test_many_chunks_trajectory(gpu):
    c, t, m, dt = base("kuhn6")
    steps = 20
    s = CR.Surface("sphere", [0.5, 0.5, float(c[:, 2].max()) + 0.6 - 0.05], radius=0.6, friction=0.2,
                   velocity=[0.0, 0.0, -0.005])
    ref = ref_run("kuhn6", "linear", [s], steps)
    assert int(ref["in_contact"][0, 0]) >= 4
    res, u, v, a, a0 = device_run(gpu, "kuhn6", "linear", [s], steps)
    assert res[0].status == "OK" and int(res[0].in_contact[0, 0]) == int(ref["in_contact"][0, 0])
    check_history(res, u, ref, steps, "kuhn6 linear")
    again, u2, _, _, _ = device_run(gpu, "kuhn6", "linear", [s], steps)
    assert torch.equal(u, u2) and torch.equal(res[0].rec_a, again[0].rec_a)
    assert torch.equal(res[0].reaction, again[0].reaction)


# ---------------------------------------------------------------- 3. histories
@pytest.mark.parametrize("case", ["slide", "indent"])
def test_histories(gpu, case):
    c, t, m, dt = base("kuhn3")
    surfs, kw = traj_case(case)
    ref = traj_ref(case, "linear")
    res, u, v, a, a0 = device_run(gpu, "kuhn3", "linear", surfs, STEPS, **kw)
    r = res[0]
    bound = TX.traj_bound(STEPS)
    rows = STEPS // 10
    assert r.reaction.shape == (rows, 1, 3) and r.in_contact.shape == r.penetration.shape == (rows, 1)
    assert r.in_contact.dtype == torch.int64 and r.contact_energy.shape == (rows,)
    assert float((r.t_contact - ref["t_contact"]).abs().max()) <= 1e-12 * float(ref["t_contact"].max())
    for k in ("reaction", "penetration", "contact_energy", "friction_power", "surface_power"):
        sc = float(ref[k].abs().max())
        d = float((getattr(r, k) - ref[k]).abs().max())
        print(f"history {case} {k}: deviation {d:.2e}, largest {sc:.3e} (bound {bound:.1e} of it)")
        assert d <= bound * sc
    U = ref["U"]
    for row in range(rows):
        if int(r.in_contact[row, 0]) != int(ref["in_contact"][row, 0]):
            g = CR.min_abs_gap(surfs, c, U[10 * row], 10 * row * dt)[0]
            print(f"  row {row}: {int(r.in_contact[row, 0])} nodes against {int(ref['in_contact'][row, 0])}, |g| {g:.2e}")
            assert g <= 1e-12
    tot = float((ref["kinetic"] + ref["strain"]).abs().max())
    for k in ("kinetic", "strain", "ext_power", "ext_work"):
        assert float((getattr(r, k) - ref[k]).abs().max()) <= bound * tot
    assert float(r.friction_power.max()) <= 1e-14 * float(r.friction_power.abs().max())
    if case == "indent":
        assert float(r.surface_power.abs().max()) > 0.0
    else:
        assert float(r.surface_power.abs().max()) == 0.0 and int(r.in_contact[1:].min()) >= 4   # row 0: g = 0


# ---------------------------------------------------------------- 4. bitwise properties
def moving_sphere(c, callable_motion):
    """A sphere that starts 0.05 into the top face (its four middle nodes) and moves on down."""
    mv = dict(displacement=lambda tt: [0.0, 1e-3 * math.sin(0.2 * tt), -0.002 * tt]) if callable_motion else \
        dict(velocity=[0.0, 0.0, -0.002])
    return CR.Surface("sphere", [0.5, 0.5, float(c[:, 2].max()) + 0.6 - 0.05], radius=0.6, friction=0.2, **mv)


@pytest.mark.parametrize("material", MATS)
def test_runs_are_reproducible_and_split(gpu, material):
    from fem355 import mesh
    c, t, m, dt = base("kuhn3")
    s = [moving_sphere(c, True)]
    kw = dict(fixed=mesh.face_nodes(c, 2, 0.0), v0=rand_v(c, 0.01))
    one, u1, v1, a1, _ = device_run(gpu, "kuhn3", material, s, STEPS, **kw)
    two, u2, v2, a2, _ = device_run(gpu, "kuhn3", material, s, STEPS, **kw)
    assert int(one[0].in_contact.min()) >= 1
    keys = ("rec_u", "rec_v", "rec_a", "reaction", "in_contact", "penetration", "kinetic", "strain", "contact_energy",
            "friction_power", "surface_power", "t_contact")
    for x, y in ((u1, u2), (v1, v2), (a1, a2)):
        assert torch.equal(x, y)
    for k in keys:
        assert torch.equal(getattr(one[0], k), getattr(two[0], k)), k
    split, u3, v3, a3, _ = device_run(gpu, "kuhn3", material, s, STEPS, chunks=[120, 80], **kw)
    assert [r.first_step for r in split] == [0, 120]
    assert torch.equal(u1, u3) and torch.equal(v1, v3) and torch.equal(a1, a3)
    for k in keys:
        assert torch.equal(getattr(one[0], k), torch.cat([getattr(r, k) for r in split])), k
    ref = ref_run("kuhn3", material, s, STEPS, **kw)                         # the callable's difference quotients
    check_history(one, u1, ref, STEPS, f"callable motion {material}")


def test_recorded_rows_equal_single_steps(gpu):
    from fem355 import mesh
    c, t, m, dt = base("kuhn3")
    steps = 24
    s = rigid([moving_sphere(c, True)])
    fixed = mesh.face_nodes(c, 2, 0.0)
    v0 = TX.padded(rand_v(c, 0.01), gpu)
    rec = torch.tensor([5, 100, 100, 3 * c.shape[0] - 1, 17])
    xd = TX.make(gpu, "kuhn3", "unit", "svk", fixed, 0.1)
    try:
        xd.set_contact(s, KAPPA, dt=dt)
        xd.start(v0=v0)
        long = xd.run(steps, dt, record=rec, contact_every=1)
        assert int(long.in_contact.max()) >= 4
        end = [x.clone() for x in (xd.u, xd.v, xd.a)]
        xd.start(v0=v0)
        for k in range(steps):
            for row, x in ((long.rec_u, xd.u), (long.rec_v, xd.v), (long.rec_a, xd.a)):
                assert torch.equal(row[k], x[rec.to(gpu)]), k
            r1 = xd.run(1, dt, contact_every=1)
            assert r1.first_step == k and r1.status == "OK"
            assert torch.equal(r1.reaction[0], long.reaction[k]) and torch.equal(r1.t_contact, long.t_contact[k: k + 1])
        for x, y in zip(end, (xd.u, xd.v, xd.a)):
            assert torch.equal(x, y)
    finally:
        xd.close()


def test_masked_dofs_stay_zero_under_contact(gpu):
    from fem355 import mesh
    c, t, m, dt = base("kuhn3")
    mask = torch.zeros((c.shape[0], 3), dtype=torch.bool)
    mask[mesh.face_nodes(c, 2, 0.0)] = True
    topn = mesh.face_nodes(c, 2, float(c[:, 2].max()))
    mask[topn, 0] = True                                                    # rollers on the face the sphere presses
    s = [moving_sphere(c, False)]
    res, u, v, a, a0 = device_run(gpu, "kuhn3", "neo_hookean", s, 50, v0=rand_v(c, 0.01), fixed=mask, contact_every=1)
    held = mask.view(-1).to(gpu)
    r = res[0]
    assert int(r.in_contact.max()) >= 4
    for x in (u, v, a, a0):
        assert float(x[held].abs().max()) == 0.0 and bool(torch.isfinite(x).all())
    for x in (r.rec_u, r.rec_v, r.rec_a):
        assert float(x[:, held].abs().max()) == 0.0
    assert float(u.view(-1, 3)[topn, 1:].abs().max()) > 0.0 and r.status == "OK"
    ref = ref_run("kuhn3", "neo_hookean", s, 50, v0=rand_v(c, 0.01), fixed=mask)
    check_history(res, u, ref, 50, "rollers under the sphere")


@pytest.mark.parametrize("material", MATS)
def test_untouched_surfaces_change_no_bit(gpu, material):
    c, t, m, dt = base("kuhn3")
    F, fixed, free, v0, dt2, om1 = TX.traj_case("kuhn3", "unit", "shear")
    assert dt2 == dt
    far = [CR.Surface("plane", [0.0, 0.0, -5.0], normal=[0, 0, 1], friction=0.3),
           CR.Surface("sphere", [0.5, 0.5, 9.0], radius=0.6, velocity=[0.0, 0.0, -0.005])]
    kw = dict(F=F, v0=v0, fixed=fixed)
    plain, u1, v1, a1, s1 = device_run(gpu, "kuhn3", material, far, STEPS, contact=False, **kw)
    con, u2, v2, a2, s2 = device_run(gpu, "kuhn3", material, far, STEPS, **kw)
    assert float(u1.abs().max()) > 0.0 and int(con[0].in_contact.max()) == 0
    for x, y in ((u1, u2), (v1, v2), (a1, a2), (s1, s2)):
        assert torch.equal(x, y)
    for k in ("rec_u", "rec_v", "rec_a", "strain"):
        assert torch.equal(getattr(plain[0], k), getattr(con[0], k)), k
    for k in ("kinetic", "ext_power", "ext_work"):                          # summed per node there, per dof here
        x, y = getattr(plain[0], k), getattr(con[0], k)
        assert float((x - y).abs().max()) <= 1e-13 * float(x.abs().max())
    for k in ("reaction", "penetration", "contact_energy", "friction_power", "surface_power"):
        assert float(getattr(con[0], k).abs().max()) == 0.0


# ---------------------------------------------------------------- 5. two surfaces at one node
def test_two_surfaces_order_rule(gpu):
    c, t, m, dt = base("kuhn3")
    lo = c.min(0).values
    v0 = torch.tensor([-0.03, 0.02, -0.04], dtype=F64).repeat(c.shape[0], 1)
    floor = CR.Surface("plane", [0.0, 0.0, float(lo[2]) + 2e-3], normal=[0, 0, 1], friction=0.4)
    wall = CR.Surface("plane", [float(lo[0]) + 2e-3, 0.0, 0.0], normal=[1, 0, 0], friction=0.4)
    steps = 40
    out = {}
    for tag, surfs in (("floor, wall", [floor, wall]), ("wall, floor", [wall, floor])):
        ref = ref_run("kuhn3", "linear", surfs, steps, v0=v0, keep=True)
        both = {r["node"] for r in ref["records"][0] if r["surface"] == 0} & \
            {r["node"] for r in ref["records"][0] if r["surface"] == 1}
        assert len(both) >= 4                                               # the edge's nodes touch both
        res, u, v, a, a0 = device_run(gpu, "kuhn3", "linear", surfs, steps, v0=v0)
        md = m.repeat_interleave(3)
        d0 = float((md * (a0.cpu() - ref["A"][0])).abs().max()) / float((md * ref["A"][0]).abs().max())
        print(f"{tag}: a_0 {d0:.2e}")
        assert d0 <= TX.OP_TOL
        check_history(res, u, ref, steps, tag)
        out[tag] = (a0.cpu(), ref["A"][0], res[0])
    (a1, r1, h1), (a2, r2, h2) = out["floor, wall"], out["wall, floor"]
    gap_ref = float((r1 - r2).abs().max()) / float(r1.abs().max())
    gap_dev = float((a1 - a2).abs().max()) / float(r1.abs().max())
    print(f"order: the two lists differ by {gap_ref:.2e} (restatement), {gap_dev:.2e} (device)")
    assert gap_ref > 1e-6 and abs(gap_dev - gap_ref) <= 1e-9 * gap_ref
    assert float((h1.reaction[:, 0] - h2.reaction[:, 1]).abs().max()) > 0.0   # the floor's reaction depends on its turn


# ---------------------------------------------------------------- 6. edges
def test_node_on_the_surface_feels_nothing(gpu):
    c, t, m, dt = base("kuhn3")
    j = int(c[:, 2].argmin())
    s = [CR.Surface("plane", c[j].tolist(), normal=[0, 0, 1], friction=0.3),
         CR.Surface("sphere", (c[j] - torch.tensor([0.0, 0.0, 0.25], dtype=F64)).tolist(), radius=0.25)]
    assert CR.gap(s[0], s[0].point, c[j].tolist())[0] == 0.0 and CR.gap(s[1], s[1].point, c[j].tolist())[0] == 0.0
    res, u, v, a, a0 = device_run(gpu, "kuhn3", "linear", s, 1, contact_every=1)
    assert float(a0.abs().max()) == 0.0 and float(u.abs().max()) == 0.0 and float(a.abs().max()) == 0.0
    assert int(res[0].in_contact.max()) == 0 and float(res[0].penetration.max()) == 0.0


def test_centre_and_axis_give_finite_output(gpu):
    c, t, m, dt = base("kuhn3")
    j = 0
    col = torch.nonzero(((c[:, :2] - c[j, :2]).abs().sum(1) == 0)).reshape(-1)
    assert col.numel() >= 2                                                  # the corner's column lies on the axis
    s = [CR.Surface("sphere", c[j].tolist(), radius=0.2, friction=0.3),
         CR.Surface("cylinder", c[j].tolist(), axis=[0, 0, 1], radius=0.2, friction=0.3),
         CR.Surface("sphere", c[j].tolist(), radius=0.2, inside=True, nodes=[j]),
         CR.Surface("cylinder", c[j].tolist(), axis=[0, 0, 1], radius=0.2, inside=True, nodes=col.tolist())]
    ref = ref_run("kuhn3", "linear", s, 3)                                 # at rest: the nodes stay where |r| = 0
    assert float(ref["FC"].abs().max()) == 0.0
    res, u, v, a, a0 = device_run(gpu, "kuhn3", "linear", s, 3, contact_every=1)
    for x in (u, v, a, a0, res[0].rec_a):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) == 0.0
    assert int(res[0].in_contact.max()) == 0 and float(res[0].reaction.abs().max()) == 0.0


def test_orphan_node_and_node_subset(gpu):
    from fem355 import system
    c, t, m, dt = base("kuhn3")
    N = c.shape[0]
    c2 = torch.cat([c, torch.tensor([[0.5, 0.5, -0.5]], dtype=F64)])        # a node of no element, below the floor
    bottom = torch.nonzero(c[:, 2] == c[:, 2].min()).reshape(-1)
    some = bottom[:4]
    floor = system.RigidSurface("plane", [0.0, 0.0, 0.01], normal=[0, 0, 1], friction=0.3,
                                nodes=some.tolist() + [N])
    xd = system.ExplicitDynamics(TX.padded(c2, gpu), TX.padded(t, gpu, 0), 1.0, 1.0, 0.3, "linear")
    try:
        assert float(xd.mass[N]) == 0.0
        xd.set_contact([floor], KAPPA, dt=dt)
        xd.start()
        a0 = xd.a.view(-1, 3).cpu()
        others = torch.ones(N + 1, dtype=torch.bool)
        others[some] = False
        assert float(a0[others].abs().max()) == 0.0                         # the subset alone is pushed (f_int(0) = 0)
        k = KAPPA / (dt * dt)
        assert float((a0[some, 2] - k * 0.01).abs().max()) <= 1e-12 * k * 0.01
        res = xd.run(20, dt, contact_every=1)
        assert res.status == "OK" and int(res.in_contact[0, 0]) == 4        # the orphan is not counted
        for x in (xd.u, xd.v, xd.a):
            assert bool(torch.isfinite(x).all()) and float(x.view(-1, 3)[N].abs().max()) == 0.0
        assert float(xd.u.view(-1, 3)[some, 2].min()) > 0.0
        xd.set_contact(None)                                                 # cleared: the plain run again
        xd.start()
        assert float(xd.a.abs().max()) == 0.0 and xd.run(2, dt).reaction is None
        with pytest.raises(ValueError):
            xd.run(2, dt, contact_every=1)
    finally:
        xd.close()


# ---------------------------------------------------------------- 7. the solver, end to end
def test_solver_end_to_end(gpu):
    from fem355 import solver, system
    c, t, m, dt = base("kuhn3")
    surfs, kw = traj_case("slide")
    steps = 40
    rs = rigid(surfs)
    u, v, a, info = solver.explicit_dynamics_solver(c, t, kw["F"], [], 1.0, 1.0, 0.3, steps, v0=kw["v0"], energy_every=8,
                                                    device=gpu, return_info=True, contact=rs, penalty=KAPPA,
                                                    contact_every=8)
    assert info.status == "OK" and abs(info.dt - dt) <= 1e-12 * dt
    assert info.reaction.shape == (5, 1, 3) and info.contact_energy.shape == (5,)
    xd = system.ExplicitDynamics(c.to(gpu), t.to(gpu), 1.0, 1.0, 0.3, "linear",
                                 torch.zeros(3 * c.shape[0], dtype=torch.uint8, device=gpu))
    try:
        xd.set_contact(rs, KAPPA, dt=info.dt)
        Fd = kw["F"].to(gpu).reshape(-1)
        xd.start(None, kw["v0"].to(gpu), Fd, 1.0)
        res = xd.run(steps, info.dt, Fd, [1.0] * (steps + 1), energy_every=8, contact_every=8)
        assert torch.equal(xd.u.view(-1, 3), u) and torch.equal(xd.v.view(-1, 3), v) and torch.equal(xd.a.view(-1, 3), a)
        for k in ("reaction", "in_contact", "penetration", "contact_energy", "friction_power", "kinetic"):
            assert torch.equal(getattr(res, k), getattr(info, k)), k
    finally:
        xd.close()
    ref = ref_run("kuhn3", "linear", surfs, steps, **kw)
    assert float((u.cpu().view(-1) - ref["U"][-1]).abs().max()) <= TX.traj_bound(steps) * float(ref["U"].abs().max())
    with pytest.raises(ValueError):
        solver.explicit_dynamics_solver(c, t, kw["F"], [], 1.0, 1.0, 0.3, steps, device=gpu, contact=rs, penalty=0.77)
    out = solver.explicit_dynamics_solver(c, t, kw["F"], [], 1.0, 1.0, 0.3, 3, dt=dt, device=gpu, contact=rs,
                                          penalty=0.77)                      # a given dt: the caller's step
    assert len(out) == 3


def test_inverted_element_is_still_reported(gpu):
    import hyperelastic_ref as HR
    c, t, n, E, nu, rho = TX.mesh_of("kuhn3", "unit")
    dt = base("kuhn3")[3]
    e = 80
    a, face = int(t[e, 0]), t[e, 1:]
    u0 = 1e-3 * HR.field("stretch", c, n)
    u0[a] = 1.6 * (c[face].mean(0) - c[a])
    assert bool(HR.Model(c, t, E, nu, "neo_hookean").deformation(u0)[1][e] <= 0)
    floor = [CR.Surface("plane", [0.0, 0.0, 0.01], normal=[0, 0, 1], friction=0.3)]
    res, u, v, acc, a0 = device_run(gpu, "kuhn3", "neo_hookean", floor, 5, u0=u0, contact_every=1)
    assert (res[0].status, res[0].stop_step) == ("INVERTED", 0)
    assert all(bool(torch.isfinite(x).all()) for x in (u, v, acc, a0)) and int(res[0].in_contact[0, 0]) >= 4
