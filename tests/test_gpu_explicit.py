"""Explicit dynamics on the device (csrc/explicit.hip, system.ExplicitDynamics, solver.explicit_dynamics_solver,
element.compute_c3d4_lumped_mass / compute_c3d4_stable_time_step) against the fp64 restatement tests/explicit_ref.py.

Meshes: a single tet, mesh.kuhn_cube(3, jitter=0.15) (162 tets, one chunk), kuhn_cube(6, jitter=0.15) (1296 tets, 343
nodes: several chunks, one of more than MF_PASS = 256 elements -- asserted), and no element at all. Scales: "unit"
(E = 1, nu = 0.3, rho = 1) and "bench" (coordinates x modal_ref.SCALE, MR.E, MR.NU, MR.RHO). The device arrays carry NaN
rows past N and M (coordinates, loads, start vectors) and zero rows past M (connectivity): no NaN comes out.

Tolerances:
  force        per node max deviation <= 1e-12 max|f_int| (the operator tolerance) for the fields random, stretch and,
               for the linear material, rigid; where the exact force is zero (zero field, a rigid motion of the nonlinear
               materials) <= 1e-12 mu max V max|g|, the scale of one element's force at unit strain (the floor of
               test_gpu_nonlinear.py). svk and linear at u = 0: exactly zero. linear vs MatFreeOperator.matvec: 1e-12.
  mass, dt_e   rel <= 1e-12 per entry; device dt <= the dense 2 / omega_max.
  trajectory   max|u_dev - u_ref| <= 4 n^2 1e-12 max|u_ref| over the whole history, n = 200 steps: each step's force
               carries the operator tolerance, a stable scheme does not amplify a perturbation in the energy norm, the
               displacement is a double sum over steps and (omega_max dt)^2 <= 4. The same bound for the damped run,
               the dispersion case and 20 steps on kuhn_cube(6).
  bitwise      two runs; run(200) == run(120) + run(80); recorded rows == the states of a run(1) loop; masked dofs
               exactly 0 (clamped nodes and single-dof rollers).
  energies     kinetic and strain at every 10th step vs the restatement's, <= 4 n^2 1e-12 of its largest kinetic +
               strain; undamped: excursion of kinetic + strain - F.u <= 1.01 x the restatement's own; damped: the
               sampled totals do not increase.
  status       an inverting u0 -> INVERTED at step 0, finite output, the other elements' forces right to 1e-12;
               dt = 1.5 x 2 / omega_max (dense) over 400 steps -> DIVERGED, or max|u| beyond 1e6 max|u0|.

Measured on the MI355X (the tests print them; bound 1.6e-7 for n = 200 steps):
  trajectory, max|u - u_ref| / max|u_ref| over the whole history, worst case over loads, damping and scales:
      linear 2.3e-14, svk 1.8e-15, neo_hookean 1.8e-15 (v: 5.7e-14, 3.8e-14, 7.3e-14; a: 1.2e-13, 7.3e-14, 1.9e-13)
  dispersion: mode 1 1.2e-13 x max|u|, highest mode 2.6e-14 x max|u|
  kuhn_cube(6) (3 chunks of 512, 512, 272 elements), 20 steps: linear 5.2e-16, svk 3.2e-16, neo_hookean 5.0e-16
      (bound 1.6e-9)
  force, worst case in units of its bound's scale: 1.8e-14 (bound 1e-12); mass rel 4.8e-16, dt_e rel 1.0e-15
  energies: worst 3.0e-15 of the largest kinetic + strain (bound 1.6e-7); the undamped excursions agree with the
      restatement's to 7 digits (linear 1.091276e-04, svk 1.410323e-04, neo_hookean 9.933722e-05)
  divergence: DIVERGED at step 370 of 400.
All orders of magnitude below the bounds, as a scheme whose per-step error is a few roundings should be."""
import contextlib
import functools
import io
import math

import pytest
import torch

import explicit_ref as XR
import hyperelastic_ref as HR
import modal_ref as MR
from conftest import rel

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
PAD = 3
MESHES = ("tet1", "kuhn3", "kuhn6")
SCALES = ("unit", "bench")
FIELDS = ("zero", "random", "rigid", "stretch")
OP_TOL = 1e-12
MF_PASS = 256


def traj_bound(n):
    return 4.0 * n * n * 1e-12


@functools.lru_cache(maxsize=None)
def mesh_of(name, scale):
    """(coords, tets, n, E, nu, rho)"""
    from fem355 import mesh
    if name == "tet1":
        c = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.3, 1.1]], dtype=F64)
        t = torch.tensor([[0, 1, 2, 3]], dtype=torch.long)
        n = 1
    else:
        n = int(name[-1])
        c, t = mesh.kuhn_cube(n, jitter=0.15)
        c = c.to(F64)
    if scale == "bench":
        return c * MR.SCALE, t, n, MR.E, MR.NU, MR.RHO
    return c, t, n, 1.0, 0.3, 1.0


def padded(x, dev, fill=NAN):
    """x on the device as a view of a buffer with PAD more rows of `fill` behind it."""
    tail = torch.full((PAD,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    return torch.cat([x, tail]).to(dev)[: x.shape[0]]


def make(dev, name, scale, material, fixed=None, damping=0.0):
    """ExplicitDynamics on NaN-tailed device arrays. fixed: node ids or a bool [N,3] mask."""
    from fem355 import system
    c, t, n, E, nu, rho = mesh_of(name, scale)
    mask = None
    if fixed is not None:
        mask = torch.zeros((c.shape[0], 3), dtype=torch.bool)
        if fixed.dtype == torch.bool:
            mask |= fixed
        else:
            mask[fixed] = True
        mask = padded(mask.to(torch.uint8).view(-1), dev, 1)
    return system.ExplicitDynamics(padded(c, dev), padded(t, dev, 0), rho, E, nu, material, mask, damping)


@functools.lru_cache(maxsize=None)
def model_of(name, scale, material):
    c, t, n, E, nu, rho = mesh_of(name, scale)
    return XR.Model(c, t, E, nu, material)


@functools.lru_cache(maxsize=None)
def force_ref(name, scale, material, fld):
    c, t, n, E, nu, rho = mesh_of(name, scale)
    u = HR.field(fld, c, n)
    return u, model_of(name, scale, material).f_int(u.reshape(-1)).detach().view(-1, 3)


# ---------------------------------------------------------------- 0. the layout covers the pass boundary
def test_layout_covers_chunks_and_passes(gpu):
    xd = make(gpu, "kuhn6", "unit", "linear")
    try:
        info = xd.op.info()
        cptr = xd.op.layout()[1].cpu()
        sizes = cptr[1:] - cptr[:-1]
        print(f"kuhn6: {info['chunks']} chunks, sizes {sizes.tolist()}")
        assert info["chunks"] >= 2 and int(sizes.max()) > MF_PASS
        one = make(gpu, "kuhn3", "unit", "linear")
        assert one.op.info()["chunks"] == 1
        one.close()
    finally:
        xd.close()


# ---------------------------------------------------------------- 1. one force evaluation
WORST = {}


@pytest.mark.parametrize("material", XR.MATERIALS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", MESHES)
def test_internal_force(gpu, name, scale, material):
    c, t, n, E, nu, rho = mesh_of(name, scale)
    lam, mu = HR.lame(E, nu)
    g, V = HR.geometry(c, t)
    floor = mu * float(V.max()) * float(g.abs().max())
    xd = make(gpu, name, scale, material)
    try:
        for fld in FIELDS:
            u, ref = force_ref(name, scale, material, fld)
            ud = padded(u, gpu)
            f = xd.internal_force(ud).view(-1, 3)
            assert bool(torch.isfinite(f).all())
            exact_zero = fld == "zero" or (fld == "rigid" and material != "linear")
            sc = floor if exact_zero else float(ref.abs().max())
            dev = float((f.cpu() - ref).abs().max()) / sc
            WORST["force"] = max(WORST.get("force", 0.0), dev)
            print(f"force {name} {scale} {material} {fld}: {dev:.2e} of the scale (bound {OP_TOL:.0e})")
            assert dev <= OP_TOL
            if fld == "zero" and material != "neo_hookean":
                assert float(f.abs().max()) == 0.0
            if material == "linear":
                assert rel(f.view(-1), xd.op.matvec(ud)) <= OP_TOL or float(ref.abs().max()) == 0.0
            # through the integrator: a_0 m = -f_int with no load, v0 = 0
            xd.start(u0=ud)
            a = (xd.a.view(-1, 3) * xd.mass.view(-1, 1)).cpu()
            assert float((a + ref).abs().max()) <= OP_TOL * sc
            assert xd.status() == ("OK", -1)
    finally:
        xd.close()


# ---------------------------------------------------------------- 2. lumped mass and step size
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", MESHES)
def test_mass_and_step(gpu, name, scale):
    from fem355 import element
    c, t, n, E, nu, rho = mesh_of(name, scale)
    m_ref = XR.lumped_mass(c, t, rho)
    dt_ref, dte_ref = XR.element_dt(c, t, E, nu, rho)
    xd = make(gpu, name, scale, "linear")
    try:
        dt, dte = xd.stable_dt()
        dm = float(((xd.mass.cpu() - m_ref).abs() / m_ref).max())
        dd = float(((dte.cpu() - dte_ref).abs() / dte_ref).max())
        print(f"{name} {scale}: mass rel {dm:.2e}  dt_e rel {dd:.2e}  dt {dt:.6e}")
        assert dm <= 1e-12 and dd <= 1e-12
        assert dt == float(dte.min()) and abs(dt - dt_ref) <= 1e-12 * dt_ref
        m2 = element.compute_c3d4_lumped_mass(c, t, rho, device=gpu)
        dt2, dte2 = element.compute_c3d4_stable_time_step(c, t, E, nu, rho, device=gpu)
        assert torch.equal(m2, xd.mass) and dt2 == dt and torch.equal(dte2, dte)
        assert element.compute_c3d4_lumped_mass(c, t, rho, device=gpu, dtype=torch.float32).dtype == torch.float32
        if name != "kuhn6" or scale == "unit":
            assert dt <= 2.0 / XR.omega_max(c, t, E, nu, rho)
    finally:
        xd.close()


def test_no_elements(gpu):
    from fem355 import element, solver
    c = torch.rand(5, 3, dtype=F64)
    t = torch.zeros((0, 4), dtype=torch.long)
    assert float(element.compute_c3d4_lumped_mass(c, t, 2.0, device=gpu).abs().max()) == 0.0
    dt, dte = element.compute_c3d4_stable_time_step(c, t, 1.0, 0.3, 1.0, device=gpu)
    assert dt == float("inf") and dte.numel() == 0
    u, v, a = solver.explicit_dynamics_solver(c, t, torch.ones(5, 3, dtype=F64), [], 1.0, 1.0, 0.3, 5, device=gpu)
    assert all(float(x.abs().max()) == 0.0 for x in (u, v, a))


# ---------------------------------------------------------------- 3. trajectory parity
STEPS = 200


@functools.lru_cache(maxsize=None)
def traj_case(name, scale, load):
    """(F [N,3], fixed ids, free [3N], v0 [N,3], dt, omega_1) -- the load scaled by E x the loaded area so that both
    scales strain alike; the bench column is twice as long and 0.7 wide, so the same transverse traction bends it
    ~4 x as far (L^3 / I is ~11 x the cube's, the shear term 2 x): its shear load is quartered."""
    c, t, n, E, nu, rho = mesh_of(name, scale)
    area = 1.0 if scale == "unit" else float(MR.SCALE[0] * MR.SCALE[1])
    bend = 0.25 if (scale == "bench" and load == "shear") else 1.0
    F, fixed = HR.solver_case(c, load, scale=E * area * bend)
    free = torch.ones((c.shape[0], 3), dtype=torch.bool)
    free[fixed] = False
    free = free.view(-1)
    v0 = 0.02 * math.sqrt(E / rho) * (2.0 * torch.rand(c.shape, dtype=F64, generator=torch.Generator().manual_seed(11))
                                      - 1.0)
    dt = 0.9 * XR.element_dt(c, t, E, nu, rho)[0]
    om1 = float(XR.modes(c, t, E, nu, rho, free)[0][0]) if name == "kuhn3" else 0.0
    return F, fixed, free, v0, dt, om1


@functools.lru_cache(maxsize=None)
def traj_ref(name, scale, load, material, damped, steps=STEPS):
    """The restatement's run, formed once and shared (never modified)."""
    c, t, n, E, nu, rho = mesh_of(name, scale)
    F, fixed, free, v0, dt, om1 = traj_case(name, scale, load)
    alpha = 0.5 * om1 if damped else 0.0
    out = XR.leapfrog(model_of(name, scale, material), XR.lumped_mass(c, t, rho), free, dt, steps, F=F, v0=v0,
                      alpha=alpha, energy_every=10)
    if material != "linear":   # the case itself is sound: no element of the restatement's run comes near inversion
        hr = model_of(name, scale, material).hr
        assert min(float(hr.deformation(u.view(-1, 3))[1].min()) for u in out["U"][::10]) > 0.2
    return out, alpha


def device_run(dev, name, scale, load, material, damped, steps=STEPS, chunks=None, energy_every=10):
    """The same run on the device with every dof recorded -> (results per run() call, final u, v, a)."""
    c, t, n, E, nu, rho = mesh_of(name, scale)
    F, fixed, free, v0, dt, om1 = traj_case(name, scale, load)
    alpha = 0.5 * om1 if damped else 0.0
    xd = make(dev, name, scale, material, fixed, alpha)
    try:
        Fd = padded(F, dev)
        xd.start(v0=padded(v0, dev), F=Fd)
        rec = torch.arange(3 * c.shape[0])
        res = [xd.run(k, dt, Fd, 1.0, record=rec, energy_every=energy_every) for k in (chunks or [steps])]
        return res, xd.u.clone(), xd.v.clone(), xd.a.clone()
    finally:
        xd.close()


def history(res, u):
    """[steps + 1, 3N]: the recorded u rows of consecutive runs and the state reached."""
    return torch.cat([r.rec_u for r in res] + [u.view(1, -1)]).cpu()


@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("material", XR.MATERIALS)
@pytest.mark.parametrize("load", ["pull", "shear"])
@pytest.mark.parametrize("scale", SCALES)
def test_trajectory_parity(gpu, scale, load, material, damped):
    ref, alpha = traj_ref("kuhn3", scale, load, material, damped)
    res, u, v, a = device_run(gpu, "kuhn3", scale, load, material, damped)
    assert res[0].status == "OK" and res[0].stop_step == -1 and res[0].steps_done == STEPS
    U = history(res, u)
    assert bool(torch.isfinite(U).all())
    um = float(ref["U"].abs().max())
    dev = float((U - ref["U"]).abs().max()) / um
    dv = float((torch.cat([res[0].rec_v.cpu(), v.cpu().view(1, -1)]) - ref["V"]).abs().max()) / \
        float(ref["V"].abs().max())
    da = float((torch.cat([res[0].rec_a.cpu(), a.cpu().view(1, -1)]) - ref["A"]).abs().max()) / \
        float(ref["A"].abs().max())
    print(f"trajectory {scale} {load} {material} alpha {alpha:.3e}: max|u - u_ref| / max|u_ref| = {dev:.2e} "
          f"(bound {traj_bound(STEPS):.1e}), v {dv:.2e}, a {da:.2e}, max|u| {um:.3e}")
    assert dev <= traj_bound(STEPS)
    assert dv <= traj_bound(STEPS) and da <= traj_bound(STEPS)


# ---------------------------------------------------------------- 4. exact discrete dispersion
@pytest.mark.parametrize("j", [0, -1])
def test_discrete_dispersion(gpu, j):
    from fem355 import mesh
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    fixed = mesh.face_nodes(c, 2, 0.0)
    free = torch.ones((c.shape[0], 3), dtype=torch.bool)
    free[fixed] = False
    om, Phi = XR.modes(c, t, E, nu, rho, free.view(-1))
    dt = 0.9 * XR.element_dt(c, t, E, nu, rho)[0]
    wh = 2.0 * math.asin(0.5 * float(om[j]) * dt) / dt
    k = torch.arange(STEPS + 1, dtype=F64)
    exact = torch.cos(wh * k * dt).view(-1, 1) * Phi[:, j].view(1, -1)
    xd = make(gpu, "kuhn3", "unit", "linear", fixed)
    try:
        xd.start(u0=padded(Phi[:, j].contiguous(), gpu))
        res = xd.run(STEPS, dt, record=torch.arange(3 * c.shape[0]))
        U = history([res], xd.u)
    finally:
        xd.close()
    dev = float((U - exact).abs().max()) / float(exact.abs().max())
    print(f"dispersion mode {j}: omega dt / 2 = {0.5 * float(om[j]) * dt:.4f}, deviation {dev:.2e} x max|u| "
          f"(bound {traj_bound(STEPS):.1e})")
    assert res.status == "OK" and dev <= traj_bound(STEPS)


# ---------------------------------------------------------------- 5. bitwise properties
@pytest.mark.parametrize("material", XR.MATERIALS)
def test_runs_are_reproducible_and_split(gpu, material):
    one, u1, v1, a1 = device_run(gpu, "kuhn3", "unit", "pull", material, True)
    two, u2, v2, a2 = device_run(gpu, "kuhn3", "unit", "pull", material, True)
    for x, y in ((u1, u2), (v1, v2), (a1, a2), (one[0].rec_u, two[0].rec_u), (one[0].rec_v, two[0].rec_v),
                 (one[0].rec_a, two[0].rec_a)):
        assert torch.equal(x, y)
    for k in ("kinetic", "strain", "ext_power", "ext_work", "t_energy"):
        assert torch.equal(getattr(one[0], k), getattr(two[0], k))
    split, u3, v3, a3 = device_run(gpu, "kuhn3", "unit", "pull", material, True, chunks=[120, 80])
    assert [r.first_step for r in split] == [0, 120]
    assert torch.equal(u1, u3) and torch.equal(v1, v3) and torch.equal(a1, a3)
    for k in ("rec_u", "rec_v", "rec_a"):
        assert torch.equal(getattr(one[0], k), torch.cat([getattr(r, k) for r in split]))
    for k in ("kinetic", "strain", "ext_work"):
        assert torch.equal(getattr(one[0], k), torch.cat([getattr(r, k) for r in split]))


def test_recorded_rows_equal_single_steps(gpu):
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    F, fixed, free, v0, dt, om1 = traj_case("kuhn3", "unit", "shear")
    steps = 24
    amps = [math.sin(0.3 * k) for k in range(steps + 1)]
    rec = torch.tensor([5, 100, 100, 3 * c.shape[0] - 1, 17])
    xd = make(gpu, "kuhn3", "unit", "svk", fixed, 0.1)
    try:
        Fd = padded(F, gpu)
        xd.start(v0=padded(v0, gpu), F=Fd, amp=amps[0])
        long = xd.run(steps, dt, Fd, amps, record=rec)
        assert long.rec_u.shape == (steps, 5)
        end = [x.clone() for x in (xd.u, xd.v, xd.a)]
        xd.start(v0=padded(v0, gpu), F=Fd, amp=amps[0])
        for k in range(steps):
            for row, x in ((long.rec_u, xd.u), (long.rec_v, xd.v), (long.rec_a, xd.a)):
                assert torch.equal(row[k], x[rec.to(gpu)]), k
            r1 = xd.run(1, dt, Fd, amps[k: k + 2])
            assert r1.first_step == k and r1.status == "OK"
        for x, y in zip(end, (xd.u, xd.v, xd.a)):
            assert torch.equal(x, y)
    finally:
        xd.close()


def test_masked_dofs_stay_zero(gpu):
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    F, fixed, free, v0, dt, om1 = traj_case("kuhn3", "unit", "pull")
    mask = torch.zeros((c.shape[0], 3), dtype=torch.bool)
    mask[fixed] = True                                  # clamped nodes
    roller = torch.nonzero(c[:, 0] == c[:, 0].max()).reshape(-1)
    mask[roller, 0] = True                              # rollers: x held on the face x = max
    xd = make(gpu, "kuhn3", "unit", "neo_hookean", mask, 0.05)
    try:
        full = 0.1 * torch.ones_like(F) * F.abs().max()   # a load on every dof, the held ones included
        u0 = 0.01 * torch.ones_like(F)
        xd.start(u0=padded(u0, gpu), v0=padded(v0, gpu), F=padded(full, gpu))
        res = xd.run(50, dt, padded(full, gpu), 1.0, record=torch.arange(3 * c.shape[0]))
        held = mask.view(-1).to(gpu)
        for x in (xd.u, xd.v, xd.a):
            assert float(x[held].abs().max()) == 0.0 and bool(torch.isfinite(x).all())
        for x in (res.rec_u, res.rec_v, res.rec_a):
            assert float(x[:, held].abs().max()) == 0.0
        assert float(xd.u.view(-1, 3)[roller, 1:].abs().max()) > 0.0 and res.status == "OK"
    finally:
        xd.close()


@pytest.mark.parametrize("material", XR.MATERIALS)
def test_many_chunks_trajectory(gpu, material):
    steps = 20
    ref, _ = traj_ref("kuhn6", "unit", "shear", material, False, steps)
    res, u, v, a = device_run(gpu, "kuhn6", "unit", "shear", material, False, steps)
    U = history(res, u)
    dev = float((U - ref["U"]).abs().max()) / float(ref["U"].abs().max())
    print(f"kuhn6 {material}: {dev:.2e} (bound {traj_bound(steps):.1e})")
    assert res[0].status == "OK" and dev <= traj_bound(steps)
    again, u2, _, _ = device_run(gpu, "kuhn6", "unit", "shear", material, False, steps)
    assert torch.equal(u, u2) and torch.equal(res[0].rec_a, again[0].rec_a)


# ---------------------------------------------------------------- 6. energies
@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("material", XR.MATERIALS)
def test_energies(gpu, material, damped):
    ref, alpha = traj_ref("kuhn3", "unit", "pull", material, damped)
    res, u, v, a = device_run(gpu, "kuhn3", "unit", "pull", material, damped)
    r = res[0]
    assert torch.equal(r.t_energy, ref["t"]) and r.kinetic.numel() == STEPS // 10
    total_ref = float((ref["kinetic"] + ref["strain"]).abs().max())
    worst = 0.0
    for k in ("kinetic", "strain", "ext_power", "ext_work"):
        d = float((getattr(r, k) - ref[k]).abs().max()) / total_ref
        worst = max(worst, d)
    print(f"energies {material} alpha {alpha:.3f}: worst deviation {worst:.2e} of max(kinetic + strain) "
          f"(bound {traj_bound(STEPS):.1e})")
    assert worst <= traj_bound(STEPS)
    tot = r.kinetic + r.strain - r.ext_work
    tot_ref = ref["kinetic"] + ref["strain"] - ref["ext_work"]
    if damped:
        assert bool((tot[1:] <= tot[:-1]).all())
    else:
        exc, exc_ref = float(tot.max() - tot.min()), float(tot_ref.max() - tot_ref.min())
        print(f"  excursion of the total {exc:.6e}, the restatement's {exc_ref:.6e}")
        assert exc <= 1.01 * exc_ref


# ---------------------------------------------------------------- 7. status words
@pytest.mark.parametrize("material", ["svk", "neo_hookean"])
def test_inverted_element_is_reported(gpu, material):
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    hr = HR.Model(c, t, E, nu, material)
    e = 80
    a, face = int(t[e, 0]), t[e, 1:]
    u0 = 1e-3 * HR.field("stretch", c, n)
    u0[a] = 1.6 * (c[face].mean(0) - c[a])              # node a pushed through the opposite face of element e
    detF = hr.deformation(u0)[1]
    bad = detF <= 0
    assert bool(bad[e]) and not bool(bad.all())
    fe = hr.element_forces_tangents(u0)[0]
    fe = torch.where(bad.view(-1, 1, 1), torch.zeros_like(fe), fe)
    ref = torch.zeros_like(c).index_add_(0, t.reshape(-1), fe.reshape(-1, 3))
    xd = make(gpu, "kuhn3", "unit", material)
    try:
        f = xd.internal_force(padded(u0, gpu)).view(-1, 3).cpu()
        assert bool(torch.isfinite(f).all())
        assert float((f - ref).abs().max()) <= OP_TOL * float(ref.abs().max())
        xd.start(u0=padded(u0, gpu))
        assert xd.status() == ("INVERTED", 0) and bool(torch.isfinite(xd.a).all())
        res = xd.run(5, 0.5 * xd.stable_dt()[0])
        assert (res.status, res.stop_step) == ("INVERTED", 0)
        assert all(bool(torch.isfinite(x).all()) for x in (xd.u, xd.v, xd.a))
        xd.start()                                       # a fresh start clears the words
        assert xd.run(3, 0.5 * xd.stable_dt()[0]).status == "OK"
    finally:
        xd.close()


def test_unstable_step_is_reported_not_raised(gpu):
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    dt = 1.5 * 2.0 / XR.omega_max(c, t, E, nu, rho)
    u0 = HR.field("random", c, n)
    xd = make(gpu, "kuhn3", "unit", "linear")
    try:
        xd.start(u0=padded(u0, gpu))
        res = xd.run(400, dt)
        grown = float(torch.nan_to_num(xd.u.abs(), nan=math.inf).max())
        print(f"dt = 1.5 x 2 / omega_max: status {res.status} at step {res.stop_step}, max|u| {grown:.3e}")
        assert res.steps_done == 400
        assert res.status == "DIVERGED" or grown > 1e6 * float(u0.abs().max())
        if res.status == "DIVERGED":
            assert 0 <= res.stop_step < 400
    finally:
        xd.close()


# ---------------------------------------------------------------- 8. the solver, end to end
def test_solver_end_to_end(gpu):
    from fem355 import solver
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    F, fixed, free, v0, dt, om1 = traj_case("kuhn3", "unit", "pull")
    steps = 40
    ramp = lambda tt: min(1.0, 1.5 * tt)
    rec = torch.tensor([63, 10])
    kw = dict(material="svk", v0=v0, damping=0.1, record=rec, energy_every=8, device=gpu, return_info=True)
    u2, v2, a2, info2 = solver.explicit_dynamics_solver(c, t, F, fixed, rho, E, nu, steps, amplitude=ramp, **kw)
    assert abs(info2.dt - dt) <= 1e-12 * dt               # dt=None: 0.9 x stable_dt()
    amps = torch.tensor([ramp(k * info2.dt) for k in range(steps + 1)], dtype=F64)
    assert 0.0 == float(amps[0]) < float(amps[3]) < float(amps[-1]) == 1.0
    u, v, a, info = solver.explicit_dynamics_solver(c, t, F, fixed, rho, E, nu, steps, amplitude=amps, **kw)
    assert info.dt == info2.dt
    assert info.status == "OK" and info.steps_done == steps
    assert u.shape == v.shape == a.shape == (c.shape[0], 3) and u.dtype == F64
    assert info.rec_u.shape == info.rec_v.shape == info.rec_a.shape == (steps + 1, 2, 3)
    assert torch.equal(info.rec_u[-1].cpu(), u[rec].cpu()) and torch.equal(info.rec_a[-1].cpu(), a[rec].cpu())
    assert info.kinetic.shape == info.strain.shape == info.t_energy.shape == (5,)
    assert torch.equal(u, u2) and torch.equal(v, v2) and torch.equal(a, a2)
    assert torch.equal(info.rec_v, info2.rec_v) and torch.equal(info.strain, info2.strain)
    # against the restatement
    ref = XR.leapfrog(model_of("kuhn3", "unit", "svk"), XR.lumped_mass(c, t, rho), free, dt, steps, F=F, amps=amps,
                      v0=v0, alpha=0.1)
    assert float((u.cpu().view(-1) - ref["U"][-1]).abs().max()) <= traj_bound(steps) * float(ref["U"].abs().max())
    # a given dt is used as is; float32 comes back as float32; a per-dof mask for `fixed`
    mask = torch.zeros((c.shape[0], 3), dtype=torch.bool)
    mask[fixed] = True
    u3, v3, a3, info3 = solver.explicit_dynamics_solver(c, t, F, mask, rho, E, nu, 10, dt=0.5 * dt, dtype=torch.float32,
                                                        device=gpu, return_info=True)
    assert info3.dt == 0.5 * dt and u3.dtype == v3.dtype == a3.dtype == torch.float32
    assert float(u3[fixed].abs().max()) == 0.0
    out = solver.explicit_dynamics_solver(c, t, F, fixed, rho, E, nu, 3, device=gpu)
    assert len(out) == 3


def test_solver_reports_divergence(gpu):
    from fem355 import solver
    c, t, n, E, nu, rho = mesh_of("kuhn3", "unit")
    F, fixed, free, v0, dt, om1 = traj_case("kuhn3", "unit", "pull")
    big = 1.5 * 2.0 / XR.omega_max(c, t, E, nu, rho, free)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        u, v, a, info = solver.explicit_dynamics_solver(c, t, F, fixed, rho, E, nu, 400, dt=big, v0=v0, device=gpu,
                                                        return_info=True)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Explicit solver:")]
    assert info.status == "DIVERGED" and len(lines) == 1 and "DIVERGED" in lines[0]
