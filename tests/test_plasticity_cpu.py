"""CPU tier of the elastoplastic c3d4 path: the restatement of tests/plasticity_ref.py against itself (the closed-form
consistent tangent against central differences of the stress, the element force against the gradient of the incremental
potential, the elastic branch against the linear stiffness of oracle.ref_cpu), the uniaxial analytic case on its direct
Newton, the properties the device tests rely on (branch margins and plastic fractions of the test fields, the sizing of
the solver cases) and the argument checks of the public functions. No device call."""
import math

import pytest
import torch

import modal_ref as MR
import plasticity_ref as PR
from conftest import rel
from oracle import ref_cpu as R

F64 = torch.float64


def _mesh(n, scale="unit"):
    from fem355 import mesh
    c, t = mesh.kuhn_cube(n, jitter=0.15)
    c = c.to(F64)
    return (c * MR.SCALE if scale == "bench" else c), t


def _model(n, scale="unit"):
    c, t = _mesh(n, scale)
    return PR.Model(c, t, *PR.material(scale))


def _random_strain(M, size, seed):
    A = size * (2.0 * torch.rand(M, 3, 3, dtype=F64, generator=torch.Generator().manual_seed(seed)) - 1.0)
    return 0.5 * (A + A.transpose(1, 2))


def _hardened(mu, kappa, sy, H, ey, M):
    o = PR.update(_random_strain(M, 3.0 * ey, 21), torch.zeros(M, 3, 3, dtype=F64), torch.zeros(M, dtype=F64), mu,
                  kappa, sy, H)
    assert bool(o["plastic"].all())
    return o["ep"], o["alpha"]


@pytest.mark.parametrize("start", ("virgin", "hardened"))
@pytest.mark.parametrize("scale", ("unit", "bench"))
def test_closed_form_tangent_matches_central_differences_of_the_stress(scale, start):
    E, nu, sy, H = PR.material(scale)
    mu, kappa = PR.moduli(E, nu)
    ey, M = PR.yield_strain(E, nu, sy), 16
    ep_n, al_n = (torch.zeros(M, 3, 3, dtype=F64), torch.zeros(M, dtype=F64)) if start == "virgin" else \
        _hardened(mu, kappa, sy, H, ey, M)
    eps = _random_strain(M, 4.0 * ey, 22)
    o = PR.update(eps, ep_n, al_n, mu, kappa, sy, H)
    assert bool(o["plastic"].all())
    # yield consistency after the return: sqrt(3/2) |s| = sigma_y + H alpha
    q = math.sqrt(1.5) * torch.sqrt((o["s"] * o["s"]).sum((1, 2)))
    assert float(((q - (sy + H * o["alpha"])).abs() / sy).max()) <= 1e-13
    Cm = PR.tangent_moduli(o, mu, kappa, H)
    h = 1e-6 * ey
    fd = torch.zeros_like(Cm)
    for k in range(3):
        for l in range(3):
            d = torch.zeros(3, 3, dtype=F64)
            d[k, l] += 0.5 * h
            d[l, k] += 0.5 * h
            fd[:, :, :, k, l] = (PR.update(eps + d, ep_n, al_n, mu, kappa, sy, H)["sigma"]
                                 - PR.update(eps - d, ep_n, al_n, mu, kappa, sy, H)["sigma"]) / (2.0 * h)
    assert float((fd - Cm).abs().max() / Cm.abs().max()) <= 1e-6
    # major and minor symmetries of C
    assert float((Cm - Cm.permute(0, 3, 4, 1, 2)).abs().max() / Cm.abs().max()) <= 1e-15
    assert float((Cm - Cm.permute(0, 2, 1, 3, 4)).abs().max() / Cm.abs().max()) <= 1e-15


@pytest.mark.parametrize("start", ("virgin", "hardened"))
@pytest.mark.parametrize("fld", ("small", "large", "graded"))
def test_force_is_the_gradient_of_the_incremental_potential(fld, start):
    m = _model(2)
    st = None if start == "virgin" else PR.hardened_state(m, 2)
    u = PR.field(fld, m.coords, 2, PR.yield_strain(m.E, m.nu, m.sigma_y))
    el = m.element(u, st)
    ue = u[m.tets].clone().requires_grad_(True)
    g = torch.autograd.grad(m.element_potential(ue, st).sum(), ue)[0]
    assert float((g - el["fe"]).abs().max() / el["fe"].abs().max()) <= 1e-6
    Kt = el["Kt"]
    assert float((Kt - Kt.transpose(1, 2)).abs().max() / Kt.abs().max()) <= 1e-14
    # the element tangent is the derivative of the element force (central differences in the 12 displacements)
    h = 1e-6 * PR.yield_strain(m.E, m.nu, m.sigma_y)
    fd = torch.zeros_like(Kt)
    for j in range(12):
        d = torch.zeros(m.M, 12, dtype=F64)
        d[:, j] = h
        up, dn = (u[m.tets] + s * d.view(-1, 4, 3) for s in (1.0, -1.0))
        ep_n, al_n = m._state(st)
        f = lambda x: (m.V.view(-1, 1, 1) * torch.einsum(
            "mij,maj->mai", PR.update(m.strain_of(x), ep_n, al_n, m.mu, m.kappa, m.sigma_y, m.H)["sigma"],
            m.g)).reshape(m.M, 12)
        fd[:, :, j] = (f(up) - f(dn)) / (2.0 * h)
    assert float(((fd - Kt).abs().amax((1, 2)) / Kt.abs().amax((1, 2))).max()) <= 1e-6


@pytest.mark.parametrize("scale", ("unit", "bench"))
def test_elastic_branch_is_the_linear_stiffness(scale):
    m = _model(3, scale)
    ey = PR.yield_strain(m.E, m.nu, m.sigma_y)
    K0 = R.tet4_K(m.coords, m.tets, m.E, m.nu)
    for fld in ("zero", "small"):
        el = m.element(PR.field(fld, m.coords, 3, ey))
        assert not bool(el["plastic"].any())
        assert rel(el["Kt"], K0) <= 1e-12
        assert float(el["ep"].abs().max()) == 0.0 and float(el["alpha"].abs().max()) == 0.0
    u = PR.field("small", m.coords, 3, ey)
    assert rel(m.f_int(u), R.nodal_forces(K0, m.tets, u)) <= 1e-12


@pytest.mark.parametrize("scale", ("unit", "bench"))
@pytest.mark.parametrize("name", ("kuhn3", "kuhn2"))
def test_fields_keep_their_class_and_stay_off_the_branch_cut(name, scale):
    """What tests/test_gpu_plasticity.py relies on: `small` is elastic everywhere, `large` yields everywhere, `graded`
    yields in 25-75 % of the elements, and |f_tr| >= 1e-6 sigma_y in every element, from both start states."""
    n = int(name[-1])
    m = _model(n, scale)
    ey = PR.yield_strain(m.E, m.nu, m.sigma_y)
    hard = PR.hardened_state(m, n)
    assert 0.25 <= float((hard[1] > 0).to(F64).mean()) <= 0.75
    for st in (None, hard):
        for fld in PR.FIELDS:
            el = m.element(PR.field(fld, m.coords, n, ey), st, tangent=False)
            frac = float(el["plastic"].to(F64).mean())
            assert float(el["f_tr"].abs().min()) >= 1e-6 * m.sigma_y, (fld, st is None)
            assert {"zero": frac == 0.0, "small": frac == 0.0, "large": frac == 1.0,
                    "graded": 0.25 <= frac <= 0.75}[fld], (fld, frac)


def _trace_over_norm(state):
    """max |tr ep| / |ep| over the elements that have yielded, |ep| the tensor norm of the contract's |s_tr|."""
    ep = state[0][state[1] > 0]
    norm = torch.sqrt((ep[:, :3] ** 2).sum(1) + 2.0 * (ep[:, 3:] ** 2).sum(1))
    return float(((ep[:, 0] + ep[:, 1] + ep[:, 2]).abs() / norm).max())


@pytest.mark.parametrize("scale", ("unit", "bench"))
@pytest.mark.parametrize("n", (2, 3))
def test_plastic_strain_stays_traceless(n, scale):
    """On the states the device tests compare: one update from the virgin and from the hardened state."""
    m = _model(n, scale)
    ey = PR.yield_strain(m.E, m.nu, m.sigma_y)
    for st in (None, PR.hardened_state(m, n)):
        for fld in ("large", "graded"):
            assert _trace_over_norm(m.next_state(PR.field(fld, m.coords, n, ey), st)) <= 1e-15


def test_uniaxial_analytic_case_on_the_direct_newton():
    m, F, mask, exact, pl = PR.uniaxial_case(*_mesh(2))
    assert abs(float(F.sum()) - 2.0 * m.sigma_y) <= 1e-15     # unit face area
    tol = 1e-10
    u, st, info = PR.newton(m, F, mask, (0.5, 1.0, 0.0), tol=tol)
    assert info["converged"]
    free = ~mask.reshape(-1)
    lam_min = float(torch.linalg.eigvalsh(m.dense_tangent(u, st)[free][:, free])[0])
    bound = 2.0 * tol * float(F.reshape(-1)[free].norm()) / lam_min
    for k in range(3):
        dev = float((info["u_steps"][k] - exact[k]).abs().max())
        print(f"step {k + 1}: max|u - u_exact| {dev:.2e} (bound {bound:.2e})")
        assert dev <= bound
    sig = m.element(info["u_steps"][1], info["states"][0], tangent=False)["sigma"]
    t = 2.0 * m.sigma_y
    want = torch.zeros(6, dtype=F64)
    want[0] = t
    assert float((sig - want).abs().max()) <= 1e-9 * t
    assert float((info["states"][1][1] - pl).abs().max()) <= 1e-9 * pl
    assert float(m.element(u, st, tangent=False)["sigma"].abs().max()) <= 1e-9 * t
    assert info["plastic_fraction"][1] == 1.0 and info["plastic_fraction"][2] == 0.0


@pytest.mark.parametrize("case", sorted(PR.SOLVER_CASES))
def test_solver_cases_are_sized_and_converge(case):
    m = _model(3)
    F, fixed = PR.solver_case(m.coords, case)
    mask = torch.zeros(m.N, 3, dtype=torch.bool)
    mask[fixed] = True
    u, st, info = PR.newton(m, F, mask, PR.LOAD_PATH, tol=1e-10)
    print(f"{case}: iterations {info['iterations']} plastic fraction {info['plastic_fraction']}")
    assert info["converged"] and max(info["iterations"]) <= 8
    assert 0.3 <= info["plastic_fraction"][1] <= 0.9
    assert info["plastic_fraction"][2] == 0.0                       # the partial unloading is elastic
    assert torch.equal(info["states"][2][0], info["states"][1][0]) and torch.equal(info["states"][2][1],
                                                                                   info["states"][1][1])
    free = ~mask.reshape(-1)
    assert float(torch.linalg.eigvalsh(m.dense_tangent(u, st)[free][:, free])[0]) > 0.0
    assert _trace_over_norm(st) <= 1e-15     # after two plastic steps and an elastic one


def test_arguments_are_checked_before_any_device_call():
    from fem355 import element, solver, system
    c, t = _mesh(2)
    F, fixed = PR.solver_case(c, "pull")
    N, M = c.shape[0], t.shape[0]
    ok = dict(coords=c, elements=t, F=F, fixed=fixed, E=1.0, nu=0.3, yield_stress=0.01, hardening=0.1)
    short = system.PlasticState(torch.zeros(M - 1, 6, dtype=F64), torch.zeros(M - 1, dtype=F64))
    for bad in (dict(yield_stress=0.0), dict(yield_stress=-1.0), dict(hardening=-0.1), dict(nu=0.5), dict(nu=-1.0),
                dict(E=0.0), dict(load_path=[]), dict(load_path=[0.5, float("nan")]), dict(load_steps=0),
                dict(F=F[:-1]), dict(fixed=[N]), dict(fixed=torch.zeros(N - 1, 3, dtype=torch.bool)),
                dict(elements=t[:, :3]), dict(u_init=F[:, :2]), dict(max_iter=0), dict(linear_rtol=0.0),
                dict(state=short), dict(state=(1, 2))):
        with pytest.raises(ValueError):
            solver.elastoplastic_static_solver(**{**ok, **bad})
    u = torch.zeros_like(c)
    for bad in (dict(yield_stress=0.0), dict(hardening=-1.0), dict(nu=0.7), dict(state=short)):
        kw = {**dict(E=1.0, nu=0.3, yield_stress=0.01, hardening=0.1), **bad}
        with pytest.raises(ValueError):
            element.compute_c3d4_plastic_update(c, t, u, device="cpu", **kw)
    with pytest.raises(ValueError):
        element.compute_c3d4_plastic_update(c, t[:, :3], u, 1.0, 0.3, 0.01, 0.1, device="cpu")
    assert "compute_c3d4_plastic_update" in element.__all__ and "PlasticState" in element.__all__
    assert element.PlasticState is system.PlasticState
    v = system.PlasticState.virgin(5, "cpu")
    assert v.plastic_strain.shape == (5, 6) and v.equivalent_plastic_strain.shape == (5,)
    assert float(v.plastic_strain.abs().max()) == 0.0
    # the new result fields default to None: nonlinear_static_solver's results are unchanged
    r = system.NonlinearResult(u, True, system.NL_OK)
    assert r.state is None and r.stress is None and r.plastic_fraction is None and r.failed_step is None
    assert "j2" not in system.C.MATERIALS
