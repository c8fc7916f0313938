"""CPU tier of the nonlinear c3d4 path: the oracle of tests/hyperelastic_ref.py against itself (the closed-form tangent
blocks of the formulation against the autograd Hessian), its limits (u = 0, rigid rotation), the dense Newton on the
solver cases of tests/test_gpu_nonlinear.py, the argument checks of the public solver and the golden fixture of
newton_raphson_solver. No device call."""
import pytest
import torch

import hyperelastic_ref as HR
from conftest import load_golden, rel
from oracle import ref_cpu as R

F64 = torch.float64
# What the direct restatement was seen to do on the solver cases when they were chosen (n = 2 and 3, both materials,
# the three loads): 4-5 Newton iterations (linear solves) per load step, never a step length below 1, det F above 0.79
# at the solution, peak displacements 0.11-0.25 of the edge, a positive definite tangent. The caps are those figures.
NEWTON_CAP, DETF_FLOOR, PEAK = 5, 0.79, (0.10, 0.26)


def _mesh(n):
    from fem355 import mesh
    return mesh.kuhn_cube(n, jitter=0.15)


@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("name", ("random", "rigid", "stretch"))
def test_closed_form_blocks_match_autograd_hessian(material, name):
    c, t = _mesh(3)
    m = HR.Model(c, t, 1.0, 0.3, material)
    u = HR.field(name, c, 3)
    _, Kt = m.element_forces_tangents(u)
    Kc = HR.closed_form_tangent(m, u)
    scale = Kt.abs().amax((1, 2), keepdim=True)
    assert float(((Kc - Kt).abs() / scale).max()) <= 1e-12
    assert float((Kt - Kt.transpose(1, 2)).abs().max() / Kt.abs().max()) <= 1e-14


@pytest.mark.parametrize("material", HR.MATERIALS)
def test_zero_displacement_is_the_linear_stiffness(material):
    c, t = _mesh(3)
    m = HR.Model(c, t, 113.8e9, 0.342, material)
    fe, Kt = m.element_forces_tangents(torch.zeros_like(c))
    assert rel(Kt, R.tet4_K(c.to(F64), t, 113.8e9, 0.342)) <= 1e-12
    assert float(fe.abs().max()) == 0.0
    assert rel(HR.closed_form_tangent(m, torch.zeros_like(c)), Kt) <= 1e-12


@pytest.mark.parametrize("material", HR.MATERIALS)
def test_rigid_rotation_has_no_force_and_no_energy(material):
    c, t = _mesh(3)
    m = HR.Model(c, t, 1.0, 0.3, material)
    u = HR.field("rigid", c, 3)
    gmax = float(m.g.abs().max())
    inc = int(torch.bincount(t.reshape(-1)).max())   # a node sums the forces of its incident elements
    assert float(m.f_int(u).abs().max()) <= 1e-12 * m.mu * float(m.V.max()) * gmax * inc
    assert float(m.energies(u).abs().max()) <= 1e-12 * m.mu * float(m.V.max())
    assert float(m.cauchy(u).abs().max()) <= 1e-12 * m.mu


@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("case", sorted(HR.SOLVER_CASES))
@pytest.mark.parametrize("n", (2, 3))
def test_direct_newton_converges_on_the_solver_cases(n, case, material):
    c, t = _mesh(n)
    m = HR.Model(c, t, 1.0, 0.3, material)
    F, fixed = HR.solver_case(c, case)
    u, info = HR.newton(m, F, fixed, load_steps=2, tol=1e-10)
    print(f"n={n} {case} {material}: iterations {info['iterations']} alphas {set(info['alphas'])} "
          f"min detF {info['min_detF']:.3f} peak {info['peak']:.3f}")
    assert info["converged"]
    assert max(info["iterations"]) <= NEWTON_CAP
    assert min(info["alphas"]) == 1.0
    assert info["min_detF"] > DETF_FLOOR
    assert PEAK[0] < info["peak"] < PEAK[1]
    free = torch.ones(3 * m.N, dtype=torch.bool)
    free.view(m.N, 3)[fixed] = False
    K = m.dense_tangent(u)
    assert float(torch.linalg.eigvalsh(K[free][:, free])[0]) > 0.0   # the tangent stays positive definite


def test_solver_arguments_are_checked_before_any_device_call():
    from fem355 import solver
    c, t = _mesh(2)
    F, fixed = HR.solver_case(c, "pull")
    ok = dict(coords=c, elements=t, F=F, fixed=fixed, E=1.0, nu=0.3)
    for bad in (dict(material="rubber"), dict(load_steps=0), dict(F=F[:-1]), dict(fixed=[c.shape[0]]),
                dict(elements=t[:, :3]), dict(u_init=F[:, :2]), dict(max_iter=0), dict(linear_rtol=0.0)):
        with pytest.raises(ValueError):
            solver.nonlinear_static_solver(**{**ok, **bad})


def test_newton_secant_golden_loads():
    g = load_golden("newton_secant_n2")
    N, M = g["coords"].shape[0], g["tets"].shape[0]
    assert g["K0"].shape == (M, 12, 12) and g["B"].shape == (M, 6, 12) and g["Kspring"].shape == (M, 12, 12)
    assert g["u"].shape == (N, 3) and g["F"].shape == (N, 3)
    text = str(g["stdout"])
    assert "Converged after" in text and text.count("Iteration") >= 2
    assert float(g["lam_min"]) > 0.0 and float(g["tol"]) == 1e-9
    # the stored u solves K(u) u = F to the stored tolerance
    eps = torch.einsum("mij,mj->mi", g["B"], g["u"][g["tets"]].reshape(M, 12))
    K = g["K0"] * (1.0 + 4.0 * (eps * eps).sum(1)).view(M, 1, 1) + g["Kspring"]
    assert float((g["F"] - R.nodal_forces(K, g["tets"], g["u"])).norm()) < 1e-9
