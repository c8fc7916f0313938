"""Nonlinear c3d4 statics on the device (csrc/nonlinear.hip, the element.compute_c3d4_* functions, system.NewtonStatics,
solver.nonlinear_static_solver, solver.newton_raphson_solver) against the autograd oracle of tests/hyperelastic_ref.py.

Meshes: mesh.kuhn_cube(3, jitter=0.15) (64 nodes, 162 tets: two full blocks of 64 elements and a partial one),
kuhn_cube(2, jitter=0.15), a single tet, and no element at all; material E = 1, nu = 0.3 on the unit cube and the
bench's 113.8e9, 0.342 on coordinates scaled by modal_ref.SCALE; both materials. Fields: zero, seeded random of amplitude
0.1 / n, a rigid rotation by 0.7 rad plus a translation, the uniform stretch u = (0.2 x, -0.05 y, 0).

Tolerances:
  element outputs  per element, max deviation <= 1e-12 x that element's max reference magnitude (the operator tolerance);
                   where the reference is zero (zero field, rigid rotation): 1e-12 mu V max|g| for the forces, 1e-12 mu V
                   for the energy, 1e-12 mu for the stress. Packed == full upper blocks, full == its transpose, the
                   Kt == NULL launch == the tangent launch in fe / we, two runs: all bitwise. NaN tails past M and N in
                   every array stay NaN and no NaN comes out.
  u = 0            tangent vs compute_c3d4_K_matrix rel <= 1e-12; svk forces exactly 0, neo-Hooke <= 8 2^-53 mu V max|g|.
  gather           fint vs the oracle's global gradient rel <= 1e-12; |sum over nodes| <= 64 2^-53 sum |fe|; masked dofs of
                   r exactly 0; two runs bitwise.
  assembled        A.matvec(d) vs the dense Hessian times d rel <= 1e-12 (layout A and FEM355_SL=0); a refilled matrix
                   == a fresh one bitwise.
  solver           kuhn_cube(3), z = 0 fixed, top-face loads pull / shear / push, load_steps 2, tol 1e-10: converged;
                   Newton iterations per step <= the direct restatement's + 2 (inexact inner solves); every step length
                   1; max|u_dev - u_direct| <= 8 x the PCG restatement's own deviation from the direct one (8: the
                   margin the transient and modal tests use for a ratio of two like errors); nonlinear vs linear answer
                   differ by more than 1e-2; at 1e-6 of the load they agree to rel 1e-5.
  newton_raphson   golden run of the reference's own function: same message forms, outer iterations within +-1,
                   max|u - u_gold| <= 2 tol / lambda_min.

Measured on the MI355X (test_solver_cases prints them: Newton iterations per step device / direct, PCG iterations per
Newton iteration, deviation of the device / of the PCG restatement from the direct restatement and their ratio (bound 8),
nonlinearity max|u_nl - u_lin| / max|u_lin|). Newton converges quadratically, so all three solvers overshoot the stop
(1e-10 ||F||) in their last step and land within a few roundings of u (|u| ~ 0.1-0.25) of each other: the ratio compares
two deviations of 1e-17 .. 3e-14.
    pull  svk          [4, 4] / [4, 4]   51-56 PCG iterations   2.30e-14  2.30e-14  1.00   0.227
    pull  neo_hookean  [4, 4] / [4, 4]   53-56                  6.94e-17  1.11e-16  0.62   0.107
    push  svk          [4, 5] / [4, 5]   56-62                  8.33e-16  8.33e-16  1.00   0.303
    push  neo_hookean  [4, 4] / [4, 4]   54-58                  1.46e-16  4.51e-17  3.23   0.062
    shear svk          [4, 4] / [4, 4]   55-57                  2.79e-14  2.79e-14  1.00   0.121
    shear neo_hookean  [4, 4] / [4, 4]   54-57                  5.47e-15  5.50e-15  0.99   0.063
Element outputs against the oracle, worst case over the 48 (mesh, scale, material, field) cases, in units of the bound's
scale: Kt 4.7e-15, det F 1.6e-15, fe 9.7e-15, we 1.9e-14, sigma 6.9e-15 (bound 1e-12).
Started from the inverted field: svk recovers (7 Newton iterations), neo_hookean ends LINE_SEARCH_FAILED at once (no
step length down to 2^-10 leaves the inverted set); neither produces a NaN.
newton_raphson_solver: 17 outer iterations against the reference's 17; max|u - u_gold| 2.68e-13 (bound 1.11e-07)."""
import contextlib
import functools
import io
import re

import pytest
import torch

import hyperelastic_ref as HR
import modal_ref as MR
from conftest import load_golden, rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -53
NAN = float("nan")
MESHES = ("kuhn3", "kuhn2", "tet1")
SCALES = ("unit", "bench")
FIELDS = ("zero", "random", "rigid", "stretch")
PAD = 3


@functools.lru_cache(maxsize=None)
def mesh_of(name, scale):
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
        return c * MR.SCALE, t, n, MR.E, MR.NU
    return c, t, n, 1.0, 0.3


@functools.lru_cache(maxsize=None)
def oracle(name, scale, material, fld):
    """The oracle's outputs for one case, formed once and shared (never modified)."""
    c, t, n, E, nu = mesh_of(name, scale)
    m = HR.Model(c, t, E, nu, material)
    u = HR.field(fld, c, n)
    fe, Kt = m.element_forces_tangents(u)
    return dict(model=m, u=u, fe=fe, Kt=Kt, we=m.energies(u).detach(), sigma=m.cauchy(u), detF=m.deformation(u)[1],
                fint=m.f_int(u))


def nan_padded(x, dev):
    return torch.cat([x.to(F64), torch.full((PAD,) + tuple(x.shape[1:]), NAN, dtype=F64)]).to(dev)


def launch(dev, c, t, u, E, nu, material, packed, tangent=True):
    """One raw fem_tet4_nl launch on arrays with NaN tails past N and M -> the outputs' first M rows (+ idx words)."""
    from fem355 import _capi as C
    lib = C.lib()
    N, M = c.shape[0], t.shape[0]
    cd, ud = nan_padded(c, dev), nan_padded(u, dev)
    td = torch.cat([t, torch.zeros((PAD, 4), dtype=torch.long)]).to(dev)
    S = int(lib.fem_ke_sym_stride(4))
    full = lambda *s: torch.full(s, NAN, dtype=F64, device=dev)
    out = dict(Kt=full(M + PAD, S) if packed else full(M + PAD, 12, 12), fe=full(M + PAD, 4, 3), we=full(M + PAD),
               sigma=full(M + PAD, 6), detF=full(M + PAD))
    idx = torch.full((2,), M, dtype=torch.int64, device=dev)
    C.check(lib.fem_tet4_nl(C.ptr(cd), C.ptr(td), M, C.ptr(ud), float(E), float(nu), C.MATERIALS[material],
                            1 if packed else 0, C.ptr(out["Kt"]) if tangent else None, C.ptr(out["fe"]),
                            C.ptr(out["we"]), C.ptr(out["sigma"]), C.ptr(out["detF"]), C.ptr(idx[0:1]),
                            C.ptr(idx[1:2]), C.stream(torch.device(dev))), "fem_tet4_nl")
    torch.cuda.synchronize()
    res = {}
    for k, v in out.items():
        v = v.cpu()
        assert bool(torch.isnan(v[M:]).all()), f"{k}: the tail past M was written"
        if k != "Kt" or tangent:
            assert not bool(torch.isnan(v[:M]).any()), f"{k}: NaN in the output"
        res[k] = v[:M]
    assert bool(torch.isnan(cd[N:]).all()) and bool(torch.isnan(ud[N:]).all())
    res["bad"], res["inverted"] = (int(x) for x in idx.cpu())
    return res


def per_element_dev(a, b):
    """max |a - b| per element -> [M]."""
    M = a.shape[0]
    return (a - b).abs().reshape(M, -1).amax(1)


def per_element_mag(b):
    return b.abs().reshape(b.shape[0], -1).amax(1)


def unpack(Kp):
    """Packed upper blocks [M, 90] -> {(a, b): [M,3,3]}."""
    out, k = {}, 0
    for a in range(4):
        for b in range(a, 4):
            out[(a, b)] = Kp[:, 9 * k: 9 * k + 9].reshape(-1, 3, 3)
            k += 1
    return out


# ---------------------------------------------------------------- element kernel
@pytest.mark.parametrize("fld", FIELDS)
@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", MESHES)
def test_element_outputs(gpu, name, scale, material, fld):
    c, t, n, E, nu = mesh_of(name, scale)
    o = oracle(name, scale, material, fld)
    m, u = o["model"], o["u"]
    full = launch(gpu, c, t, u, E, nu, material, packed=False)
    pk = launch(gpu, c, t, u, E, nu, material, packed=True)
    nt = launch(gpu, c, t, u, E, nu, material, packed=False, tangent=False)
    again = launch(gpu, c, t, u, E, nu, material, packed=False)
    M = t.shape[0]
    assert full["bad"] == M and full["inverted"] == M
    # bitwise properties
    for (a, b), blk in unpack(pk["Kt"]).items():
        assert torch.equal(blk, full["Kt"][:, 3 * a: 3 * a + 3, 3 * b: 3 * b + 3]), (a, b)
    assert torch.equal(full["Kt"], full["Kt"].transpose(1, 2))
    for k in ("fe", "we", "sigma", "detF"):
        assert torch.equal(nt[k], full[k]) and torch.equal(pk[k], full[k]), k
    for k in ("Kt", "fe", "we", "sigma", "detF"):
        assert torch.equal(again[k], full[k]), k
    # against the oracle, per element
    gmax = m.g.abs().reshape(M, -1).amax(1)
    zero_ref = fld in ("zero", "rigid")
    scales = {"Kt": per_element_mag(o["Kt"]), "detF": per_element_mag(o["detF"]),
              "fe": m.mu * m.V * gmax if zero_ref else per_element_mag(o["fe"]),
              "we": m.mu * m.V if zero_ref else per_element_mag(o["we"]),
              "sigma": torch.full((M,), m.mu, dtype=F64) if zero_ref else per_element_mag(o["sigma"])}
    worst = {k: float((per_element_dev(full[k], o[k]) / scales[k]).max()) for k in scales}
    print(f"{name} {scale} {material} {fld}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-12, (k, v)
    if fld == "zero":
        if material == "svk":
            assert float(full["fe"].abs().max()) == 0.0
        else:
            assert bool((full["fe"].abs().reshape(M, -1).amax(1) <= 8 * EPS * m.mu * m.V * gmax).all())


@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("scale", SCALES)
def test_zero_displacement_is_the_linear_stiffness(gpu, scale, material):
    from fem355 import element
    c, t, n, E, nu = mesh_of("kuhn3", scale)
    Kt = element.compute_c3d4_tangent_K_matrix(c, t, torch.zeros_like(c), E, nu, material=material, device=gpu,
                                               dtype=F64)
    K0 = element.compute_c3d4_K_matrix(c, t, E, nu, device=gpu, dtype=F64)
    assert rel(Kt, K0) <= 1e-12
    # usable as element matrices: K(0) p through the element-by-element operator
    p = torch.randn(c.shape[0], 3, dtype=F64, generator=torch.Generator().manual_seed(3))
    assert rel(element.compute_nodal_forces(Kt, t, p, device=gpu, dtype=F64),
               element.compute_nodal_forces(K0, t, p, device=gpu, dtype=F64)) <= 1e-12


def test_no_elements(gpu):
    from fem355 import _capi as C, element
    lib = C.lib()
    c = torch.rand(4, 3, dtype=F64)
    t = torch.zeros((0, 4), dtype=torch.long)
    z = torch.zeros_like(c)
    assert element.compute_c3d4_tangent_K_matrix(c, t, z, 1.0, 0.3, device=gpu, dtype=F64).shape == (0, 12, 12)
    assert element.compute_c3d4_strain_energy(c, t, z, 1.0, 0.3, device=gpu, dtype=F64).shape == (0,)
    # M == 0 and N == 0 return FEM_OK without a launch: null pointers are never touched
    assert lib.fem_tet4_nl(None, None, 0, None, 1.0, 0.3, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert lib.fem_tet4_nl_gather(None, None, None, 0, None, 1.0, None, None, None, None) == 0
    assert lib.fem_tet4_nl(None, None, 0, None, 1.0, 0.3, 7, 0, None, None, None, None, None, None, None, None) \
        == C.FEM_EARG


def test_public_functions(gpu):
    """The element.py layer on one case: shapes, dtype conversion, the stress chain, the error messages."""
    from fem355 import element
    o = oracle("kuhn3", "unit", "neo_hookean", "random")
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    u = o["u"]
    kw = dict(material="neo_hookean", device=gpu, dtype=F64)
    assert rel(element.compute_c3d4_internal_forces(c, t, u, E, nu, **kw), o["fint"]) <= 1e-12
    assert rel(element.compute_c3d4_strain_energy(c, t, u, E, nu, **kw), o["we"]) <= 1e-12
    sig = element.compute_c3d4_cauchy_stress(c, t, u, E, nu, **kw)
    assert rel(sig, o["sigma"]) <= 1e-12
    ten = element.compute_stress_tensor(sig)
    assert rel(element.compute_von_mises_stress(ten), R.von_mises(R.stress_tensor(o["sigma"]))) <= 1e-12
    Fm, J = element.compute_c3d4_deformation_gradient(c, t, u, device=gpu, dtype=F64)
    Fr, Jr = o["model"].deformation(u)
    assert rel(Fm, Fr) <= 1e-12 and rel(J, Jr) <= 1e-12
    assert element.compute_c3d4_tangent_K_matrix(c, t, u, E, nu, material="svk", device=gpu).dtype == torch.float32
    Kp = element._tet4_tangent_sym(c, t, u, E, nu, material="svk", device=gpu)
    assert Kp.shape == (t.shape[0], 90) and Kp.is_cuda
    with pytest.raises(ValueError, match="Unknown material"):
        element.compute_c3d4_tangent_K_matrix(c, t, u, E, nu, material="rubber", device=gpu)
    flat = c.clone()
    flat[t[5]] = flat[t[5, 0]].clone()
    with pytest.raises(ValueError, match="Singular matrix"):
        element.compute_c3d4_strain_energy(flat, t, u, E, nu, device=gpu)
    for name in ("compute_c3d4_tangent_K_matrix", "compute_c3d4_internal_forces", "compute_c3d4_strain_energy",
                 "compute_c3d4_cauchy_stress", "compute_c3d4_deformation_gradient"):
        assert name in element.__all__


# ---------------------------------------------------------------- gather
@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("name", ("kuhn3", "kuhn2"))
def test_gather(gpu, name, material):
    from fem355 import _capi as C, system
    lib = C.lib()
    c, t, n, E, nu = mesh_of(name, "unit")
    o = oracle(name, "unit", material, "random")
    N, M = c.shape[0], t.shape[0]
    fe = launch(gpu, c, t, o["u"], E, nu, material, packed=False, tangent=False)["fe"]
    inc_ptr, inc = system.incidence(t.to(gpu), N)
    fed = torch.cat([fe, torch.full((PAD, 4, 3), NAN, dtype=F64)]).to(gpu)
    fext = torch.randn(N, 3, dtype=F64, generator=torch.Generator().manual_seed(5))
    fextd = nan_padded(fext, gpu)
    mask = torch.zeros(3 * N + PAD, dtype=torch.uint8)
    mask[: 3 * N: 7] = 1
    maskd = mask.to(gpu)

    def run():
        fint = torch.full((N + PAD, 3), NAN, dtype=F64, device=gpu)
        r = torch.full((N + PAD, 3), NAN, dtype=F64, device=gpu)
        C.check(lib.fem_tet4_nl_gather(C.ptr(fed), C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(fextd), 0.75, C.ptr(maskd),
                                       C.ptr(fint), C.ptr(r), C.stream(torch.device(gpu))), "fem_tet4_nl_gather")
        torch.cuda.synchronize()
        fint, r = fint.cpu(), r.cpu()
        assert bool(torch.isnan(fint[N:]).all()) and bool(torch.isnan(r[N:]).all())
        return fint[:N], r[:N]

    fint, r = run()
    fint2, r2 = run()
    assert torch.equal(fint, fint2) and torch.equal(r, r2)
    assert rel(fint, o["fint"]) <= 1e-12
    assert float(fint.sum(0).abs().max()) <= 64 * EPS * float(fe.abs().sum())
    mk = mask[: 3 * N].view(N, 3) != 0
    assert float(r[mk].abs().max()) == 0.0
    want = 0.75 * fext - fint
    assert bool(((r - want)[~mk].abs() <= 2 * EPS * (0.75 * fext.abs() + fint.abs())[~mk]).all())


# ---------------------------------------------------------------- assembled tangent
@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("layout", ("layoutA", "plain"))
def test_assembled_tangent_and_refill(gpu, layout, material, monkeypatch):
    from fem355 import system
    if layout == "plain":
        monkeypatch.setenv("FEM355_SL", "0")
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    o1, o2 = oracle("kuhn3", "unit", material, "random"), oracle("kuhn3", "unit", material, "stretch")
    N = c.shape[0]
    mask = torch.zeros(3 * N, dtype=torch.uint8, device=gpu)

    def make():
        return system.NewtonStatics(c.to(gpu), t.to(gpu), E, nu, material, mask)

    d = torch.randn(3 * N, dtype=F64, generator=torch.Generator().manual_seed(11))
    ns = make()
    A = ns.tangent(o1["u"].to(gpu))
    assert A.solver_layout == (layout == "layoutA")
    y1 = A.matvec(d.to(gpu)).cpu()
    assert rel(y1, o1["model"].dense_tangent(o1["u"]) @ d) <= 1e-12
    y2 = ns.tangent(o2["u"].to(gpu)).matvec(d.to(gpu)).cpu()      # refilled in place
    fresh = make()
    y2f = fresh.tangent(o2["u"].to(gpu)).matvec(d.to(gpu)).cpu()
    assert torch.equal(y2, y2f)
    assert torch.equal(ns.jacobi().cpu(), fresh.jacobi().cpu())
    assert rel(y2, o2["model"].dense_tangent(o2["u"]) @ d) <= 1e-12
    # evaluate: the residual, the energy (two runs bit-equal) and the tangent kept for tangent()
    fext = torch.randn(3 * N, dtype=F64, generator=torch.Generator().manual_seed(13)).to(gpu)
    r, en, rn, inv = ns.evaluate(o1["u"].to(gpu), 0.5, fext, tangent=True)
    r = r.clone()
    r_b, en_b, rn_b, _ = fresh.evaluate(o1["u"].to(gpu), 0.5, fext, tangent=False)
    assert inv is None and en == en_b and rn == rn_b and torch.equal(r, r_b)
    assert abs(en - float(o1["we"].sum())) <= 1e-12 * float(o1["we"].abs().sum())
    assert rel(r.cpu().view(N, 3), 0.5 * fext.cpu().view(N, 3) - o1["fint"]) <= 1e-12
    assert torch.equal(ns.tangent().matvec(d.to(gpu)).cpu(), y1)
    ns.close()
    fresh.close()


# ---------------------------------------------------------------- inverted elements
@functools.lru_cache(maxsize=None)
def inverted_case():
    """A field that pushes one node of a tet of the second block through its opposite face: u_a = -1.5 g_a / |g_a|^2
    takes N_a from 1 to -0.5 (det F = 1 + u_a . g_a = -0.5 there). The tet is chosen so that it is the lowest inverted
    one (the node's other tets may invert too)."""
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    g = R.tet4_gradients(c, t)
    for e in range(64, t.shape[0]):
        for a in range(4):
            u = torch.zeros_like(c)
            u[t[e, a]] = -1.5 * g[e, a] / (g[e, a] @ g[e, a])
            detF = HR.Model(c, t, E, nu, "svk").deformation(u)[1]
            if int(torch.nonzero(detF <= 0)[0]) == e:
                return e, u, detF
    raise AssertionError("no such element")


@pytest.mark.parametrize("material", HR.MATERIALS)
def test_inverted_element(gpu, material):
    from fem355 import element, solver, system
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    e_inv, u, detF = inverted_case()
    M = t.shape[0]
    bad = detF <= 0
    m = HR.Model(c, t, E, nu, material)
    full = launch(gpu, c, t, u, E, nu, material, packed=False)     # asserts: no NaN anywhere
    assert full["inverted"] == e_inv and full["bad"] == M
    assert float(full["Kt"][bad].abs().max()) == 0.0 and float(full["fe"][bad].abs().max()) == 0.0
    assert float(full["sigma"][bad].abs().max()) == 0.0
    assert bool((full["we"][bad] == float("inf")).all())
    assert rel(full["detF"], detF) <= 1e-12 and bool((full["detF"][bad] <= 0).all())
    # the good elements still match the oracle (svk is defined for any F; neo-Hooke only where det F > 0)
    good = ~bad
    fe, Kt = HR.Model(c, t[good], E, nu, material).element_forces_tangents(u)
    assert float((per_element_dev(full["Kt"][good], Kt) / per_element_mag(Kt)).max()) <= 1e-12
    assert float((per_element_dev(full["fe"][good], fe) / (m.mu * m.V[good] * m.g[good].abs().reshape(-1, 12).amax(1))
                  ).max()) <= 1e-12
    for fn in (element.compute_c3d4_tangent_K_matrix, element.compute_c3d4_internal_forces,
               element.compute_c3d4_strain_energy, element.compute_c3d4_cauchy_stress):
        with pytest.raises(ValueError, match=rf"Inverted element \(det F <= 0\) at element {e_inv}\."):
            fn(c, t, u, E, nu, material=material, device=gpu, dtype=F64)
    F, fixed = HR.solver_case(c, "pull")
    with contextlib.redirect_stdout(io.StringIO()):
        un, info = solver.nonlinear_static_solver(c, t, F, fixed, E, nu, material=material, tol=1e-10, u_init=u,
                                                  device=gpu, return_info=True)
    assert not bool(torch.isnan(un).any())
    assert info.converged or info.status == system.NL_LINE_SEARCH_FAILED
    print(f"inverted start, {material}: status {info.status}, iterations {info.newton_iterations}")


# ---------------------------------------------------------------- solver
@functools.lru_cache(maxsize=None)
def restatements(case, material):
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    m = HR.Model(c, t, E, nu, material)
    F, fixed = HR.solver_case(c, case)
    ud, idir = HR.newton(m, F, fixed, load_steps=2, tol=1e-10)
    up, ipcg = HR.newton(m, F, fixed, load_steps=2, tol=1e-10, linear="pcg", linear_rtol=1e-6)
    assert idir["converged"] and ipcg["converged"]
    return F, fixed, ud, idir, up, ipcg


@pytest.mark.parametrize("material", HR.MATERIALS)
@pytest.mark.parametrize("case", sorted(HR.SOLVER_CASES))
def test_solver_cases(gpu, case, material, capsys):
    from fem355 import solver
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    F, fixed, ud, idir, up, ipcg = restatements(case, material)
    u, info = solver.nonlinear_static_solver(c, t, F, fixed, E, nu, material=material, load_steps=2, tol=1e-10,
                                             device=gpu, return_info=True)
    text = capsys.readouterr().out
    u = u.cpu()
    ulin = solver.solve_tet4(c, t, F, fixed, kind="elastic", E=E, nu=nu, rtol=1e-12, device=gpu)[0].cpu()
    dev_d, pcg_d = float((u - ud).abs().max()), float((up - ud).abs().max())
    nonlin = float((u - ulin).abs().max() / ulin.abs().max())
    with capsys.disabled():
        print(f"\n    {case:5s} {material:11s} newton {info.newton_iterations} / {idir['iterations']}  pcg "
              f"{info.pcg_iterations}  dev {dev_d:.2e}  pcg-restatement {pcg_d:.2e}  ratio {dev_d / max(pcg_d, 1e-300):.2f}  "
              f"nonlinearity {nonlin:.3f}")
    assert info.converged and info.status == "OK"
    assert text.count("Load step") == 2 and "Load step 2/2" in text
    assert text.count("Converged after") == 2 and "Iteration 1, Residual Norm: " in text
    assert len(info.newton_iterations) == 2
    for k_dev, k_dir in zip(info.newton_iterations, idir["iterations"]):
        assert k_dev <= k_dir + 2
    assert all(a == 1.0 for s in info.step_lengths for a in s)
    assert dev_d <= 8 * pcg_d
    assert nonlin > 1e-2


@pytest.mark.parametrize("material", HR.MATERIALS)
def test_small_load_is_linear(gpu, material, capsys):
    from fem355 import solver
    c, t, n, E, nu = mesh_of("kuhn3", "unit")
    F, fixed = HR.solver_case(c, "pull", scale=1e-6)
    u = solver.nonlinear_static_solver(c, t, F, fixed, E, nu, material=material, tol=1e-10, device=gpu).cpu()
    ulin = solver.solve_tet4(c, t, F, fixed, kind="elastic", E=E, nu=nu, rtol=1e-12, device=gpu)[0].cpu()
    capsys.readouterr()
    assert rel(u, ulin) <= 1e-5


# ---------------------------------------------------------------- newton_raphson_solver (the reference's signature)
def secant_K_func(g, dev, linear=False):
    K0, B, Ks, tets = (g[k].to(dev) for k in ("K0", "B", "Kspring", "tets"))
    M = tets.shape[0]

    def K_func(u):
        if linear:
            return K0 + Ks
        eps = torch.einsum("mij,mj->mi", B, u[tets].reshape(M, 12))
        return K0 * (1.0 + 4.0 * (eps * eps).sum(1)).view(M, 1, 1) + Ks
    return K_func


LINE_FORMS = (r"Iteration (\d+), Residual Norm: \S+", r"Converged after (\d+) iterations\.",
              r"CG did not converge within the maximum number of iterations\.")


def parse_lines(text):
    """[(form index, number or None)] of a newton_raphson_solver transcript; every line must be of a known form."""
    out = []
    for line in text.strip().splitlines():
        for i, f in enumerate(LINE_FORMS):
            mt = re.fullmatch(f, line.strip())
            if mt:
                out.append((i, int(mt.group(1)) if mt.groups() else None))
                break
        else:
            raise AssertionError(f"unexpected line {line!r}")
    return out


def test_newton_raphson_matches_the_reference_run(gpu, capsys):
    from fem355 import solver
    g = load_golden("newton_secant_n2")
    tol, lam_min = float(g["tol"]), float(g["lam_min"])
    u = solver.newton_raphson_solver(secant_K_func(g, gpu), g["tets"], g["F"], tol=tol, device=gpu, dtype=F64)
    text = capsys.readouterr().out
    mine, gold = parse_lines(text), parse_lines(str(g["stdout"]))
    outer = lambda p: [n for i, n in p if i == 0]
    assert outer(mine) == list(range(1, len(outer(mine)) + 1))
    assert mine[-1] == (1, len(outer(mine))) and gold[-1] == (1, len(outer(gold)))
    assert abs(len(outer(mine)) - len(outer(gold))) <= 1
    dev_u = float((u.cpu() - g["u"]).abs().max())
    with capsys.disabled():
        print(f"\n    newton_raphson: {len(outer(mine))} / {len(outer(gold))} outer iterations, max|u - u_gold| "
              f"{dev_u:.2e} (bound {2 * tol / lam_min:.2e})")
    assert dev_u <= 2 * tol / lam_min


def test_newton_raphson_with_a_linear_K_func(gpu, capsys):
    from fem355 import solver
    g = load_golden("newton_secant_n2")
    K = (g["K0"] + g["Kspring"]).to(gpu)
    u = solver.newton_raphson_solver(secant_K_func(g, gpu, linear=True), g["tets"], g["F"], tol=1e-12, device=gpu,
                                     dtype=F64)
    ucg = solver.stable_conjugate_gradient_solver(K, g["tets"], g["F"], None, tol=1e-12, device=gpu, dtype=F64)
    capsys.readouterr()
    assert rel(u, ucg) <= 1e-8
