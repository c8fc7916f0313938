"""GPU: distributed loads (csrc/loads.hip, loads.py) against the dense restatement tests/loads_ref.py
(pinned by tests/test_loads_cpu.py), and end-to-end cases with closed-form answers.

Tolerances (fp64, coordinates of order 1): load vectors 1e-13, stresses 1e-12 relative to the largest entry
(conftest.rel); closed-form cases 1e-8 (the solves run at tol 1e-12). A second call returns identical bits.
"""
import functools

import pytest
import torch

from conftest import rel
from oracle import ref_cpu as R

import loads_ref as L

pytestmark = pytest.mark.gpu
F64 = torch.float64
RHO, E, NU, ALPHA, T_REF = 7.8e-3, 210.0, 0.3, 1.2e-2, 20.0
G = torch.tensor([0.3, -0.2, -9.81], dtype=F64)
LOAD_TOL, STRESS_TOL = 1e-13, 1e-12


def _mods():
    import fem355  # noqa: F401
    from fem355 import element, loads, mesh, solver
    return element, loads, mesh, solver


@functools.lru_cache(maxsize=None)
def case(name):
    """(coords, elements, element type) of the shapes under test; references are formed from these on the CPU."""
    _, _, mesh, _ = _mods()
    if name == "tet":
        return mesh.kuhn_cube(3, jitter=0.2) + ("c3d4",)
    if name == "hex":
        return mesh.hex_box(3, jitter=0.1) + ("c3d8",)
    if name == "wedge":
        return mesh.wedge_box(3, jitter=0.1) + ("c3d6",)
    if name == "tet10":
        return mesh.tet10_cube(2) + ("c3d10",)
    if name == "tet7":       # 512 nodes, 2,058 tets: more than one 256-thread block, more than one 64-row group
        return mesh.kuhn_cube(7, jitter=0.2) + ("c3d4",)
    if name == "trailing":   # a node no element uses: its row must be written as zeros
        c, t = mesh.kuhn_cube(2, jitter=0.2)
        return torch.cat([c, torch.tensor([[2.0, 2.0, 2.0]], dtype=F64)]), t, "c3d4"
    if name == "inverted":   # one tet with two nodes swapped: negative det
        c, t = mesh.kuhn_cube(3, jitter=0.2)
        t = t.clone()
        t[5, [0, 1]] = t[5, [1, 0]]
        return c, t, "c3d4"
    raise KeyError(name)


def fields(c, t):
    """A smooth nodal temperature, a per-element one, and a nodal acceleration (spin about a skew axis plus g)."""
    _, loads, _, _ = _mods()
    Tn = 40.0 + 25.0 * c[:, 0] - 12.0 * c[:, 1] * c[:, 2] + 7.0 * c[:, 2] ** 2
    Te = Tn[t].mean(1) + 3.0
    an = loads.centrifugal_acceleration(c, [1.0, -2.0, 3.0], origin=[0.5, 0.4, 0.0]) + G
    return Tn, Te, an


VOLUME_CASES = ("tet", "hex", "wedge", "tet10", "tet7", "trailing", "inverted")


@pytest.mark.parametrize("name", VOLUME_CASES)
def test_body_force_vs_restatement(gpu, name):
    _, loads, _, _ = _mods()
    c, t, et = case(name)
    _, _, an = fields(c, t)
    for accel in (G, an):
        got = loads.compute_body_force(c, t, et, RHO, accel, device=gpu, dtype=F64)
        want = L.body_force(c, t, et, RHO, accel)
        err = rel(got, want)
        print(name, "body", "nodal" if accel.dim() == 2 else "uniform", err)
        assert got.shape == (c.shape[0], 3) and err < LOAD_TOL
        assert torch.equal(got, loads.compute_body_force(c, t, et, RHO, accel, device=gpu, dtype=F64))
    if name == "trailing":
        assert torch.equal(got[-1].cpu(), torch.zeros(3, dtype=F64))
    assert loads.compute_body_force(c, t, et.upper(), RHO, G, device=gpu).dtype == torch.float32


@pytest.mark.parametrize("name", [n for n in VOLUME_CASES if n != "tet10"])
def test_thermal_load_vs_restatement(gpu, name):
    _, loads, _, _ = _mods()
    c, t, et = case(name)
    Tn, Te, _ = fields(c, t)
    for kind, T in (("float", 75.0), ("nodal", Tn), ("element", Te)):
        got = loads.compute_thermal_load(c, t, et, E, NU, ALPHA, T, T_ref=T_REF, device=gpu, dtype=F64)
        want = L.thermal_load(c, t, et, E, NU, ALPHA, T, T_ref=T_REF)
        err = rel(got, want)
        print(name, "thermal", kind, err)
        assert err < LOAD_TOL
        assert torch.equal(got, loads.compute_thermal_load(c, t, et, E, NU, ALPHA, T, T_ref=T_REF, device=gpu,
                                                           dtype=F64))
    if name == "trailing":
        assert torch.equal(got[-1].cpu(), torch.zeros(3, dtype=F64))


def test_inverted_tet_keeps_volume_in_body_and_sign_in_thermal(gpu):
    """Swapping two nodes of a tet leaves both of its loads unchanged: the body term uses |det|, the thermal term
    V grad N_a with V = |det| / 6 and the gradients of the signed det (the true gradients), as K does."""
    _, loads, _, _ = _mods()
    c, t, _ = case("tet")
    ci, ti, _ = case("inverted")
    assert float(torch.det((c[ti[5, 1:]] - c[ti[5, :1]])) * torch.det((c[t[5, 1:]] - c[t[5, :1]]))) < 0
    for fn, args in ((loads.compute_body_force, (RHO, G)), (loads.compute_thermal_load, (E, NU, ALPHA, 75.0, T_REF))):
        a = fn(c, t, "c3d4", *args, device=gpu, dtype=F64)
        b = fn(ci, ti, "c3d4", *args, device=gpu, dtype=F64)
        assert rel(b, a) < LOAD_TOL


def test_volume_loads_one_call_equals_the_parts_and_both_forms_agree(gpu):
    _, loads, _, _ = _mods()
    c, t, et = case("tet7")
    Tn, _, an = fields(c, t)
    body = loads.compute_body_force(c, t, et, RHO, an, device=gpu, dtype=F64)
    th = loads.compute_thermal_load(c, t, et, E, NU, ALPHA, Tn, T_ref=T_REF, device=gpu, dtype=F64)
    both = loads._volume_loads(c, t, et, body=(RHO, an), thermal=(E, NU, ALPHA, Tn, T_REF), device=gpu)
    assert torch.equal(both, body + th)
    two = loads._volume_loads(c, t, et, body=(RHO, an), thermal=(E, NU, ALPHA, Tn, T_REF), device=gpu, form="two-pass")
    assert rel(two, both) < LOAD_TOL
    assert torch.equal(two, loads._volume_loads(c, t, et, body=(RHO, an), thermal=(E, NU, ALPHA, Tn, T_REF),
                                                device=gpu, form="two-pass"))


def _surface_groups(name):
    c, t, et = case(name)
    return c, [g for g in L.boundary(t, et)]


@pytest.mark.parametrize("name", ("tet", "hex", "wedge", "tet7"))
def test_surface_loads_vs_restatement(gpu, name):
    _, loads, _, _ = _mods()
    c, groups = _surface_groups(name)
    for faces, extra in groups:
        Fn = faces.shape[0]
        pf = 1.0 + torch.arange(Fn, dtype=F64) / Fn
        tf = torch.stack([pf, -0.5 * pf, 0.25 + 0 * pf], 1)
        # a face with a repeated node and a reversed one ride along
        faces = torch.cat([faces, faces[:1].clone(), torch.flip(faces[1:2], dims=[1])])
        faces[-2, 1] = faces[-2, 0]
        extra = torch.cat([extra, extra[:2]])
        pf, tf = torch.cat([pf, pf[:2]]), torch.cat([tf, tf[:2]])
        for kw in ({"pressure": 2.5}, {"pressure": pf}, {"traction": [0.5, -1.0, 2.0]}, {"traction": tf}):
            for x in (extra, None):
                got = loads.compute_surface_load(c, faces, extra=x, device=gpu, dtype=F64, **kw)
                want = L.surface_load(c, faces, x, **kw)
                err = rel(got, want)
                print(name, faces.shape[1], list(kw), x is not None, err)
                assert err < LOAD_TOL
                assert torch.equal(got, loads.compute_surface_load(c, faces, extra=x, device=gpu, dtype=F64, **kw))


def test_warped_quad_and_orientation(gpu):
    _, loads, _, _ = _mods()
    c = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [1.1, 1.0, 0.3], [-0.1, 0.9, 0.0], [0.5, 0.5, -1.0]], dtype=F64)
    q, x = torch.tensor([[0, 1, 2, 3]]), torch.tensor([4])
    got = loads.compute_surface_load(c, q, extra=x, pressure=2.0, device=gpu, dtype=F64)
    assert rel(got, L.surface_load(c, q, x, pressure=2.0, order=6)) < LOAD_TOL
    for faces in (q, torch.tensor([[0, 1, 2]])):
        rev = torch.flip(faces, dims=[1])
        a = loads.compute_surface_load(c, faces, extra=x, pressure=2.0, device=gpu, dtype=F64)
        assert rel(loads.compute_surface_load(c, rev, extra=x, pressure=2.0, device=gpu, dtype=F64), a) < LOAD_TOL
        b = loads.compute_surface_load(c, faces, pressure=2.0, device=gpu, dtype=F64)
        assert rel(-loads.compute_surface_load(c, rev, pressure=2.0, device=gpu, dtype=F64), b) < LOAD_TOL
        assert float(a[:, 2].sum()) < 0      # outward is +z (extra below): the pressure pushes along -z
    # zero area: three collinear nodes
    cz = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]], dtype=F64)
    z = loads.compute_surface_load(cz, torch.tensor([[0, 1, 2]]), pressure=1.0, device=gpu, dtype=F64)
    assert torch.equal(z.cpu(), torch.zeros(3, 3, dtype=F64))


def test_empty_inputs_give_zero_outputs(gpu):
    _, loads, _, _ = _mods()
    c, t, _ = case("tet")
    ch, th, _ = case("hex")
    zero = torch.zeros((c.shape[0], 3), dtype=F64)
    assert torch.equal(loads.compute_body_force(c, t[:0], "c3d4", RHO, G, device=gpu, dtype=F64).cpu(), zero)
    f_th = loads.compute_thermal_load(c, t[:0], "c3d4", E, NU, ALPHA, 5.0, device=gpu, dtype=F64)
    assert torch.equal(f_th.cpu(), zero)
    assert torch.equal(loads.compute_body_force(ch, th[:0], "c3d8", RHO, G, device=gpu, dtype=F64).cpu(), zero)
    for nf in (3, 4):
        f = loads.compute_surface_load(c, torch.zeros((0, nf), dtype=torch.long), pressure=1.0, device=gpu, dtype=F64)
        assert torch.equal(f.cpu(), zero)
    s, v = loads.compute_thermal_element_stress(c, t[:0], "c3d4", zero, E, NU, ALPHA, 5.0, device=gpu, dtype=F64)
    assert s.shape == (0, 3, 3) and v.shape == (0,)


@pytest.mark.parametrize("name", ("tet", "hex", "wedge", "tet7", "inverted"))
def test_thermal_stress_vs_restatement(gpu, name):
    _, loads, _, _ = _mods()
    c, t, et = case(name)
    Tn, Te, _ = fields(c, t)
    u = 1e-3 * torch.stack([c[:, 0] * c[:, 1], torch.sin(c[:, 2]) + c[:, 0], c[:, 1] ** 2 - c[:, 2]], 1)
    for kind, T in (("float", 75.0), ("nodal", Tn), ("element", Te)):
        for single in ((True,) if et == "c3d4" else (True, False)):
            kw = {} if et == "c3d4" else {"single": single}
            sig, vm = loads.compute_thermal_element_stress(c, t, et, u, E, NU, ALPHA, T, T_ref=T_REF, device=gpu,
                                                           dtype=F64, **kw)
            rs, rv = L.thermal_stress(c, t, et, u, E, NU, ALPHA, T, T_ref=T_REF, single=single)
            print(name, "stress", kind, single, rel(sig, rs), rel(vm, rv))
            assert sig.shape == rs.shape and vm.shape == rv.shape
            assert rel(sig, rs) < STRESS_TOL and rel(vm, rv) < STRESS_TOL
            s2, v2 = loads.compute_thermal_element_stress(c, t, et, u, E, NU, ALPHA, T, T_ref=T_REF, device=gpu,
                                                          dtype=F64, **kw)
            assert torch.equal(sig, s2) and torch.equal(vm, v2)


def test_argument_errors(gpu):
    el, loads, _, _ = _mods()
    c, t, _ = case("tet")
    c10, t10, _ = case("tet10")
    with pytest.raises(ValueError, match="Unsupported element type"):
        loads.compute_body_force(c, t, "c3d20", RHO, G, device=gpu)
    with pytest.raises(ValueError, match="elements"):
        loads.compute_body_force(c, t, "c3d8", RHO, G, device=gpu)
    with pytest.raises(ValueError, match="accel"):
        loads.compute_body_force(c, t, "c3d4", RHO, torch.zeros(2), device=gpu)
    with pytest.raises(ValueError, match="T must"):
        loads.compute_thermal_load(c, t, "c3d4", E, NU, ALPHA, torch.zeros(5), device=gpu)
    with pytest.raises(ValueError, match="c3d10"):
        loads.compute_thermal_load(c10, t10, "c3d10", E, NU, ALPHA, 5.0, device=gpu)
    with pytest.raises(ValueError, match="c3d10"):
        loads.compute_thermal_element_stress(c10, t10, "c3d10", torch.zeros_like(c10), E, NU, ALPHA, 5.0, device=gpu)
    f, x = L.boundary(t, "c3d4")[0]
    for kw in ({}, {"pressure": 1.0, "traction": [0.0, 0.0, 1.0]}):
        with pytest.raises(ValueError, match="exactly one of pressure and traction"):
            loads.compute_surface_load(c, f, extra=x, device=gpu, **kw)
    with pytest.raises(ValueError, match="pressure"):
        loads.compute_surface_load(c, f, pressure=torch.zeros(3), device=gpu)
    with pytest.raises(ValueError, match="extra"):
        loads.compute_surface_load(c, f, extra=x[:-1], pressure=1.0, device=gpu)
    with pytest.raises(ValueError, match="rho"):
        loads.distributed_loads(c, c3d4=t, gravity=G, device=gpu)
    with pytest.raises(ValueError, match="material"):
        loads.distributed_loads(c, c3d4=t, temperature=5.0, material={"E": E, "nu": NU}, device=gpu)
    # a singular tet (four collinear lattice nodes): the text of compute_c3d4_K_matrix
    ts = t.clone()
    ts[3] = torch.tensor([0, 1, 2, 3])
    with pytest.raises(ValueError) as k_err:
        el.compute_c3d4_K_matrix(c, ts, E, NU, device=gpu)
    with pytest.raises(ValueError) as l_err:
        loads.compute_thermal_load(c, ts, "c3d4", E, NU, ALPHA, 5.0, device=gpu)
    assert str(l_err.value) == str(k_err.value)
    with pytest.raises(ValueError) as s_err:
        loads.compute_thermal_element_stress(c, ts, "c3d4", torch.zeros_like(c), E, NU, ALPHA, 5.0, device=gpu)
    assert str(s_err.value) == str(k_err.value)


# ----------------------------------------------------------------------------- end to end, closed-form answers
E1, NU1, A1, DT1 = 100.0, 0.3, 1e-3, 100.0      # E alpha dT = 10
MAT = {"E": E1, "nu": NU1, "alpha": A1}
EYE = torch.eye(3, dtype=F64)


def _e2e(kind):
    _, _, mesh, _ = _mods()
    return (mesh.kuhn_cube(4, jitter=0.2) + ("c3d4",)) if kind == "tet" else (mesh.hex_box(4) + ("c3d8",))


def _boundary_nodes(c):
    return torch.nonzero(((c < 1e-12) | (c > 1 - 1e-12)).any(1)).reshape(-1)


def _stresses(loads, el, c, t, et, u, gpu, thermal):
    kw = {} if et == "c3d4" else {"single": False}
    if thermal:
        return loads.compute_thermal_element_stress(c, t, et, u, E1, NU1, A1, T_REF + DT1, T_ref=T_REF, device=gpu,
                                                    dtype=F64, **kw)[0].cpu()
    return el.compute_element_stress(c, t, u, E1, NU1, et, device=gpu, dtype=F64, **kw)[0].cpu()


@pytest.mark.parametrize("kind", ("tet", "hex"))
def test_free_expansion_is_stress_free(gpu, kind):
    el, loads, _, solver = _mods()
    c, t, et = _e2e(kind)
    F = loads.distributed_loads(c, material=MAT, temperature=T_REF + DT1, T_ref=T_REF, device=gpu, **{et: t})
    assert F.shape == (c.shape[0], 6) and float(F[:, 3:].abs().max()) == 0.0
    u = solver.static_structure_solver(c, F, torch.tensor([0]), material=MAT, tol=1e-12, max_iter=5000, device=gpu,
                                       **{et: t})[:, :3]
    scale = E1 * A1 * DT1
    s = _stresses(loads, el, c, t, et, u, gpu, thermal=True)
    print(kind, "free expansion: max |sigma| / (E alpha dT) =", float(s.abs().max()) / scale)
    assert float(s.abs().max()) <= 1e-8 * scale
    plain = _stresses(loads, el, c, t, et, u, gpu, thermal=False)
    assert rel(plain, (scale / (1 - 2 * NU1)) * EYE.expand_as(plain)) <= 1e-8


@pytest.mark.parametrize("kind", ("tet", "hex"))
def test_clamped_boundary_gives_hydrostatic_thermal_stress(gpu, kind):
    el, loads, _, solver = _mods()
    c, t, et = _e2e(kind)
    F = loads.distributed_loads(c, material=MAT, temperature=T_REF + DT1, T_ref=T_REF, device=gpu, **{et: t})
    u = solver.static_structure_solver(c, F, _boundary_nodes(c), material=MAT, tol=1e-12, max_iter=5000, device=gpu,
                                       **{et: t})[:, :3]
    assert float(u.abs().max()) <= 1e-12
    s = _stresses(loads, el, c, t, et, u, gpu, thermal=True)
    assert rel(s, (-E1 * A1 * DT1 / (1 - 2 * NU1)) * EYE.expand_as(s)) <= 1e-8


def test_self_weight_column(gpu):
    _, loads, mesh, solver = _mods()
    c, t = mesh.hex_box(6)
    rho, g = 2.0, 0.5
    mat = {"E": E1, "nu": 0.0, "alpha": 0.0}
    F = loads.distributed_loads(c, c3d8=t, material=mat, gravity=[0.0, 0.0, -g], rho=rho, device=gpu)
    u = solver.static_structure_solver(c, F, mesh.face_nodes(c, 2, 0.0), c3d8=t, material=mat, tol=1e-12,
                                       max_iter=5000, device=gpu).cpu()
    z = c[:, 2]
    want = -rho * g * (1.0 * z - z ** 2 / 2) / E1
    print("self-weight: rel err", float((u[:, 2] - want).abs().max() / want.abs().max()))
    assert float((u[:, 2] - want).abs().max()) <= 1e-8 * float(want.abs().max())
    assert float(u[:, :2].abs().max()) <= 1e-8 * float(want.abs().max())


@pytest.mark.parametrize("kind", ("tet", "hex"))
def test_hydrostatic_pressure(gpu, kind):
    el, loads, _, solver = _mods()
    c, t, et = _e2e(kind)
    p = 3.0
    F = loads.distributed_loads(c, pressure=[(f, x, p) for f, x in L.boundary(t, et)], device=gpu)
    u = solver.static_structure_solver(c, F, torch.tensor([0]), material=MAT, tol=1e-12, max_iter=5000, device=gpu,
                                       **{et: t})[:, :3]
    s = _stresses(loads, el, c, t, et, u, gpu, thermal=False)
    print(kind, "hydrostatic: rel err", rel(s, -p * EYE.expand_as(s)))
    assert rel(s, -p * EYE.expand_as(s)) <= 1e-8


def test_conduction_and_thermal_stress_pipeline(gpu):
    _, loads, mesh, solver = _mods()
    c, t = mesh.kuhn_cube(4, jitter=0.2)
    lo, hi = mesh.face_nodes(c, 2, 0.0), mesh.face_nodes(c, 2, 1.0)
    ids = torch.cat([lo, hi])
    vals = torch.cat([torch.full((lo.numel(),), 20.0, dtype=F64), torch.full((hi.numel(),), 120.0, dtype=F64)])
    T, res = loads.heat_conduction_solver(c, t, 2.5, ids, vals, tol=1e-12, device=gpu)
    assert rel(T, 20.0 + 100.0 * c[:, 2]) <= 1e-8
    args = (E1, NU1, A1, T_REF)
    Ts, u, sig, vm, info = solver.thermal_stress_solver(c, t, 2.5, ids, vals, *args, lo, tol=1e-12, device=gpu)
    assert torch.equal(Ts, T) and info["conduction"].iterations == res.iterations
    f = loads.compute_thermal_load(c, t, "c3d4", E1, NU1, A1, T, T_REF, device=gpu, dtype=F64)
    u2, _, _ = solver.solve_tet4(c, t, f, lo, kind="elastic", E=E1, nu=NU1, tol=1e-12, device=gpu)
    assert torch.equal(u, u2)
    s2, v2 = loads.compute_thermal_element_stress(c, t, "c3d4", u2, E1, NU1, A1, T, T_REF, device=gpu, dtype=F64)
    assert torch.equal(sig, s2) and torch.equal(vm, v2)
    assert sig.shape == (t.shape[0], 3, 3) and bool(torch.isfinite(sig).all())
    # a heat input q: the lifted right-hand side is q - K T0 (one matvec), checked through the residual
    q = torch.zeros(c.shape[0], dtype=F64)
    q[c.shape[0] // 2] = 1.0
    Tq, _ = loads.heat_conduction_solver(c, t, 2.5, ids, vals, q=q, tol=1e-12, device=gpu)
    Kp = R.tet4_poisson_K(c, t, 2.5)
    r = R.nodal_forces(Kp, t, Tq.cpu().view(-1, 1)).view(-1) - q
    free = torch.ones(c.shape[0], dtype=torch.bool)
    free[ids] = False
    assert float(r[free].abs().max()) <= 1e-10 and torch.equal(Tq.cpu()[ids], vals)
