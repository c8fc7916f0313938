"""CPU tier: pins tests/loads_ref.py, the dense restatement of the distributed loads that checks the device kernels
(tests/test_gpu_loads.py), against identities that do not depend on it: total force, the oracle's consistent mass,
closed-surface equilibrium, a high-order quadrature, orientation rules, and the oracle's assembled K."""
import pytest
import torch

import fem355  # noqa: F401
from fem355 import element as el
from fem355 import mesh
from oracle import ref_cpu as R

import loads_ref as L

F64 = torch.float64
RHO, E, NU, ALPHA = 7.8e-3, 210.0, 0.3, 1.2e-2
G = torch.tensor([0.3, -0.2, -9.81], dtype=F64)


def meshes():
    return {"c3d4": mesh.kuhn_cube(3, jitter=0.2), "c3d8": mesh.hex_box(3, jitter=0.1),
            "c3d6": mesh.wedge_box(3, jitter=0.1), "c3d10": mesh.tet10_cube(2)}


MESHES = meshes()
FAMILIES = ("c3d4", "c3d8", "c3d6", "c3d10")


@pytest.mark.parametrize("et", FAMILIES)
def test_body_force_sums_to_weight(et):
    c, t = MESHES[et]
    f = L.body_force(c, t, et, RHO, G)
    want = RHO * L.family_volume(c, t, et) * G
    assert float((f.sum(0) - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("et", FAMILIES)
def test_body_force_is_consistent_mass_times_field(et):
    c, t = MESHES[et]
    N = c.shape[0]
    if et == "c3d4":
        V = R.tet_volumes(c, t)
        Me = torch.kron((RHO * V / 20.0).view(-1, 1, 1) * (torch.ones(4, 4, dtype=F64) + torch.eye(4, dtype=F64)),
                        torch.eye(3, dtype=F64).view(1, 3, 3))
    else:
        p, w = el.mass_integration_points(et)
        Me = R.iso_mass(c, t, el._N[et], R.DN[et], p, w, RHO)
    want = R.nodal_forces(Me, t, G.view(1, 3).expand(N, 3).contiguous())
    got = L.body_force(c, t, et, RHO, G)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # a nodal field equal to the constant gives the same load; a linear one the mass times it
    a = G.view(1, 3) + c @ torch.tensor([[0.5, 0.1, 0.0], [0.0, -0.3, 0.2], [0.4, 0.0, 0.7]], dtype=F64)
    want = R.nodal_forces(Me, t, a.contiguous())
    got = L.body_force(c, t, et, RHO, a)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("et", ("c3d4", "c3d8", "c3d6"))
def test_uniform_pressure_on_closed_boundary_is_self_equilibrated(et):
    c, t = MESHES[et]
    p = 3.5
    f = torch.zeros((c.shape[0], 3), dtype=F64)
    area = 0.0
    groups = L.boundary(t, et)
    assert len(groups) == (2 if et == "c3d6" else 1)      # wedges: quads and triangles
    for faces, extra in groups:
        f += L.surface_load(c, faces, extra, pressure=p)
        area += L.face_area(c, faces)
    assert abs(area - 6.0) < 1e-12
    scale = p * area
    assert float(f.sum(0).abs().max()) <= 1e-12 * scale
    assert float(torch.cross(c, f, dim=1).sum(0).abs().max()) <= 1e-12 * scale
    # outward normals: the pressure pushes inwards, so the virtual work on the expansion field x is -3 p V
    assert abs(float((f * c).sum()) + 3.0 * p * 1.0) <= 1e-12 * scale


def warped_quad():
    c = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [1.1, 1.0, 0.3], [-0.1, 0.9, 0.0], [0.5, 0.5, -1.0]],
                     dtype=F64)
    return c, torch.tensor([[0, 1, 2, 3]]), torch.tensor([4])


def test_warped_quad_matches_high_order_quadrature():
    c, q, x = warped_quad()
    a = L.surface_load(c, q, x, pressure=2.0)
    b = L.surface_load(c, q, x, pressure=2.0, order=6)
    assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


def test_orientation_rules():
    c, q, x = warped_quad()
    tri = torch.tensor([[0, 1, 2]])
    for faces in (q, tri):
        rev = torch.flip(faces, dims=[1])
        with_x = L.surface_load(c, faces, x, pressure=2.0)
        assert float((L.surface_load(c, rev, x, pressure=2.0) - with_x).abs().max()) <= 1e-15
        plain = L.surface_load(c, faces, None, pressure=2.0)
        assert float((L.surface_load(c, rev, None, pressure=2.0) + plain).abs().max()) <= 1e-15
        assert float(with_x[:, 2].sum()) < 0.0      # extra lies below the face: outward is +z, pressure pushes along -z


@pytest.mark.parametrize("et", ("c3d4", "c3d8", "c3d6"))
def test_uniform_dT_load_is_K_times_expansion(et):
    c, t = MESHES[et]
    dT = 35.0
    got = L.thermal_load(c, t, et, E, NU, ALPHA, 20.0 + dT, T_ref=20.0)
    want = L.assembled_K_times(c, t, et, E, NU, ALPHA * dT * c)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the same through the nodal and the per-element forms of a constant field
    for T in (torch.full((c.shape[0],), 20.0 + dT, dtype=F64), torch.full((t.shape[0],), 20.0 + dT, dtype=F64)):
        again = L.thermal_load(c, t, et, E, NU, ALPHA, T, T_ref=20.0)
        assert float((again - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("et", ("c3d4", "c3d8"))
def test_constant_nodal_T_sums_to_zero_on_interior_nodes(et):
    """int grad N_a dV = 0 for an interior node wherever the rule integrates it exactly (c3d4 closed form, c3d8
    2x2x2). The c3d6 single-point volume form does not on a distorted wedge: its load is K x like its K (above)."""
    c, t = MESHES[et]
    f = L.thermal_load(c, t, et, E, NU, ALPHA, torch.full((c.shape[0],), 50.0, dtype=F64))
    interior = ((c > 1e-9) & (c < 1 - 1e-9)).all(1)
    assert int(interior.sum()) == 8
    assert float(f[interior].abs().max()) <= 1e-12 * float(f.abs().max())


def test_thermal_stress_of_free_expansion_vanishes():
    for et in ("c3d4", "c3d8", "c3d6"):
        c, t = MESHES[et]
        dT = 35.0
        s, vm = L.thermal_stress(c, t, et, ALPHA * dT * c, E, NU, ALPHA, dT)
        assert float(s.abs().max()) <= 1e-12 * E * ALPHA * dT and float(vm.abs().max()) <= 1e-12 * E * ALPHA * dT
        plain, _ = (R.tet4_stress(c, t, ALPHA * dT * c, E, NU) if et == "c3d4"
                    else R.iso_stress(c, t, ALPHA * dT * c, et, E, NU, single=False))
        d = torch.diagonal(plain, dim1=-2, dim2=-1)
        assert float((d - E * ALPHA * dT / (1 - 2 * NU)).abs().max()) <= 1e-11 * E * ALPHA * dT
