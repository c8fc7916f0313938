"""Dense torch fp64 restatement of the distributed loads: body force, thermal load, surface loads and the
thermal stress, on the CPU, from the oracle's own pieces (ref_cpu.tet4_gradients, iso_jacobian, iso_gradients,
elasticity_matrix, element_face_normals; ref_cpu.iso_mass pins the body force in tests/test_loads_cpu.py). Nodal sums
are index_add in ascending element order. Pinned by tests/test_loads_cpu.py; the checker of tests/test_gpu_loads.py."""
import torch

from oracle import ref_cpu as R

F64 = torch.float64
M_VEC = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=F64)
NPE = {"c3d4": 4, "c3d6": 6, "c3d8": 8, "c3d10": 10}


def _el():
    from fem355 import element
    return element


def scatter(vec, conn, N):
    """[N,3] = sum of the element / face vectors [K, npe, 3] per node, ascending (element, local) order."""
    return torch.zeros((N, 3), dtype=F64).index_add(0, conn.reshape(-1), vec.reshape(-1, 3))


def shape_tables(etype, points):
    """(Nv [n, npe], [dN [npe, 3]] * n) at the points, the package's shape values and the oracle's derivatives."""
    el = _el()
    Nv = torch.tensor([el._N[etype](*[float(v) for v in p]) for p in points], dtype=F64)
    return Nv, [R.DN[etype](*[float(v) for v in p]) for p in points]


def stiffness_rule(etype):
    """(points, weights, volume-form?) of the K static_structure_solver assembles (ref_cpu.static_structure)."""
    if etype == "c3d6":
        return torch.tensor([[1 / 3, 1 / 3, 0.0]], dtype=F64), torch.ones(1, dtype=F64), True
    p, w = R.POINTS[etype]()
    return p, w, False


def _dT(T, T_ref, N, M):
    """('uniform' | 'nodal' | 'element', T - T_ref as a tensor)."""
    t = torch.as_tensor(T, dtype=F64)
    if t.numel() == 1 and t.dim() <= 1:
        return "uniform", t.reshape(()) - T_ref
    if tuple(t.shape) == (N,):
        return "nodal", t - T_ref
    assert tuple(t.shape) == (M,), t.shape
    return "element", t - T_ref


# ----------------------------------------------------------------------------- volume loads, per element [M, npe, 3]
def body_element_vectors(coords, elements, etype, rho, accel):
    M, npe = elements.shape
    accel = torch.as_tensor(accel, dtype=F64)
    nodal = accel.dim() == 2
    if etype == "c3d4":
        V = R.tet_volumes(coords, elements)
        if not nodal:
            return (rho * V / 4.0).view(M, 1, 1) * accel.view(1, 1, 3).expand(M, 4, 3)
        ae = accel[elements]                                        # [M,4,3]
        return (rho * V / 20.0).view(M, 1, 1) * (ae + ae.sum(1, keepdim=True))
    pts, wts = _el().mass_integration_points(etype)
    Nv, dNs = shape_tables(etype, pts)
    fe = torch.zeros((M, npe, 3), dtype=F64)
    for q in range(pts.shape[0]):
        detJ = torch.det(R.iso_jacobian(coords, elements, dNs[q])).abs()
        aq = torch.einsum("b,mbk->mk", Nv[q], accel[elements]) if nodal else accel.view(1, 3).expand(M, 3)
        fe += (rho * float(wts[q]) * detJ).view(M, 1, 1) * Nv[q].view(1, npe, 1) * aq.view(M, 1, 3)
    return fe


def _BtDm(grads, D):
    """B_a^T D m per node from gradients [M, npe, 3] -> [M, npe, 3] (dense: the Voigt B of the oracle)."""
    Mn, npe, _ = grads.shape
    B = R._voigt_B(grads)                                           # [M,6,3npe]
    return torch.einsum("mji,j->mi", B, D @ M_VEC).view(Mn, npe, 3)


def thermal_element_vectors(coords, elements, etype, E, nu, alpha, T, T_ref=0.0):
    M, npe = elements.shape
    N = coords.shape[0]
    D = R.elasticity_matrix(E, nu)
    kind, dT = _dT(T, T_ref, N, M)
    if etype == "c3d4":
        g = R.tet4_gradients(coords, elements)                      # true gradients (signed det inside the inverse)
        V = R.tet_volumes(coords, elements)                         # |det| / 6
        dTe = dT[elements].mean(1) if kind == "nodal" else dT.expand(M)
        return (V * alpha * dTe).view(M, 1, 1) * _BtDm(g, D)
    pts, wts, volume = stiffness_rule(etype)
    Nv, dNs = shape_tables(etype, pts)
    fe = torch.zeros((M, npe, 3), dtype=F64)
    for q in range(pts.shape[0]):
        g = R.iso_gradients(coords, elements, dNs[q])
        cq = R.wedge_volumes(coords, elements) if volume else \
            float(wts[q]) * torch.det(R.iso_jacobian(coords, elements, dNs[q]))
        dTq = torch.einsum("b,mb->m", Nv[q], dT[elements]) if kind == "nodal" else dT.expand(M)
        fe += (cq * alpha * dTq).view(M, 1, 1) * _BtDm(g, D)
    return fe


def body_force(coords, elements, etype, rho, accel):
    return scatter(body_element_vectors(coords, elements, etype, rho, accel), elements, coords.shape[0])


def thermal_load(coords, elements, etype, E, nu, alpha, T, T_ref=0.0):
    return scatter(thermal_element_vectors(coords, elements, etype, E, nu, alpha, T, T_ref), elements,
                   coords.shape[0])


# ----------------------------------------------------------------------------- surface loads
QUAD_SIGNS = ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0))


def quad_shape(xi, eta):
    """(N [4], dN/dxi [4], dN/deta [4]) of the bilinear face."""
    N = torch.tensor([0.25 * (1 + a * xi) * (1 + b * eta) for a, b in QUAD_SIGNS], dtype=F64)
    dx = torch.tensor([0.25 * a * (1 + b * eta) for a, b in QUAD_SIGNS], dtype=F64)
    dy = torch.tensor([0.25 * b * (1 + a * xi) for a, b in QUAD_SIGNS], dtype=F64)
    return N, dx, dy


def gauss_line(n):
    """n-point Gauss-Legendre rule on [-1, 1] (numpy)."""
    import numpy as np
    x, w = np.polynomial.legendre.leggauss(n)
    return [float(v) for v in x], [float(v) for v in w]


def face_vectors(coords, faces, extra=None, pressure=None, traction=None, order=2):
    """[F, nf, 3] nodal forces per face. tri3: the oracle's element_face_normals (scale 1/2: the area vector A n,
    flipped towards `extra` by its own orientation rule); quad4: order x order Gauss on x_xi x x_eta, the sign fixed
    once per face at the centre."""
    assert (pressure is None) != (traction is None)
    F, nf = faces.shape
    p = None if pressure is None else torch.as_tensor(pressure, dtype=F64).reshape(-1).expand(F) \
        if torch.as_tensor(pressure).numel() == 1 else torch.as_tensor(pressure, dtype=F64)
    t = None if traction is None else torch.as_tensor(traction, dtype=F64).expand(F, 3)
    x = coords[faces]                                               # [F,nf,3]
    rep = torch.zeros(F, dtype=torch.bool)
    for a in range(nf):
        for b in range(a + 1, nf):
            rep |= faces[:, a] == faces[:, b]
    if nf == 3:
        if extra is None:
            An = R.element_face_normals(coords, faces, [[0, 1, 2]], [(0, 1, 2)], None, scale=0.5)[:, 0]
        else:
            fx = torch.cat([faces, extra.view(-1, 1)], 1)
            An = R.element_face_normals(coords, fx, [[0, 1, 2]], [(0, 1, 2)], [3], scale=0.5)[:, 0]
        if p is not None:
            fv = (-(p / 3.0)).view(F, 1, 1) * An.view(F, 1, 3).expand(F, 3, 3)
        else:
            fv = (torch.norm(An, dim=1) / 3.0).view(F, 1, 1) * t.view(F, 1, 3).expand(F, 3, 3)
    else:
        _, dx0, dy0 = quad_shape(0.0, 0.0)
        nc = torch.cross(torch.einsum("a,fak->fk", dx0, x), torch.einsum("a,fak->fk", dy0, x), dim=1)
        sign = torch.ones(F, dtype=F64)
        if extra is not None:
            d = (nc * (coords[extra] - x.mean(1))).sum(1)
            sign[d > 0] = -1.0
        gx, gw = gauss_line(order)
        fv = torch.zeros((F, 4, 3), dtype=F64)
        for xi, wx in zip(gx, gw):
            for eta, wy in zip(gx, gw):
                Nq, dx, dy = quad_shape(xi, eta)
                nA = sign.view(F, 1) * torch.cross(torch.einsum("a,fak->fk", dx, x), torch.einsum("a,fak->fk", dy, x),
                                                   dim=1)
                if p is not None:
                    fv += (wx * wy) * (-p).view(F, 1, 1) * Nq.view(1, 4, 1) * nA.view(F, 1, 3)
                else:
                    fv += (wx * wy) * torch.norm(nA, dim=1).view(F, 1, 1) * Nq.view(1, 4, 1) * t.view(F, 1, 3)
    fv = fv.clone()
    fv[rep] = 0.0
    return fv


def surface_load(coords, faces, extra=None, pressure=None, traction=None, order=2):
    return scatter(face_vectors(coords, faces, extra, pressure, traction, order), faces, coords.shape[0])


# ----------------------------------------------------------------------------- thermal stress
def _thermal_point_stress(B, ue, D, eth):
    strain = torch.bmm(B, ue.unsqueeze(2)).squeeze(2) - eth.view(-1, 1) * M_VEC.view(1, 6)
    s = R.stress_tensor(torch.matmul(strain, D.t()))
    return s, R.von_mises(s)


def thermal_stress(coords, elements, etype, u, E, nu, alpha, T, T_ref=0.0, single=True):
    """(sigma, von Mises) = D (B u_e - alpha dT m) in the layouts of ref_cpu.tet4_stress / iso_stress (c3d8, c3d6)."""
    M, npe = elements.shape
    D = R.elasticity_matrix(E, nu)
    kind, dT = _dT(T, T_ref, coords.shape[0], M)
    ue = u[elements].reshape(M, -1)
    if etype == "c3d4":
        dTe = dT[elements].mean(1) if kind == "nodal" else dT.expand(M)
        return _thermal_point_stress(R.tet4_B(coords, elements), ue, D, alpha * dTe)
    pts, wts = R.POINTS[etype]()
    Nv, dNs = shape_tables(etype, pts)
    sig, vm = [], []
    for q in range(pts.shape[0]):
        dTq = torch.einsum("b,mb->m", Nv[q], dT[elements]) if kind == "nodal" else dT.expand(M)
        s, v = _thermal_point_stress(R._voigt_B(R.iso_gradients(coords, elements, dNs[q])), ue, D, alpha * dTq)
        sig.append(s)
        vm.append(v)
    S, V = torch.stack(sig, 1), torch.stack(vm, 1)
    if single:
        return torch.einsum("i,mijk->mjk", wts, S), torch.einsum("i,mi->m", wts, V)
    return S, V


# ----------------------------------------------------------------------------- checks' helpers
def assembled_K_times(coords, elements, etype, E, nu, x):
    """K x [N,3] with the oracle's element matrices of the static solver's rule (ref_cpu.tet4_K / iso_K defaults)."""
    Ke = R.tet4_K(coords, elements, E, nu) if etype == "c3d4" else R.iso_K(coords, elements, etype, E, nu)
    return R.nodal_forces(Ke, elements, x.contiguous())


def family_volume(coords, elements, etype):
    """Mesh volume by the family's mass rule (sum_q w_q |detJ_q|; c3d4: |det| / 6)."""
    if etype == "c3d4":
        return float(R.tet_volumes(coords, elements).sum())
    pts, wts = _el().mass_integration_points(etype)
    _, dNs = shape_tables(etype, pts)
    return float(sum(float(wts[q]) * torch.det(R.iso_jacobian(coords, elements, dNs[q])).abs().sum()
                     for q in range(pts.shape[0])))


def boundary(elements, etype):
    """[(faces, extra)] of the closed boundary from the oracle's boundary_faces and the package's face tables."""
    from fem355 import topology as tp
    if etype == "c3d4":
        return [R.boundary_faces(elements, tp.TET_SURFACE, tp.TET_SURFACE_X)]
    if etype == "c3d8":
        return [R.boundary_faces(elements, tp.HEX, tp.HEX_SURFACE_X)]
    return [R.boundary_faces(elements, tp.WEDGE_QUAD, tp.WEDGE_QUAD_X),
            R.boundary_faces(elements, tp.WEDGE_TRI, tp.WEDGE_TRI_X)]


def face_area(coords, faces):
    if faces.shape[1] == 3:
        return float(torch.norm(R.element_face_normals(coords, faces, [[0, 1, 2]], [(0, 1, 2)], None, scale=0.5)[:, 0],
                                dim=1).sum())
    return float(face_vectors(coords, faces, None, traction=[1.0, 0.0, 0.0])[:, :, 0].sum())

