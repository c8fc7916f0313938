"""Reference-compatible shell API (`solver/shell.py` of sml2004/CUDA-powered-mesh-handling-and-Iterative-solvers
@ 2025-04-18), executed by the fem355 HIP kernels (`csrc/shell.hip`).

Flat s3 / s4 shells with 6 dofs per node (u, v, w, thx, thy, thz). Same names, arguments, defaults and return shapes
as the reference. Its formulation is reproduced as it is: membrane stiffness on the local (u, v), a
rotation-only bending block on the local (thx, thy), no stiffness on w and thz, the fp32-rounded Gauss abscissa of
s4, the stress functions applying the local B to global displacement rows. As everywhere in the package the
arithmetic is fp64 on the device and `dtype` selects the dtype of what is returned.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

try:
    from . import _capi as C
    from .element import _dev, _out, _prep, _bad_scalar, cached_incidence
except ImportError:  # pragma: no cover - flat import from the package directory
    import _capi as C  # type: ignore
    from element import _dev, _out, _prep, _bad_scalar, cached_incidence  # type: ignore

F64 = torch.float64
LONG = torch.long

__all__ = [
    "compute_kirchoff_D_matrix", "compute_global_to_local_displacement", "compute_shell_nodal_forces",
    "compute_shell_postprocess_values",
    "compute_s3_normal", "identify_s3_shared_edges", "compute_triangle_surface_faces_with_third_node",
    "compute_s3_local_unitvector", "compute_s3_global_to_local_coordinates", "compute_s3_jacobian",
    "compute_s3_shape_gradient", "compute_s3_B_matrix", "compute_s3_K_matrix", "compute_s3_shell_stress",
    "compute_s4_normal", "identify_s4_shared_edges", "compute_square_surface_faces_with_fourth_node",
    "compute_s4_local_unitvector", "compute_s4_global_to_local_coordinates", "s4_integration_points",
    "compute_s4_jacobian", "compute_s4_shape_gradient", "compute_s4_B_matrix_single", "compute_s4_B_matrix",
    "compute_s4_K_matrix", "compute_s4_shell_stress",
    "shell_extrude",
]


# ============================================================================ material and point tables (host)
def _triple(x):
    return tuple(float(v) for v in x)


def _d_rows(membrane, bending):
    """The six distinct entries of D, each formed as the reference forms it (python floats)."""
    E_m, nu_m, t_m = _triple(membrane)
    E_b, nu_b, t_b = _triple(bending)
    a = E_m * t_m / (1 - nu_m ** 2)
    b = E_b * t_b ** 3 / (12 * (1 - nu_b ** 2))
    return [a, nu_m * a, a * (1 - nu_m) / 2, b, nu_b * b, b * (1 - nu_b) / 2]


def _host_doubles(values):
    return (ctypes.c_double * len(values))(*values)


def compute_kirchoff_D_matrix(membrane, bending, device="cuda:0", dtype=torch.float32):
    """[6, 6] blockdiag(membrane, bending) from [E, nu, t] twice: a = E t / (1 - nu^2) and
    b = E t^3 / (12 (1 - nu^2)). `solver/shell.py:15-39`."""
    m0, m1, m2, b0, b1, b2 = _d_rows(membrane, bending)
    D = torch.zeros((6, 6), dtype=F64)
    D[0, 0] = D[1, 1] = m0
    D[0, 1] = D[1, 0] = m1
    D[2, 2] = m2
    D[3, 3] = D[4, 4] = b0
    D[3, 4] = D[4, 3] = b1
    D[5, 5] = b2
    return D.to(device=device, dtype=dtype)


def s4_integration_points(device="cuda:0"):
    """2x2 Gauss rule as float32 tensors: points (+g,-g), (+g,+g), (-g,+g), (-g,-g), weights 1.
    `solver/shell.py:651-672`."""
    g = 1 / np.sqrt(3)
    pts = torch.tensor([[g, -g], [g, g], [-g, g], [-g, -g]], dtype=torch.float32)
    return pts.to(device), torch.ones(4, dtype=torch.float32).to(device)


def _factors(xi, eta):
    """(1 - xi, 1 + xi, 1 - eta, 1 + eta) in the arithmetic of the arguments: a float32 tensor scalar gives factors
    rounded to float32 (the reference's compute_s4_B_matrix iterates over the float32 point tensor), a python float
    gives double factors (its K takes `.item()` of the points)."""
    return [float(1 - xi), float(1 + xi), float(1 - eta), float(1 + eta)]


def _k_points(points):
    """The 4 x 4 factor table of the K rule: the points' values widened to double first (`.item()`)."""
    out = []
    for f in range(4):
        out += _factors(float(points[f, 0]), float(points[f, 1]))
    return out


def _b_points(points):
    out = []
    for f in range(4):
        out += _factors(points[f, 0], points[f, 1])
    return out


# ============================================================================ kernels
def _raise_degenerate(bad, M, what):
    e = int(bad.item())
    if e < M:
        raise ValueError(f"{what}: degenerate shell element {e} (zero edge 0->1, collinear frame or singular "
                         "2x2 Jacobian)")


def _shell_ke(coords, shell, membrane, bending, points, frame, device, want_K=True, want_unit=False):
    lib = C.lib()
    dev, coords, shell = _prep(coords, shell, device)
    M, npe = shell.shape
    d = 6 * npe
    shape = (M, d, d, 4) if frame == C.SHELL_POINTS else (M, d, d)
    K = torch.empty(shape, dtype=F64, device=dev) if want_K else None
    unit = torch.empty((M, 3, 3), dtype=F64, device=dev) if want_unit else None
    bad = _bad_scalar(dev, M)
    D6 = _host_doubles(_d_rows(membrane, bending))
    pts = _host_doubles(_k_points(points)) if npe == 4 else None
    C.check(lib.fem_shell_ke(C.ptr(coords), C.ptr(shell), M, npe, D6, pts, frame, C.ptr(K), C.ptr(unit), C.ptr(bad),
                             C.stream(dev)), "fem_shell_ke")
    _raise_degenerate(bad, M, "fem_shell_ke")
    return K, unit


def _shell_geom(coords, shell, device, factors=None, unit=False, local=False, J=False, grads=False, B=False):
    lib = C.lib()
    dev, coords, shell = _prep(coords, shell, device)
    M, npe = shell.shape

    def buf(want, *shape):
        return torch.empty((M,) + shape, dtype=F64, device=dev) if want else None

    out = (buf(unit, 3, 3), buf(local, npe, 3), buf(J, 2, 2), buf(grads, npe, 2), buf(B, 6, 6 * npe))
    bad = _bad_scalar(dev, M)
    pt = _host_doubles(factors) if factors is not None else None
    C.check(lib.fem_shell_geom(C.ptr(coords), C.ptr(shell), M, npe, pt, *(C.ptr(t) for t in out), C.ptr(bad),
                               C.stream(dev)), "fem_shell_geom")
    _raise_degenerate(bad, M, "fem_shell_geom")
    return out


def _one(t):
    return next(x for x in t if x is not None)


# ============================================================================ shared by s3 and s4
def compute_global_to_local_displacement(shell, displacement, unit, device="cuda:0"):
    """Element displacements [M, npe, 6] with translations and rotations rotated into the element frames.
    `solver/shell.py:41-56`."""
    shell = shell.to(device)
    g = displacement.to(device)[shell]
    unit = unit.to(device)
    rot = lambda v: torch.matmul(v, unit.transpose(1, 2))   # noqa: E731
    return torch.cat([rot(g[..., :3]), rot(g[..., 3:])], dim=-1)


def compute_shell_nodal_forces(K, shell, displacement, unit, device="cuda:0", dtype=torch.float32):
    """y [N, 6] = sum_e R_e^T K_e R_e u from local-frame K [M, d, d] and unit [M, 3, 3], without assembly
    (deterministic row gather, `fem_shell_apply`). `solver/shell.py:58-102`."""
    lib = C.lib()
    dev = _dev(device)
    shell = shell.to(device=dev, dtype=LONG).contiguous()
    K = K.to(device=dev, dtype=F64).contiguous()
    unit = unit.to(device=dev, dtype=F64).contiguous()
    u = displacement.to(device=dev, dtype=F64).contiguous()
    M, npe = shell.shape
    N = u.shape[0]
    if u.dim() != 2 or u.shape[1] != 6:
        raise ValueError(f"displacement must be [N, 6], got {list(u.shape)}")
    if tuple(K.shape) != (M, 6 * npe, 6 * npe) or tuple(unit.shape) != (M, 3, 3):
        raise ValueError(f"K must be [{M}, {6 * npe}, {6 * npe}] and unit [{M}, 3, 3], got {list(K.shape)} and "
                         f"{list(unit.shape)}")
    inc_ptr, inc = cached_incidence(shell, N)
    y = torch.empty((N, 6), dtype=F64, device=dev)
    C.check(lib.fem_shell_apply(C.ptr(K), C.ptr(unit), C.ptr(shell), npe, C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(u),
                                C.ptr(y), C.stream(dev)), "fem_shell_apply")
    return _out(y, device, dtype)


def compute_shell_postprocess_values(NMQ, t, z=0, device="cuda:0", dtype=torch.float32):
    """In-plane stresses at height z from the resultants [M, 6] = (Nxx, Nyy, Nxy, Mxx, Myy, Mxy): s = N / t +
    6 z M / t^2, then principal values, principal angle, max shear and the plane von Mises value.
    `solver/shell.py:104-162`."""
    R = NMQ.to(device=device, dtype=dtype)
    s = R[:, :3] * (1.0 / t) + R[:, 3:6] * (6.0 * z / (t ** 2))
    sx, sy, txy = s[:, 0], s[:, 1], s[:, 2]
    mean = 0.5 * (sx + sy)
    dev_ = 0.5 * (sx - sy)
    rad = torch.sqrt(dev_ * dev_ + txy * txy)
    s1, s2 = mean + rad, mean - rad
    theta = 0.5 * torch.atan2(2.0 * txy, (sx - sy).clamp(min=1.0e-30))
    return {"sx": sx, "sy": sy, "txy": txy, "s1": s1, "s2": s2, "theta_p": theta, "tau_max": 0.5 * (s1 - s2),
            "vm_stress": torch.sqrt(s1 * s1 - s1 * s2 + s2 * s2 + 1.0e-30)}


def _shared_edges(shell, device):
    """[S, 2, 2] = for every edge used by exactly two elements the two (element, edge) pairs, edges in the order of
    their sorted node pairs, the lower (element, edge) first."""
    shell = shell.to(device)
    M, npe = shell.shape
    nxt = torch.roll(torch.arange(npe, device=shell.device), -1)
    pairs = torch.stack([shell, shell[:, nxt]], dim=2).sort(dim=2).values.reshape(-1, 2)   # row = element * npe + edge
    _, inv, cnt = torch.unique(pairs, dim=0, return_inverse=True, return_counts=True)
    order = torch.sort(inv, stable=True).indices
    first = torch.cumsum(cnt, 0) - cnt
    sel = first[cnt == 2]
    if sel.numel() == 0:
        return torch.empty((0, 2, 2), dtype=LONG, device=shell.device)
    slot = torch.stack([order[sel], order[sel + 1]], dim=1)
    return torch.stack([slot // npe, slot % npe], dim=2)


def _boundary_edges(shell, device):
    """Edges used once, listed edge 0 of every element first, then edge 1, ... -> ([K, 2], the node opposite [K])."""
    shell = shell.to(device)
    npe = shell.shape[1]
    edges = torch.cat([shell[:, [k, (k + 1) % npe]] for k in range(npe)], dim=0)
    other = torch.cat([shell[:, (k + npe - 1) % npe] for k in range(npe)], dim=0)
    _, inv, cnt = torch.unique(edges.sort(dim=1).values, dim=0, return_inverse=True, return_counts=True)
    once = cnt[inv] == 1
    return edges[once], other[once]


def _corner_cross(coords, shell, last, device):
    coords = coords.to(device)
    shell = shell.to(device)
    p0 = coords[shell[:, 0]]
    return torch.cross(coords[shell[:, 1]] - p0, coords[shell[:, last]] - p0, dim=1)


def _shell_stress(coords, shell, membrane, bending, displacement, device, dtype):
    lib = C.lib()
    dev, coords, shell = _prep(coords, shell, device)
    M, npe = shell.shape
    u = displacement.to(device=dev, dtype=F64).contiguous()
    if u.dim() != 2 or u.shape[1] != 6 or u.shape[0] != coords.shape[0]:
        raise ValueError(f"displacement must be [N, 6] with N = {coords.shape[0]} nodes, got {list(u.shape)}")
    nmq = torch.empty((M, 6), dtype=F64, device=dev)
    bad = _bad_scalar(dev, M)
    D6 = _host_doubles(_d_rows(membrane, bending))
    pts = _host_doubles(_b_points(s4_integration_points(device="cpu")[0])) if npe == 4 else None
    C.check(lib.fem_shell_stress(C.ptr(coords), C.ptr(shell), M, npe, D6, pts, C.ptr(u), C.ptr(nmq), C.ptr(bad),
                                 C.stream(dev)), "fem_shell_stress")
    _raise_degenerate(bad, M, "fem_shell_stress")
    return _out(nmq, device, dtype)


# ============================================================================ s3
def compute_s3_normal(coords, shell, device="cuda:0"):
    """Area-weighted normals [M, 3] = (x1 - x0) x (x2 - x0) / 2. `solver/shell.py:184-203`."""
    return _corner_cross(coords, shell, 2, device) * 0.5


def identify_s3_shared_edges(shell, device="cuda:0"):
    """`solver/shell.py:205-259`."""
    return _shared_edges(shell, device)


def compute_triangle_surface_faces_with_third_node(shell, device="cuda:0"):
    """`solver/shell.py:261-295`."""
    return _boundary_edges(shell, device)


def compute_s3_local_unitvector(coords, shell, device="cuda:0"):
    """unit [M, 3, 3] = [a; b; c]. `solver/shell.py:297-321`."""
    return _one(_shell_geom(coords, shell, device, unit=True)).to(device=torch.device(device), dtype=coords.dtype)


def _local_from_unit(coords, shell, unit, device):
    coords = coords.to(device)
    x = coords[shell.to(device)]
    return torch.matmul(x - x[:, :1], unit.to(device).transpose(1, 2))


def compute_s3_global_to_local_coordinates(coords, shell, unit, device="cuda:0", dtype=torch.float32):
    """(x - x0) unit^T -> [M, 3, 3] with the caller's `unit`. `solver/shell.py:323-347`."""
    return _local_from_unit(coords, shell, unit, device)


def compute_s3_jacobian(coords, shell, device="cuda:0", dtype=torch.float32):
    """J [M, 2, 2] = [[dx/dxi, dx/deta], [dy/dxi, dy/deta]] of the local x, y. `solver/shell.py:349-384`."""
    return _out(_one(_shell_geom(coords, shell, device, J=True)), device, dtype)


def compute_s3_shape_gradient(coords, shell, device="cuda:0", dtype=torch.float32):
    """(dN/dx, dN/dy) [M, 3, 2]. `solver/shell.py:386-402`."""
    return _out(_one(_shell_geom(coords, shell, device, grads=True)), device, dtype)


def compute_s3_B_matrix(coords, shell, device="cuda:0", dtype=torch.float32):
    """B [M, 6, 18]. `solver/shell.py:404-438`."""
    return _out(_one(_shell_geom(coords, shell, device, B=True)), device, dtype)


def compute_s3_K_matrix(coords, shell, membrane, bending, device="cuda:0", dtype=torch.float32):
    """K [M, 18, 18] = B^T D B detJ / 2 in the element frames (signed detJ). `solver/shell.py:440-453`."""
    K, _ = _shell_ke(coords, shell, membrane, bending, None, C.SHELL_LOCAL, device)
    return _out(K, device, dtype)


def compute_s3_shell_stress(coords, shell, membrane, bending, displacement, device="cuda:0", dtype=torch.float32):
    """Resultants [M, 6] = D B u_e. `solver/shell.py:455-468`."""
    return _shell_stress(coords, shell, membrane, bending, displacement, device, dtype)


# ============================================================================ s4
def compute_s4_normal(coords, shell, device="cuda:0"):
    """(x1 - x0) x (x3 - x0) -> [M, 3]. `solver/shell.py:483-502`."""
    return _corner_cross(coords, shell, 3, device)


def identify_s4_shared_edges(shell, device="cuda:0"):
    """`solver/shell.py:504-559`."""
    return _shared_edges(shell, device)


def compute_square_surface_faces_with_fourth_node(shell, device="cuda:0"):
    """`solver/shell.py:561-597`."""
    return _boundary_edges(shell, device)


def compute_s4_local_unitvector(coords, shell, device="cuda:0"):
    """unit [M, 3, 3] = [a; b; c] with b from edge 0->3. `solver/shell.py:599-623`."""
    return _one(_shell_geom(coords, shell, device, unit=True)).to(device=torch.device(device), dtype=coords.dtype)


def compute_s4_global_to_local_coordinates(coords, shell, unit, device="cuda:0", dtype=torch.float32):
    """(x - x0) unit^T -> [M, 4, 3] with the caller's `unit`. `solver/shell.py:625-649`."""
    return _local_from_unit(coords.to(dtype=dtype), shell, unit, device)


def compute_s4_jacobian(coords, shell, xi, eta, device="cuda:0", dtype=torch.float32):
    """J [M, 2, 2] at (xi, eta). `solver/shell.py:674-721`."""
    return _out(_one(_shell_geom(coords, shell, device, _factors(xi, eta), J=True)), device, dtype)


def compute_s4_shape_gradient(coords, shell, xi, eta, device="cuda:0", dtype=torch.float32):
    """(dN/dx, dN/dy) [M, 4, 2] at (xi, eta). `solver/shell.py:723-746`."""
    return _out(_one(_shell_geom(coords, shell, device, _factors(xi, eta), grads=True)), device, dtype)


def compute_s4_B_matrix_single(coords, shell, xi, eta, device="cuda:0", dtype=torch.float32):
    """B [M, 6, 24] at (xi, eta). `solver/shell.py:748-800`."""
    return _out(_one(_shell_geom(coords, shell, device, _factors(xi, eta), B=True)), device, dtype)


def compute_s4_B_matrix(coords, shell, integration_points=None, single=True, device="cuda:0", dtype=torch.float32):
    """B at every integration point, [M, 6, 24, 4], or their sum [M, 6, 24] (single=True). The points are taken as
    the float32 tensor scalars they are, so the factors 1 +- xi are rounded to float32 (`solver/shell.py:802-823`;
    the reference only defines its weights for integration_points=None, unit weights are used for given points)."""
    if integration_points is None:
        integration_points, _ = s4_integration_points(device="cpu")
    Bs = [compute_s4_B_matrix_single(coords, shell, xi, eta, device=device, dtype=dtype)
          for xi, eta in integration_points]
    B = torch.stack(Bs, dim=-1)
    return B.sum(dim=-1) if single else B


def compute_s4_K_matrix(coords, shell, membrane, bending, integration_points=None, single=True, device="cuda:0",
                        dtype=torch.float32):
    """K [M, 24, 24] = sum over the 2x2 rule of w detJ B^T D B in the element frames, or the four terms
    [M, 24, 24, 4] (single=False). integration_points: (points [4, 2], weights [4]); the rule of
    s4_integration_points by default, whose abscissa is 1/sqrt(3) rounded to float32. `solver/shell.py:825-861`."""
    if integration_points is None:
        pts, w = s4_integration_points(device="cpu")
    else:
        pts, w = integration_points
    if tuple(pts.shape) != (4, 2) or not bool((torch.as_tensor(w).cpu() == 1).all()):
        raise ValueError("compute_s4_K_matrix: a 4-point rule with unit weights is supported")
    K, _ = _shell_ke(coords, shell, membrane, bending, pts.cpu(), C.SHELL_LOCAL if single else C.SHELL_POINTS, device)
    return _out(K, device, dtype)


def compute_s4_shell_stress(coords, shell, membrane, bending, displacement, device="cuda:0", dtype=torch.float32):
    """Resultants [M, 6] = D (sum of the four points' B) u_e. `solver/shell.py:863-876`."""
    return _shell_stress(coords, shell, membrane, bending, displacement, device, dtype)


def shell_global_K(coords, shell, membrane, bending, device="cuda:0"):
    """(K [M, d, d] in the global frame and the block order of the 6-dof assembly, unit [M, 3, 3]) on the compute
    device, fp64: what `system.SixDofMap` / `SellMatrix.add_shell_matrices` take."""
    pts = s4_integration_points(device="cpu")[0] if shell.shape[1] == 4 else None
    return _shell_ke(coords, shell, membrane, bending, pts, C.SHELL_GLOBAL, device, want_unit=True)


# ============================================================================ extrusion to solids
def shell_extrude(coords, tri, quad, thickness, device="cuda:0", dtype=torch.float32):
    """Mid-surface (triangles + quads) -> a layer of wedges and hexahedra of the given thickness: node normals are
    the normalised mean of the unit normals of the adjacent triangles (a quad counts as its triangles 0-1-2 and
    0-2-3), nodes are offset by -+ thickness / 2 along them (bottom layer first), and element k joins its bottom
    and top copies. Returns (coords [2N, 3], wedges [T, 6], hexahedra [S, 4 + 4]). `solver/shell.py:885-984`."""
    eps = 1e-8
    coords = coords.to(device, dtype=dtype)
    N = coords.shape[0]
    normals = torch.zeros((N, 3), dtype=dtype, device=device)
    count = torch.zeros(N, dtype=dtype, device=device)
    for corners in (tri, quad[:, :3], quad[:, [0, 2, 3]]):
        p = coords[corners]
        n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
        n = n / (n.norm(dim=1, keepdim=True) + eps)
        flat = corners.reshape(-1)
        normals.index_add_(0, flat, n.repeat_interleave(3, dim=0))
        count.index_add_(0, flat, torch.ones_like(flat, dtype=dtype))
    normals = normals / (count.unsqueeze(1) + eps)
    normals = normals / (normals.norm(dim=1, keepdim=True) + eps)
    half = 0.5 * thickness * normals
    return (torch.cat([coords - half, coords + half], dim=0), torch.cat([tri, tri + N], dim=1),
            torch.cat([quad, quad + N], dim=1))


# every public function runs in the scope of the device its `device` argument names (_capi.on_device)
C.scope_module(globals())
