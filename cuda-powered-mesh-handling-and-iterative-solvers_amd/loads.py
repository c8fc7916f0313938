"""Distributed loads: body force, surface pressure / traction and thermal strain turned into the nodal force arrays
the solvers take, the stress recovery that takes the thermal strain off, and the two drivers built on them (steady
heat conduction with prescribed temperatures, conduction -> thermal load -> elastic solve -> thermal stress).

The reference has no such functions (its solvers take a finished force array): parity is unpinned; the formulas are the
consistent ones for the element matrices of `element.py` and run in `csrc/loads.hip`. Conventions follow
`element.py`: arithmetic is fp64 on the device, `dtype` selects the dtype of the returned tensor, `device="cpu"`
computes on the current HIP device and returns on the CPU. Argument errors are ValueErrors naming the argument.
"""
from __future__ import annotations

import torch

try:
    from . import _capi as C
    from . import element as _el
    from . import system as _sys
except ImportError:  # pragma: no cover - flat import from the package directory
    import _capi as C  # type: ignore
    import element as _el  # type: ignore
    import system as _sys  # type: ignore

F64 = torch.float64
LONG = torch.long

__all__ = [
    "compute_body_force", "centrifugal_acceleration", "compute_surface_load", "compute_thermal_load",
    "compute_thermal_element_stress", "distributed_loads", "heat_conduction_solver", "thermal_stress_solver",
]

_NPE = {"c3d4": 4, "c3d6": 6, "c3d8": 8, "c3d10": 10}


def _solver():
    try:
        from . import solver
    except ImportError:  # pragma: no cover - flat import
        import solver  # type: ignore
    return solver


def _family(element_type, elements):
    et = str(element_type).lower()
    if et not in _NPE:
        _el._unsupported(element_type)
    if elements.dim() != 2 or elements.shape[1] != _NPE[et]:
        raise ValueError(f"elements: {et} expects [M, {_NPE[et]}], got {list(elements.shape)}")
    return et


def _field(name, value, dev, width, rows):
    """(device fp64 array, FEM_LOAD_* mode) of an optional load field. `width`: trailing size of one row (0: a scalar
    field); `rows`: ((count, mode), ...) of the per-row forms accepted, tried in order."""
    if value is None:
        return None, C.LOAD_NONE
    t = torch.as_tensor(value).detach().to(device=dev, dtype=F64).contiguous()
    one = (width,) if width else ()
    if tuple(t.shape) == one or (not width and t.numel() == 1 and t.dim() <= 1):
        return t.reshape(max(width, 1)), C.LOAD_UNIFORM
    for count, mode in rows:
        if tuple(t.shape) == (count,) + one:
            return t, mode
    want = " or ".join([str(list(one)) if width else "a float"] + [str([c] + list(one)) for c, _ in rows])
    raise ValueError(f"{name} must be {want}, got {list(t.shape)}")


def _gather(vec, conn, N, dev):
    """[N,3] = element / face vectors [K, npe, 3] summed per node in ascending incidence order."""
    if conn.shape[0] == 0:
        return torch.zeros((N, 3), dtype=F64, device=dev)
    inc_ptr, inc = _el.cached_incidence(conn, N)
    out = torch.empty((N, 3), dtype=F64, device=dev)
    C.check(C.lib().fem_tet4_nl_gather(C.ptr(vec), C.ptr(inc_ptr), C.ptr(inc), N, None, 0.0, None, C.ptr(out), None,
                                       C.stream(dev)), "fem_tet4_nl_gather")
    return out


def _iso_tables(et, points, weights, dev):
    p = points.detach().to("cpu", F64).contiguous()
    dN = _el._dn_table(et, p, dev)
    Nv = _el._dev_const((et, "N", p.numpy().tobytes()),
                        lambda: torch.tensor([_el._N[et](*[float(v) for v in p[q]]) for q in range(p.shape[0])],
                                             dtype=F64), dev)
    wh = weights.detach().to("cpu", F64).contiguous()
    w = _el._dev_const(("w", wh.numpy().tobytes()), lambda: wh, dev)
    return Nv, dN, w


def _stiffness_rule(et):
    """(points, weights, fem_iso_ke mode) of the K that static_structure_solver assembles for the family."""
    if et == "c3d6":   # compute_c3d6_K_matrix single=True: B at (1/3, 1/3, 0) times the wedge volume
        return torch.tensor([[1 / 3, 1 / 3, 0.0]], dtype=F64), torch.ones(1, dtype=F64), C.ISO_VOLUME
    p, w = _el._points_weights(et, None)
    return p, w, C.ISO_SUM


def _volume_loads(coords, elements, element_type, body=None, thermal=None, device="cuda:0", form="node"):
    """fp64 device [N,3] of one family: body = (rho, accel) and / or thermal = (E, nu, alpha, T, T_ref). form (c3d4):
    "node" the node-centred kernel, "two-pass" element vectors [M,4,3] then the incidence gather."""
    lib = C.lib()
    dev, coords, elements = _el._prep(coords, elements, device)
    et = _family(element_type, elements)
    N, M = coords.shape[0], elements.shape[0]
    rho, accel, amode = 0.0, None, C.LOAD_NONE
    E, nu, alpha, T, tmode, T_ref = 1.0, 0.0, 0.0, None, C.LOAD_NONE, 0.0
    if body is not None:
        rho = float(body[0])
        accel, amode = _field("accel", body[1], dev, 3, ((N, C.LOAD_NODAL),))
        if accel is None:
            raise ValueError("accel must be [3] or [N, 3], got None")
    if thermal is not None:
        if et == "c3d10":
            raise ValueError("element_type: thermal loads are not built for c3d10 (its reference stiffness rule is "
                             "negative definite, DESIGN Q2); supported: c3d4, c3d6, c3d8")
        E, nu, alpha, T_ref = (float(v) for v in (thermal[0], thermal[1], thermal[2], thermal[4]))
        T, tmode = _field("T", thermal[3], dev, 0, ((N, C.LOAD_NODAL), (M, C.LOAD_ELEMENT)))
        if T is None:
            raise ValueError("T must be a float, [N] or [M], got None")
    if form not in ("node", "two-pass"):
        raise ValueError(f"form must be 'node' or 'two-pass', got {form!r}")
    if M == 0 or (body is None and thermal is None):
        return torch.zeros((N, 3), dtype=F64, device=dev)
    if et == "c3d4":
        inc_ptr, inc = _el.cached_incidence(elements, N)
        F = torch.empty((N, 3), dtype=F64, device=dev)
        fe = torch.empty((M, 4, 3), dtype=F64, device=dev) if form == "two-pass" else None
        bad = _el._bad_scalar(dev, M)
        C.check(lib.fem_tet4_loads(C.ptr(coords), C.ptr(elements), M, C.ptr(inc_ptr), C.ptr(inc), N, rho, C.ptr(accel),
                                   amode, E, nu, alpha, C.ptr(T), tmode, T_ref, C.ptr(fe), C.ptr(F), C.ptr(bad),
                                   C.stream(dev)), "fem_tet4_loads")
        if thermal is not None:   # the gradients' ValueError of compute_c3d4_K_matrix; the body term only needs |det|
            _el._raise_if_singular(bad, M)
        return F
    npe = _NPE[et]
    out = None
    parts = []
    if body is not None:   # the consistent-mass rule
        p, w = _el.mass_integration_points(et)
        parts.append((p, w, C.ISO_SUM, (rho, accel, amode), (1.0, 0.0, 0.0, None, C.LOAD_NONE, 0.0)))
    if thermal is not None:   # the family's stiffness rule: consistent with the K the static solver assembles
        p, w, mode = _stiffness_rule(et)
        parts.append((p, w, mode, (0.0, None, C.LOAD_NONE), (E, nu, alpha, T, tmode, T_ref)))
    for p, w, mode, (r_, a_, am_), (E_, nu_, al_, T_, tm_, Tr_) in parts:
        Nv, dN, wd = _iso_tables(et, p, w, dev)
        fe = torch.empty((M, npe, 3), dtype=F64, device=dev)
        C.check(lib.fem_iso_loads(C.ptr(coords), C.ptr(elements), M, npe, C.ptr(Nv), C.ptr(dN), C.ptr(wd), dN.shape[0],
                                  mode, r_, C.ptr(a_), am_, E_, nu_, al_, C.ptr(T_), tm_, Tr_, C.ptr(fe),
                                  C.stream(dev)), "fem_iso_loads")
        part = _gather(fe, elements, N, dev)
        out = part if out is None else out + part
    return out


def compute_body_force(coords, elements, element_type, rho, accel, device="cuda:0", dtype=torch.float32):
    """Consistent nodal forces [N,3] of the body force rho * accel on c3d4 / c3d6 / c3d8 / c3d10 elements: the
    consistent mass (compute_M_matrix's rules) times the acceleration field. accel: [3] (uniform, e.g. gravity) or
    [N,3] (nodal, e.g. centrifugal_acceleration). ValueError for another element_type or shape."""
    return _el._out(_volume_loads(coords, elements, element_type, body=(rho, accel), device=device), device, dtype)


def centrifugal_acceleration(coords, omega, origin=(0.0, 0.0, 0.0)):
    """Nodal acceleration [N,3] whose body force is the centrifugal load of a spin `omega` [3] (rad/s) about an axis
    through `origin`: -omega x (omega x (x - origin)), pointing away from the axis. On coords' device and dtype."""
    x = torch.as_tensor(coords)
    om = torch.as_tensor(omega, dtype=x.dtype, device=x.device).reshape(-1)
    o = torch.as_tensor(origin, dtype=x.dtype, device=x.device).reshape(-1)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"coords must be [N, 3], got {list(x.shape)}")
    if om.numel() != 3:
        raise ValueError(f"omega must be [3], got {list(om.shape)}")
    if o.numel() != 3:
        raise ValueError(f"origin must be [3], got {list(o.shape)}")
    r = x - o
    om = om.expand_as(r)
    return -torch.cross(om, torch.cross(om, r, dim=1), dim=1)


def compute_thermal_load(coords, elements, element_type, E, nu, alpha, T, T_ref=0.0, device="cuda:0",
                         dtype=torch.float32):
    """Nodal forces [N,3] of the thermal strain alpha (T - T_ref) I: int B^T D (alpha dT m), on the rule of the K that
    static_structure_solver assembles (c3d4 closed form, c3d8 2x2x2, c3d6 the single-point volume form), so a uniform
    dT gives exactly K times the expansion field. T: a float, [N] (nodal; c3d4 takes the element mean) or [M] (per
    element; [N] wins when N == M). ValueError for c3d10 and other element types."""
    return _el._out(_volume_loads(coords, elements, element_type, thermal=(E, nu, alpha, T, T_ref), device=device),
                    device, dtype)


def compute_surface_load(coords, faces, extra=None, pressure=None, traction=None, device="cuda:0",
                         dtype=torch.float32):
    """Nodal forces [N,3] of a load on tri3 [F,3] or quad4 [F,4] faces: a `pressure` (float or [F]) acting against the
    face normal, or a `traction` vector ([3] or [F,3]) -- exactly one. The normal is the right-hand normal of the node
    order; with `extra` [F] (a node off each face on the inner side, as compute_*_surface_faces_with_* return it) it is
    flipped to point away from that node, i.e. outward. A face with a repeated node or zero area contributes zero."""
    lib = C.lib()
    if (pressure is None) == (traction is None):
        raise ValueError("exactly one of pressure and traction must be given")
    dev, coords, faces = _el._prep(coords, faces, device)
    if faces.dim() != 2 or faces.shape[1] not in (3, 4):
        raise ValueError(f"faces must be [F, 3] or [F, 4], got {list(faces.shape)}")
    N, F = coords.shape[0], faces.shape[0]
    if extra is not None:
        extra = torch.as_tensor(extra).to(device=dev, dtype=LONG).contiguous()
        if tuple(extra.shape) != (F,):
            raise ValueError(f"extra must be [{F}] (one node per face), got {list(extra.shape)}")
        _sys.check_connectivity(extra, N)
    p, pmode = _field("pressure", pressure, dev, 0, ((F, C.LOAD_ELEMENT),))
    t, tmode = _field("traction", traction, dev, 3, ((F, C.LOAD_ELEMENT),))
    if F == 0:
        return _el._out(torch.zeros((N, 3), dtype=F64, device=dev), device, dtype)
    fv = torch.empty((F, faces.shape[1], 3), dtype=F64, device=dev)
    C.check(lib.fem_face_loads(C.ptr(coords), C.ptr(faces), F, faces.shape[1], C.ptr(extra), C.ptr(p), pmode, C.ptr(t),
                               tmode, C.ptr(fv), C.stream(dev)), "fem_face_loads")
    return _el._out(_gather(fv, faces, N, dev), device, dtype)


def compute_thermal_element_stress(coords, elements, element_type, displacement, E, nu, alpha, T, T_ref=0.0,
                                   integral_point=None, single=True, device="cuda:0", dtype=torch.float32):
    """compute_element_stress with the thermal strain taken off: sigma = D (B u_e - alpha dT m) and its von Mises, in
    the layouts of compute_c3d4 / c3d8 / c3d6_element_stress ([M,3,3], [M]; c3d8 / c3d6 with single=False
    [M,n_ip,3,3], [M,n_ip]). dT as compute_thermal_load reads T (c3d4: the element mean of a nodal field; c3d8 / c3d6:
    interpolated to each point). ValueError on a degenerate c3d4 element like compute_c3d4_element_stress."""
    lib = C.lib()
    dev, coords, elements = _el._prep(coords, elements, device)
    et = _family(element_type, elements)
    if et == "c3d10":
        raise ValueError("element_type: thermal stress is not built for c3d10 (DESIGN Q2); supported: c3d4, c3d6, c3d8")
    N, M = coords.shape[0], elements.shape[0]
    u = _el._disp(displacement, dev, N)
    Td, tmode = _field("T", T, dev, 0, ((N, C.LOAD_NODAL), (M, C.LOAD_ELEMENT)))
    if Td is None:
        raise ValueError("T must be a float, [N] or [M], got None")
    if et == "c3d4":
        sig = torch.empty((M, 3, 3), dtype=F64, device=dev)
        vm = torch.empty(M, dtype=F64, device=dev)
        bad = _el._bad_scalar(dev, M)
        C.check(lib.fem_tet4_stress_thermal(C.ptr(coords), C.ptr(elements), M, C.ptr(u), float(E), float(nu),
                                            float(alpha), C.ptr(Td), tmode, float(T_ref), C.ptr(sig), C.ptr(vm),
                                            C.ptr(bad), C.stream(dev)), "fem_tet4_stress_thermal")
        _el._raise_if_singular(bad, M)
        return _el._out(sig, device, dtype), _el._out(vm, device, dtype)
    p, w = _el._points_weights(et, integral_point)
    Nv, dN, wd = _iso_tables(et, p, w, dev)
    n_ip = dN.shape[0]
    shape = (M,) if single else (M, n_ip)
    sig = torch.empty(shape + (3, 3), dtype=F64, device=dev)
    vm = torch.empty(shape, dtype=F64, device=dev)
    C.check(lib.fem_iso_stress_thermal(C.ptr(coords), C.ptr(elements), M, _NPE[et], C.ptr(u), float(E), float(nu),
                                       float(alpha), C.ptr(Td), tmode, float(T_ref), C.ptr(Nv), C.ptr(dN), C.ptr(wd),
                                       n_ip, 0 if single else 1, C.ptr(sig), C.ptr(vm), C.stream(dev)),
            "fem_iso_stress_thermal")
    return _el._out(sig, device, dtype), _el._out(vm, device, dtype)


def distributed_loads(coords, c3d4=None, c3d6=None, c3d8=None, material=None, gravity=None, rho=None, pressure=None,
                      temperature=None, T_ref=0.0, device="cuda:0", dtype=torch.float64):
    """Force array [N,6] (columns 3-5 zero) for static_structure_solver: the sum over the families present of the
    body force rho * gravity (gravity [3] or [N,3]) and the thermal load of `temperature` (a float or [N]; material
    carries E, nu, alpha), plus the surface loads pressure = [(faces, extra, p), ...] (compute_surface_load)."""
    dev = _el._dev(device)
    N = coords.shape[0]
    fams = [(et, el) for et, el in (("c3d4", c3d4), ("c3d8", c3d8), ("c3d6", c3d6)) if el is not None]
    body = thermal = None
    if gravity is not None:
        if rho is None:
            raise ValueError("rho must be given with gravity")
        body = (rho, gravity)
    if temperature is not None:
        if material is None or any(k not in material for k in ("E", "nu", "alpha")):
            raise ValueError("material must carry E, nu and alpha with temperature")
        thermal = (material["E"], material["nu"], material["alpha"], temperature, T_ref)
    if (body is not None or thermal is not None) and not fams:
        raise ValueError("gravity / temperature need at least one of c3d4, c3d6, c3d8")
    F = torch.zeros((N, 6), dtype=F64, device=dev)
    if body is not None or thermal is not None:
        for et, el in fams:
            F[:, :3] += _volume_loads(coords, el, et, body=body, thermal=thermal, device=dev)
    for item in (pressure or ()):
        if len(item) != 3:
            raise ValueError("pressure must be a list of (faces, extra, p)")
        faces, extra, p = item
        F[:, :3] += compute_surface_load(coords, faces, extra=extra, pressure=p, device=dev, dtype=F64)
    return _el._out(F, device, dtype)


def heat_conduction_solver(coords, elements, kappa, T_nodes, T_values, q=None, tol=1e-8, max_iter=10000, rtol=None,
                           device="cuda:0"):
    """Steady c3d4 heat conduction K T = q with prescribed temperatures T[T_nodes] = T_values (a float or one value
    per node), by lifting: T = T0 + theta with T0 the prescribed values, K theta = q - K T0 on the free rows
    (SellMatrix.matvec on assemble_tet4_system's matrix), solved by the Jacobi-PCG of solve_tet4 (absolute `tol` on
    sqrt(r.z); `rtol` scales it by sqrt(r0.z0)). q: nodal heat input [N] or None. Returns (T [N] fp64 on the device,
    PcgResult)."""
    dev, coords, elements = _el._prep(coords, elements, device)
    _family("c3d4", elements)
    N = coords.shape[0]
    ids = torch.as_tensor(T_nodes).to(device=dev, dtype=LONG).reshape(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise ValueError(f"T_nodes must lie in [0, {N})")
    vals = torch.as_tensor(T_values).to(device=dev, dtype=F64)
    if vals.numel() != 1 and tuple(vals.shape) != (ids.numel(),):
        raise ValueError(f"T_values must be a float or [{ids.numel()}], got {list(vals.shape)}")
    T0 = torch.zeros(N, dtype=F64, device=dev)
    T0[ids] = vals
    A = _sys.assemble_tet4_system(coords, elements, "poisson", float(kappa))
    A.check_singular()
    b = -A.matvec(T0)
    if q is not None:
        qd = torch.as_tensor(q).to(device=dev, dtype=F64).reshape(-1)
        if qd.numel() != N:
            raise ValueError(f"q must be [{N}], got {list(torch.as_tensor(q).shape)}")
        b += qd
    b[ids] = 0.0
    mask = torch.zeros(N, dtype=torch.uint8, device=dev)
    mask[ids] = 1
    w = A.jacobi(mask)
    if rtol is not None:
        tol = float(rtol) * float(torch.sqrt(torch.dot(b, w * b)))
    res = A.pcg(b, None, w=w, mode=C.MODE_PCG, tol=tol, max_iter=max_iter)
    return T0 + res.x.view(N), res


def thermal_stress_solver(coords, elements, kappa, T_nodes, T_values, E, nu, alpha, T_ref, fixed, q=None, tol=1e-8,
                          max_iter=10000, rtol=None, device="cuda:0"):
    """c3d4 thermal stress end to end on the device: heat_conduction_solver -> compute_thermal_load of the nodal
    temperatures -> solve_tet4(kind="elastic") with `fixed` nodes held -> compute_thermal_element_stress. tol /
    rtol / max_iter apply to both solves. Returns (T [N], u [N,3], sigma [M,3,3], von Mises [M], info) in fp64 on the
    device; info = {"conduction": PcgResult, "elastic": PcgResult}."""
    dev = _el._dev(device)
    T, hres = heat_conduction_solver(coords, elements, kappa, T_nodes, T_values, q=q, tol=tol, max_iter=max_iter,
                                     rtol=rtol, device=dev)
    f = compute_thermal_load(coords, elements, "c3d4", E, nu, alpha, T, T_ref, device=dev, dtype=F64)
    u, res, _ = _solver().solve_tet4(coords, elements, f, fixed, kind="elastic", E=E, nu=nu, tol=tol,
                                     max_iter=max_iter, device=dev, rtol=rtol)
    sig, vm = compute_thermal_element_stress(coords, elements, "c3d4", u, E, nu, alpha, T, T_ref, device=dev,
                                             dtype=F64)
    return T, u, sig, vm, {"conduction": hres, "elastic": res}


# every public function runs in the scope of the device its `device` argument names (_capi.on_device)
C.scope_module(globals())
