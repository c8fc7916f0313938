"""Reference-compatible solver API (`solver/solver.py` of sml2004/CUDA-powered-mesh-handling-and-Iterative-
solvers @ 2025-04-18), executed on the MI355X.

Like the reference, this module re-exports the element and shell APIs (`from element import *`, `from shell import *`,
`solver/solver.py:1-2`), so `solver.compute_nodal_forces(...)`, `solver.compute_s3_K_matrix(...)` etc. resolve exactly
as in the notebooks.

The solvers take the reference's hand-off object (element matrices K [M, d, d] + connectivity), assemble them
once on the device into a SELL-64 global matrix (deterministic row-gather, `system.py`) and run the whole
(P)CG iteration on the device (`csrc/pcg.hip`). They print the reference's messages and never raise on
breakdown or non-convergence (`solver/solver.py:187-227,805-811`).
"""
from __future__ import annotations

import torch

try:
    from . import _capi as C
    from . import system as _sys
    from .element import *  # noqa: F401,F403  (the reference's `from element import *`)
    from .element import _dev, _key, cached_incidence, compute_c3d4_K_matrix, compute_c3d6_K_matrix, \
        compute_c3d8_K_matrix
    from .shell import *  # noqa: F401,F403  (the reference's `from shell import *`)
    from .shell import shell_global_K
    from .constraints import *  # noqa: F401,F403
    from .constraints import ConstraintSet
    from .loads import *  # noqa: F401,F403  (distributed loads, re-exported like the element API)
except ImportError:  # pragma: no cover - flat import from the package directory
    import _capi as C  # type: ignore
    import system as _sys  # type: ignore
    from element import *  # type: ignore # noqa
    from element import _dev, _key, cached_incidence, compute_c3d4_K_matrix, compute_c3d6_K_matrix, \
        compute_c3d8_K_matrix  # type: ignore
    from shell import *  # type: ignore # noqa
    from shell import shell_global_K  # type: ignore
    from constraints import *  # type: ignore # noqa
    from constraints import ConstraintSet  # type: ignore
    from loads import *  # type: ignore # noqa

from collections import OrderedDict

F64 = torch.float64
LONG = torch.long

_GRAPH_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()


def cached_graph(elements: torch.Tensor, n_nodes: int) -> "_sys.Graph":
    """Pattern of `elements` kept across calls (keyed on pointer + version + shape, like a plan cache)."""
    k = _key(elements, n_nodes)
    hit = _GRAPH_CACHE.get(k)
    if hit is not None:
        _GRAPH_CACHE.move_to_end(k)
        return hit[1]
    g = _sys.build_graph(elements, n_nodes)
    _GRAPH_CACHE[k] = (elements, g)
    while len(_GRAPH_CACHE) > 4:
        _GRAPH_CACHE.popitem(last=False)
    return g


def assemble(K, elements, n_nodes, device="cuda:0"):
    """Global operator of one element family: SELL-64 with dpn x dpn blocks (dpn = d / npe)."""
    dev = _dev(device)
    elements = elements.to(device=dev, dtype=LONG).contiguous()
    K = K.to(device=dev, dtype=F64).contiguous()
    dpn = K.shape[-1] // elements.shape[1]
    g = cached_graph(elements, n_nodes)
    return _sys.SellMatrix(g, dpn).add_element_matrices(K, elements)


def _cg_messages(res, style):
    """The reference's prints for each stop (`solver/solver.py:96-133` static, `:187-227` stable CG)."""
    lead = ("\n",) if style == "static" else ()
    if res.status == C.PCG_CONVERGED:
        print(*lead, f"Converged after {res.iterations} iterations. Residual norm: {res.rz:.3e}")
    elif res.status == C.PCG_BREAKDOWN:
        print(*lead, f"Terminating early at iteration {res.iterations}: p^T K p = {res.pq:.3e}, "
              "which is invalid for SPD systems.")
    elif res.status == C.PCG_ALPHA_NAN:
        print(*lead, f"Terminating at iteration {res.iterations}: alpha is NaN or Inf.")
    elif res.status == C.PCG_BETA_NAN:
        print(*lead, f"Terminating at iteration {res.iterations}: beta is NaN or Inf.")
    else:
        print(*lead, "CG did not converge within the maximum number of iterations.")


def _free_mask(n_nodes, dpn, fixed, dev):
    w = torch.ones((n_nodes, dpn), dtype=F64, device=dev)
    if fixed is not None:
        w[torch.as_tensor(fixed).to(device=dev, dtype=LONG)] = 0.0
    return w.view(-1)


# ============================================================================ CG (`solver/solver.py:144-229`)
def stable_conjugate_gradient_solver(K, elements, F, rbe2, u_init=None, tol=1e-10, max_iter=1000, device="cuda:0",
                                     dtype=torch.float64, eps=1e-30, return_info=False):
    """CG on K u = F with the nodes `rbe2` held at zero (u, r, p zeroed there); alpha = rs/(pAp+eps),
    beta = rs_new/(rs_old+eps); stop when sqrt(r.r) < tol (absolute). Returns u [N, dpn]."""
    dev = _dev(device)
    N = F.shape[0]
    A = assemble(K, elements, N, dev)
    w = _free_mask(N, A.bs, rbe2, dev)
    b = F.to(device=dev, dtype=F64).reshape(-1)
    res = A.pcg(b, u_init, w=w, mode=C.MODE_CG_STABLE, tol=tol, max_iter=max_iter, eps=eps)
    _cg_messages(res, "stable")
    u = res.x.view(N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


# ============================================================================ final_solver (`solver/solver.py:231-295`)
def final_solver(K, elements, F, rbe2, u_init=None, tol=1e-10, max_iter=1000, device="cuda:0", dtype=torch.float64,
                 eps=1e-30, return_info=False):
    """The reference's out-of-place CG: the iteration of `stable_conjugate_gradient_solver` (the nodes `rbe2` held
    at zero through a 0/1 mask, alpha = rs/(pAp+eps), beta = rs_new/(rs_old+eps), stop when sqrt(r.r) < tol), the
    same early-stop prints, and no message when max_iter is reached (`:231-295` has no for-else). Runs the same
    device CG (mode CG_STABLE). The reference builds u with requires_grad for autograd through its torch ops; the
    device solve returns a plain tensor."""
    dev = _dev(device)
    N = F.shape[0]
    A = assemble(K, elements, N, dev)
    w = _free_mask(N, A.bs, rbe2, dev)
    b = F.to(device=dev, dtype=F64).reshape(-1)
    res = A.pcg(b, u_init, w=w, mode=C.MODE_CG_STABLE, tol=tol, max_iter=max_iter, eps=eps)
    if res.status != C.PCG_MAXITER:
        _cg_messages(res, "stable")
    u = res.x.view(N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


# ============================================================================ constrained CG (`solver/solver.py:394-759`)
def _constrained_messages(res):
    """`solver/solver.py:566-598` / `:735-757`."""
    if res.status == C.PCG_CONVERGED:
        print(f"[CG] Converged @ iter {res.iterations}, residual norm = {res.rz:.3e}")
    elif res.status == C.PCG_BREAKDOWN:
        print(f"[CG] Early terminate @ iter {res.iterations}: p^T K p = {res.pq:.3e}, not valid for SPD.")
    elif res.status == C.PCG_ALPHA_NAN:
        print(f"[CG] Terminate @ iter {res.iterations}: alpha is NaN/Inf.")
    elif res.status == C.PCG_BETA_NAN:
        print(f"[CG] Terminate @ iter {res.iterations}: beta is NaN/Inf.")
    else:
        print("[CG] Did not converge within max_iter.")


def _constrained_solve(K, elements, F, cons_args, order, u_init, tol, max_iter, device, dtype, eps, return_info):
    dev = _dev(device)
    N = F.shape[0]
    A = assemble(K, elements, N, dev)
    if F.shape[1] != A.bs:
        raise ValueError(f"F is [N, {F.shape[1]}] but the element matrices have {A.bs} dofs per node")
    cs = ConstraintSet(N, A.bs, dev, *cons_args, order=order)
    b = F.to(device=dev, dtype=F64).reshape(-1)
    res = A.pcg(b, u_init, w=cs.mask(), mode=C.MODE_CG_CONSTRAINED, tol=tol, max_iter=max_iter, eps=eps,
                schedule=_sys.SCHED_THREE, constraints=cs)
    _constrained_messages(res)
    u = res.x.view(N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


def constrained_conjugate_gradient_solver(K, elements, F, rbe2_list, spc_list, u_init=None, tol=1e-10, max_iter=1000,
                                          device="cuda:0", dtype=torch.float64, eps=1e-30, return_info=False):
    """CG on the assembled K with RBE2 (slave dofs follow the master) and SPC (prescribed values) enforced after
    every update, residual zeroed on those dofs; r0 = F - K u0 is formed before the first projection, like the
    reference (`solver/solver.py:512-600`). Stop when sqrt(r.r) < tol. Returns u [N, dpn] (fp64 arithmetic)."""
    cons = (parse_spc_list(spc_list, "cpu"), parse_rbe2_list(rbe2_list, "cpu"))  # noqa: F405
    return _constrained_solve(K, elements, F, cons, 0, u_init, tol, max_iter, device, dtype, eps, return_info)


def new_constrained_conjugate_gradient_solver(K, elements, N, rbe2_list, rbe3_list, spc_list, load_list, u_init=None,
                                              tol=1e-10, max_iter=1000, device="cuda:0", dtype=torch.float64,
                                              eps=1e-30, return_info=False):
    """F [N, 3] from the nodal loads, then the constrained CG with SPC, RBE2 and RBE3 (master = weighted mean of
    its slaves per dof) enforced after every update (`solver/solver.py:702-759`)."""
    F = torch.zeros((N, 3), dtype=F64)
    apply_loads_to_F(F, load_list)  # noqa: F405
    cons = (parse_spc_list(spc_list, "cpu"), parse_rbe2_list(rbe2_list, "cpu"),  # noqa: F405
            parse_rbe3_list(rbe3_list, "cpu"))  # noqa: F405
    return _constrained_solve(K, elements, F, cons, 1, u_init, tol, max_iter, device, dtype, eps, return_info)


# ============================================================================ PCG (`solver/solver.py:766-833`)
def _pcg_messages(res):
    """`solver/solver.py:805-811`."""
    if res.status == C.PCG_CONVERGED:
        print(f"Converged after {res.iterations} iterations.")
    else:
        print("Preconditioned CG did not converge within the maximum number of iterations.")


def preconditioned_conjugate_gradient_solver(K, elements, F, M_inv, u_init=None, tol=1e-8, max_iter=1000,
                                             device="cuda:0", dtype=torch.float32, return_info=False):
    """Jacobi-PCG: z = M_inv r, stop when sqrt(r.z) < tol (absolute), no eps and no breakdown guards; fixed DOFs
    are handled only through zeros in M_inv, as in the reference. Returns u [N, dpn].
    Arithmetic is fp64 whatever `dtype` (the reference's default fp32 only sets the output dtype here)."""
    dev = _dev(device)
    N = F.shape[0]
    A = assemble(K, elements, N, dev)
    w = M_inv.to(device=dev, dtype=F64).reshape(-1)
    b = F.to(device=dev, dtype=F64).reshape(-1)
    res = A.pcg(b, u_init, w=w, mode=C.MODE_PCG, tol=tol, max_iter=max_iter)
    _pcg_messages(res)
    u = res.x.view(N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


def compute_diagonal_preconditioner(K, elements, N, device="cuda:0", dtype=torch.float32, exact_diagonal=False):
    """M_inv [N, dpn] of `solver/solver.py:814-833`, inf -> 0.

    By default this reproduces the reference bit for bit, including its slice bug (quirk Q1: `K.view(-1, d)
    [:, ::d+1]` picks column 0 of every element row, `:828`). exact_diagonal=True gives 1/diag(K), the
    function's documented intent (what `solve_tet4` and bench.py use)."""
    lib = C.lib()
    dev = _dev(device)
    elements = elements.to(device=dev, dtype=LONG).contiguous()
    Kd = K.to(device=dev, dtype=F64).contiguous()
    npe = elements.shape[1]
    dpn = Kd.shape[-1] // npe
    inc_ptr, inc = cached_incidence(elements, N)
    diag = torch.empty(N * dpn, dtype=F64, device=dev)
    C.check(lib.fem_ebe_diag(C.ptr(Kd), C.ptr(elements), npe, dpn, C.ptr(inc_ptr), C.ptr(inc), N,
                             0 if exact_diagonal else 1, C.ptr(diag), C.stream(dev)), "fem_ebe_diag")
    minv = torch.empty_like(diag)
    C.check(lib.fem_invert_diag(C.ptr(diag), N * dpn, C.ptr(minv), C.stream(dev)), "fem_invert_diag")
    return minv.view(N, dpn).to(device=torch.device(device), dtype=dtype)


# ============================================================================ static solve (`solver/solver.py:11-135`)
def static_structure_solver(coords, force, fixed, c3d4=None, c3d6=None, c3d8=None, s3=None, s4=None, material=None,
                            u_init=None, tol=1e-10, max_iter=1000, device="cuda:0", dtype=torch.float64, eps=1e-30,
                            return_info=False):
    """Mixed mesh: assemble c3d4 (`compute_c3d4_K_matrix`), c3d8 (8-point rule), c3d6 (single point) and the shells
    s3 / s4 (`compute_s3_K_matrix` / `compute_s4_K_matrix` with material['membrane'], material['bending']) into one
    global operator, then stable CG with `fixed` nodes held at zero in all six columns. u, force are [N, 6]; solids
    use columns 0-2, shells all six. With shells the system has 6 dofs per node on the bs = 3 matrix
    (`system.SixDofMap`); a rotation dof of a node without a shell has no rows: it keeps its u_init value (or 0) and
    a load on it is a ValueError. Without shells the 3-dof path below runs as before."""
    if s3 is not None or s4 is not None:
        return _static_with_shells(coords, force, fixed, c3d4, c3d6, c3d8, s3, s4, material, u_init, tol, max_iter,
                                   device, dtype, eps, return_info)
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    force = force.to(device=dev, dtype=F64)
    N = coords.shape[0]
    if force.shape[1] > 3 and bool((force[:, 3:] != 0).any()):
        raise ValueError("static_structure_solver: rotational loads need shell elements (out of scope)")
    fams = []
    E, nu = material["E"], material["nu"]
    if c3d4 is not None:
        el = c3d4.to(device=dev, dtype=LONG).contiguous()
        fams.append((compute_c3d4_K_matrix(coords, el, E, nu, device=dev, dtype=F64), el))
    if c3d8 is not None:
        el = c3d8.to(device=dev, dtype=LONG).contiguous()
        fams.append((compute_c3d8_K_matrix(coords, el, E, nu, device=dev, dtype=F64), el))
    if c3d6 is not None:
        el = c3d6.to(device=dev, dtype=LONG).contiguous()
        fams.append((compute_c3d6_K_matrix(coords, el, E, nu, device=dev, dtype=F64), el))
    print("Preprocessing done.")
    npe_max = max(el.shape[1] for _, el in fams)
    g = _sys.build_graph(_sys.pad_connectivity([el for _, el in fams], npe_max), N)
    A = _sys.SellMatrix(g, 3)
    for Ke, el in fams:
        A.add_element_matrices(Ke, el, inc=_sys.incidence(el, N))
    u0 = None
    if u_init is not None:
        u0 = u_init.to(device=dev, dtype=F64)[:, :3].contiguous()
    w = _free_mask(N, 3, fixed, dev)
    res = A.pcg(force[:, :3].contiguous(), u0, w=w, mode=C.MODE_CG_STABLE, tol=tol, max_iter=max_iter, eps=eps)
    _cg_messages(res, "static")
    u = torch.zeros((N, 6), dtype=F64, device=dev)
    if u_init is not None:
        u[:, 3:] = u_init.to(device=dev, dtype=F64)[:, 3:]
    u[:, :3] = res.x.view(N, 3)
    u[torch.as_tensor(fixed).to(device=dev, dtype=LONG)] = 0.0
    u = u.to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


def _solid_families(coords, c3d4, c3d6, c3d8, material, dev):
    """(K_e, connectivity) of the solid families present, in the reference's order c3d4, c3d8, c3d6."""
    fams = []
    for el, ke in ((c3d4, compute_c3d4_K_matrix), (c3d8, compute_c3d8_K_matrix), (c3d6, compute_c3d6_K_matrix)):
        if el is not None:
            el = el.to(device=dev, dtype=LONG).contiguous()
            fams.append((ke(coords, el, material["E"], material["nu"], device=dev, dtype=F64), el))
    return fams


def _static_with_shells(coords, force, fixed, c3d4, c3d6, c3d8, s3, s4, material, u_init, tol, max_iter, device, dtype,
                        eps, return_info):
    """static_structure_solver with s3 and / or s4: shell K_e in the global frame, one bs = 3 matrix over the
    translation and rotation blocks, stable CG on one context with the 6-dof free mask."""
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    force = force.to(device=dev, dtype=F64)
    N = coords.shape[0]
    if tuple(force.shape) != (N, 6):
        raise ValueError(f"static_structure_solver: force must be [{N}, 6] with shell elements, got "
                         f"{list(force.shape)}")
    shells = [s.to(device=dev, dtype=LONG).contiguous() for s in (s3, s4) if s is not None]
    dm = _sys.SixDofMap(N, shells)
    if dm.rowless_load(force):
        raise ValueError("static_structure_solver: rotational loads need shell elements on the loaded nodes")
    fams = _solid_families(coords, c3d4, c3d6, c3d8, material, dev)
    shell_fams = [(shell_global_K(coords, s, material["membrane"], material["bending"], device=dev)[0], s)
                  for s in shells]
    print("Preprocessing done.")
    conns = [el for _, el in fams] + [dm.shell_connectivity(s) for _, s in shell_fams]
    g = _sys.build_graph(_sys.pad_connectivity(conns, max(c.shape[1] for c in conns)), dm.n_blocks)
    A = _sys.SellMatrix(g, 3)
    for Ke, el in fams:
        A.add_element_matrices(Ke, el, inc=_sys.incidence(el, dm.n_blocks))
    for Kg, s in shell_fams:
        A.add_shell_matrices(Kg, s, dm)
    base = None if u_init is None else u_init.to(device=dev, dtype=F64)
    u0 = None if base is None else dm.to_blocks(base)
    res = A.pcg(dm.to_blocks(force), u0, w=dm.free_mask(fixed), mode=C.MODE_CG_STABLE, tol=tol, max_iter=max_iter,
                eps=eps, schedule=_sys.SCHED_THREE)
    _cg_messages(res, "static")
    u = dm.from_blocks(res.x, base)
    u[torch.as_tensor(fixed).to(device=dev, dtype=LONG)] = 0.0
    u = u.to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


# ============================================================================ fused mesh -> solution pipeline
def solve_tet4(coords, elements, f, fixed, kind="poisson", E=1.0, nu=0.0, tol=1e-8, max_iter=10000, device="cuda:0",
               rtol=None, reorder=None, operator="assembled", preconditioner="jacobi", n_aggregates=None,
               modulus_scale=None, hierarchy=None, mg_degree=2):
    """Assembly + Jacobi-PCG straight from the mesh (the benchmark pipeline; no element matrices stored):
    c3d4 Poisson (dpn 1, kappa = E) or elasticity (dpn 3), Dirichlet zero on `fixed` nodes via zeros in the
    exact Jacobi M_inv, reference PCG semantics (absolute tol on sqrt(r.z); `rtol` scales it by sqrt(r0.z0)).
    reorder="rcm": solve on the reverse Cuthill-McKee renumbering of the nodes (system.rcm_order; for meshes in
    file order) and return u in the caller's numbering (the returned SellMatrix is the renumbered one).
    preconditioner="two-level" (kind="elastic", operator="assembled" only): the Jacobi weights plus the rigid-body
    coarse correction over `n_aggregates` aggregates (SellMatrix.rigid_coarse_space / pcg_two_level; sqrt(r.z) is then
    measured with the two-level z).
    modulus_scale: a float64 device tensor [M] -- element e has the stiffness modulus_scale[e] K_e(E, nu) (a
    heterogeneous Young's modulus, or conductivity for kind="poisson"; operator="assembled" only).
    preconditioner="multigrid" (operator="assembled" only): a V(mg_degree, mg_degree) cycle over `hierarchy`, a
    topology.MeshHierarchy whose finest level is this mesh (coords / elements must be `hierarchy.fine`); sqrt(r.z) is
    measured with the multigrid z, the system.Multigrid comes back in `res.multigrid`, the SellMatrix is its finest one.
    `device` must be the hierarchy's device. The Multigrid holds every level's matrix and the device context until
    `res.multigrid.close()` (or until the result is dropped); keep it to solve further right-hand sides with
    `res.multigrid.pcg`.
    The hierarchy chose its numbering (no `reorder`), the coarse levels have a constant material (no `modulus_scale`).
    Returns (u [N, dpn], PcgResult, SellMatrix)."""
    if modulus_scale is not None and operator == "matfree":
        raise ValueError("modulus_scale needs operator='assembled': the matrix-free operator has no per-element scale")
    if preconditioner not in ("jacobi", "two-level", "multigrid"):
        raise ValueError(f"unknown preconditioner {preconditioner!r} (supported: 'jacobi', 'two-level', 'multigrid')")
    if preconditioner == "multigrid":
        return _solve_tet4_multigrid(coords, elements, f, fixed, kind, E, nu, tol, max_iter, device, rtol, reorder,
                                     operator, modulus_scale, hierarchy, mg_degree)
    if hierarchy is not None:
        raise ValueError("hierarchy= needs preconditioner='multigrid'")
    if preconditioner == "two-level" and (kind != "elastic" or operator != "assembled"):
        raise ValueError("preconditioner='two-level' needs kind='elastic' and operator='assembled' "
                         f"(got kind={kind!r}, operator={operator!r})")
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    elements = elements.to(device=dev, dtype=LONG).contiguous()
    N = coords.shape[0]
    dpn = 1 if kind == "poisson" else 3
    fixed_mask = torch.zeros(N, dtype=torch.bool, device=dev)
    fixed_mask[torch.as_tensor(fixed).to(device=dev)] = True
    b = f.to(device=dev, dtype=F64).reshape(N, dpn)
    inv = None
    if reorder is not None:
        if reorder != "rcm":
            raise ValueError(f"unknown reorder {reorder!r} (supported: 'rcm')")
        perm, inv = _sys.rcm_order(elements, N)
        coords, elements = _sys.renumber(coords, elements, perm, inv)
        fixed_mask, b = fixed_mask[perm], b[perm]
    if modulus_scale is not None:   # element order is untouched by a node renumbering
        modulus_scale = _sys.check_element_scale("solve_tet4", modulus_scale, elements.shape[0], dev)
    if operator == "matfree":
        A = _sys.MatFreeOperator(coords, elements, kind, E, nu)
    elif modulus_scale is not None:
        A = _sys.assemble_tet4_system(coords, elements, kind, E, nu, scale=modulus_scale)
    else:
        A = _sys.assemble_tet4_system(coords, elements, kind, E, nu)
    A.check_singular()
    mask = torch.zeros((N, A.bs), dtype=torch.uint8, device=dev)
    mask[fixed_mask] = 1
    w = A.jacobi(mask.view(-1))
    b = b.reshape(-1).contiguous().clone()
    if preconditioner == "two-level":
        cs = A.rigid_coarse_space(coords, w, n_aggregates=n_aggregates)
        if rtol is not None:
            tol = float(rtol) * float(torch.sqrt(torch.dot(b, cs.apply(b))))
        res = A.pcg_two_level(b, None, coarse=cs, tol=tol, max_iter=max_iter)
        res.coarse = cs
    else:
        if rtol is not None:
            tol = float(rtol) * float(torch.sqrt(torch.dot(b, w * b)))
        res = A.pcg(b, None, w=w, mode=C.MODE_PCG, tol=tol, max_iter=max_iter)
    u = res.x.view(N, A.bs)
    if inv is not None:
        u = u[inv]
    return u, res, A


def _solve_tet4_multigrid(coords, elements, f, fixed, kind, E, nu, tol, max_iter, device, rtol, reorder, operator,
                          modulus_scale, hierarchy, mg_degree):
    """solve_tet4's preconditioner="multigrid" route."""
    if hierarchy is None:
        raise ValueError("preconditioner='multigrid' needs hierarchy= (topology.refine_c3d4 of the coarse mesh)")
    if operator != "assembled":
        raise ValueError(f"preconditioner='multigrid' needs operator='assembled' (got operator={operator!r}); a "
                         "matrix-free fine level is out of scope")
    if modulus_scale is not None:
        raise ValueError("preconditioner='multigrid' has no modulus_scale: the coarse levels are rediscretised with a "
                         "constant material")
    if reorder is not None:
        raise ValueError("preconditioner='multigrid' takes no reorder=: the hierarchy already chose its numbering "
                         "(refine_c3d4(reorder=...))")
    if kind not in ("poisson", "elastic"):
        raise ValueError(f"preconditioner='multigrid' needs kind 'poisson' (bs = 1) or 'elastic' (bs = 3), got {kind!r}")
    fc, fe = hierarchy.fine
    dev = fc.device
    if _dev(device) != dev:
        raise ValueError(f"preconditioner='multigrid': device={device!r} is not the hierarchy's device {str(dev)!r} "
                         "(the levels live where refine_c3d4 built them)")
    if tuple(coords.shape) != tuple(fc.shape) or tuple(elements.shape) != tuple(fe.shape):
        raise ValueError(f"preconditioner='multigrid': coords / elements must be hierarchy.fine ({list(fc.shape)}, "
                         f"{list(fe.shape)}), got {list(coords.shape)}, {list(elements.shape)}")
    with C.device_scope(dev):
        if not (torch.equal(elements.to(device=dev, dtype=LONG), fe)
                and torch.equal(coords.to(device=dev, dtype=F64), fc)):
            raise ValueError("preconditioner='multigrid': coords / elements differ from hierarchy.fine")
        N = fc.shape[0]
        dpn = 1 if kind == "poisson" else 3
        fixed_mask = torch.zeros(N, dtype=torch.bool, device=dev)
        fixed_mask[torch.as_tensor(fixed).to(device=dev)] = True
        mg = _sys.Multigrid(hierarchy, kind, E, nu, fixed_mask, degree=mg_degree)
        b = f.to(device=dev, dtype=F64).reshape(N, dpn).reshape(-1).contiguous().clone()
        if rtol is not None:
            tol = float(rtol) * float(torch.sqrt(torch.dot(b, mg.apply(b))))
        res = mg.pcg(b, None, tol=tol, max_iter=max_iter)
        res.multigrid = mg
        return res.x.view(N, dpn), res, mg.fine


def multigrid_pcg_solver(hierarchy, F, fixed, kind="elastic", E=1.0, nu=0.0, u_init=None, tol=1e-8, rtol=None,
                         max_iter=1000, degree=2, eig_iters=10, boost=1.1, ratio=30.0, device=None,
                         dtype=torch.float64, return_info=False):
    """PCG on the finest mesh of `hierarchy` (topology.refine_c3d4) with z = one multigrid V(degree, degree) cycle:
    every level assembled from its own mesh with the constant material (E, nu), Chebyshev-Jacobi smoothing on
    [lmax boost / ratio, lmax boost] with lmax from `eig_iters` power iterations, a dense solve on level 0. `fixed`
    are node ids of the finest mesh (hierarchy.carry brings a coarse set there), held at their u_init value, zero by
    default. Stop on sqrt(r.z) < tol (`rtol`: times sqrt(r0.z0)); prints preconditioned_conjugate_gradient_solver's
    messages. Returns u [N, dpn] on `device` (default: the hierarchy's, where the solve always runs); with return_info
    (u, PcgResult) with the system.Multigrid in `.multigrid`, which then lives until its close() or the result is
    dropped -- without return_info it is closed here."""
    fc, _ = hierarchy.fine
    dev = fc.device
    N = fc.shape[0]
    dpn = 1 if kind == "poisson" else 3
    if tuple(F.shape) != (N, dpn):
        raise ValueError(f"multigrid_pcg_solver: F must be [{N}, {dpn}], got {list(F.shape)}")
    with C.device_scope(dev):
        fixed_mask = torch.zeros(N, dtype=torch.bool, device=dev)
        if fixed is not None:
            fixed_mask[torch.as_tensor(fixed).to(device=dev, dtype=LONG)] = True
        mg = _sys.Multigrid(hierarchy, kind, E, nu, fixed_mask, degree=degree, eig_iters=eig_iters, boost=boost,
                            ratio=ratio)
        b = F.to(device=dev, dtype=F64).reshape(-1).contiguous()
        x0 = None if u_init is None else u_init.to(device=dev, dtype=F64).reshape(-1).contiguous()
        if rtol is not None:
            r0 = b if x0 is None else b - mg.fine.matvec(x0)
            tol = float(rtol) * float(torch.sqrt(torch.dot(r0, mg.apply(r0))))
        res = mg.pcg(b, x0, tol=tol, max_iter=max_iter)
        res.multigrid = mg
        _pcg_messages(res)
        out_dev = dev if device is None else torch.device(device)
        u = res.x.view(N, dpn).to(device=out_dev, dtype=dtype)
        if return_info:   # the caller owns the Multigrid (res.multigrid.close() releases the context)
            return u, res
        mg.close()
        return u


# ============================================================================ two-level PCG
def two_level_pcg_solver(K, elements, coords, F, fixed, u_init=None, tol=1e-8, rtol=None, max_iter=1000,
                         n_aggregates=None, device="cuda:0", dtype=torch.float64, return_info=False):
    """PCG on K u = F with M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T: the exact Jacobi weights w (zero on the dofs of the
    `fixed` nodes, which are thereby held at their u_init value, zero by default) plus the rigid-body coarse correction
    over `n_aggregates` aggregates of the free nodes (SellMatrix.rigid_coarse_space). K / elements are one solid family
    with 3 dofs per node, or lists of families on the same nodes (as static_structure_solver assembles them). Stop on
    sqrt(r.z) < tol (`rtol`: times sqrt(r0.z0)); prints preconditioned_conjugate_gradient_solver's messages. Returns
    u [N, 3] (with return_info: (u, PcgResult), the CoarseSpace in `.coarse`)."""
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    N = coords.shape[0]
    fams = list(zip(K, elements)) if isinstance(K, (list, tuple)) else [(K, elements)]
    fams = [(k.to(device=dev, dtype=F64).contiguous(), el.to(device=dev, dtype=LONG).contiguous()) for k, el in fams]
    for k, el in fams:
        if k.shape[-1] != 3 * el.shape[1]:
            raise ValueError(f"two_level_pcg_solver: 3 dofs per node are needed (element matrices of size "
                             f"{k.shape[-1]} for {el.shape[1]} nodes)")
    if tuple(F.shape) != (N, 3):
        raise ValueError(f"two_level_pcg_solver: F must be [{N}, 3], got {list(F.shape)}")
    if len(fams) == 1:
        A = assemble(fams[0][0], fams[0][1], N, dev)
    else:
        g = _sys.build_graph(_sys.pad_connectivity([el for _, el in fams], max(el.shape[1] for _, el in fams)), N)
        A = _sys.SellMatrix(g, 3)
        for k, el in fams:
            A.add_element_matrices(k, el, inc=_sys.incidence(el, N))
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    if fixed is not None:
        mask[torch.as_tensor(fixed).to(device=dev, dtype=LONG)] = 1
    w = A.jacobi(mask.view(-1))
    cs = A.rigid_coarse_space(coords, w, n_aggregates=n_aggregates)
    b = F.to(device=dev, dtype=F64).reshape(-1).contiguous()
    x0 = None if u_init is None else u_init.to(device=dev, dtype=F64).reshape(-1).contiguous()
    if rtol is not None:
        r0 = b if x0 is None else b - A.matvec(x0)
        tol = float(rtol) * float(torch.sqrt(torch.dot(r0, cs.apply(r0))))
    res = A.pcg_two_level(b, x0, coarse=cs, tol=tol, max_iter=max_iter)
    res.coarse = cs
    _pcg_messages(res)
    u = res.x.view(N, 3).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


# ============================================================================ several load cases per matrix
# The structural cases come with several load cases per part (the notebooks' SimJEB `forces` sets), and the reference
# applies K to several vectors by looping `compute_nodal_forces` over them (`solver/solver.py:1151-1168,1207-1216`).
# These solvers run the load cases in lock-step on one assembled matrix (SellMatrix.pcg_multi): the matrix is read once
# per iteration for all load cases of a pass. Each load case is the CG / PCG of the single solver above and prints its message.
def _check_loads(what, F, n_nodes_min, dpn, u_init):
    """ValueError for a load set that does not fit the mesh -- before any device call."""
    if F.dim() != 3:
        raise ValueError(f"{what}: F must be [L, N, dpn] (one [N, dpn] load per case), got {tuple(F.shape)}")
    L, N, d = F.shape
    if L < 1:
        raise ValueError(f"{what}: no load case (F is {tuple(F.shape)})")
    if d != dpn:
        raise ValueError(f"{what}: F is [L, N, {d}] but the operator has {dpn} dofs per node")
    if N < n_nodes_min:
        raise ValueError(f"{what}: F has {N} nodes but the mesh references node {n_nodes_min - 1}")
    if u_init is not None and tuple(u_init.shape) != (L, N, d):
        raise ValueError(f"{what}: u_init must be {(L, N, d)} like F, got {tuple(u_init.shape)}")
    return L, N


def _ke_dpn(what, K, elements):
    if K.dim() != 3 or elements.dim() != 2 or K.shape[-1] % elements.shape[1]:
        raise ValueError(f"{what}: K {tuple(K.shape)} does not fit elements {tuple(elements.shape)}")
    return K.shape[-1] // elements.shape[1]


def _max_node(elements):
    return int(elements.max()) + 1 if elements.numel() else 0


def _to_columns(F, dev):
    """[L, N, dpn] -> the kernels' [N * dpn, L] (the L values of one dof adjacent)."""
    L, N, d = F.shape
    return F.to(device=dev, dtype=F64).permute(1, 2, 0).reshape(N * d, L).contiguous()


def _from_columns(x, N, dpn):
    return x.view(N, dpn, -1).permute(2, 0, 1).contiguous()


def _prefixed(prefix, messages, *args):
    """Print what `messages(*args)` prints, led by `prefix`."""
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        messages(*args)
    print(prefix + buf.getvalue(), end="")


def multi_load_cg_solver(K, elements, F, rbe2, u_init=None, tol=1e-10, max_iter=1000, device="cuda:0",
                         dtype=torch.float64, eps=1e-30, return_info=False):
    """`stable_conjugate_gradient_solver` for L load cases F [L, N, dpn] on one matrix, solved in lock-step; the nodes
    `rbe2` are held at zero in every case. `tol` is a float or one value per load case. Prints, per load case in
    order, the single solver's message led by "Load case j: ". Returns u [L, N, dpn] (with return_info also the
    MultiPcgResult)."""
    what = "multi_load_cg_solver"
    dpn = _ke_dpn(what, K, elements)
    L, N = _check_loads(what, F, _max_node(elements), dpn, u_init)
    dev = _dev(device)
    A = assemble(K, elements, N, dev)
    w = _free_mask(N, A.bs, rbe2, dev)
    x0 = None if u_init is None else _to_columns(u_init, dev)
    res = A.pcg_multi(_to_columns(F, dev), x0, w=w, mode=C.MODE_CG_STABLE, tol=tol, max_iter=max_iter, eps=eps)
    for j in range(L):
        _prefixed(f"Load case {j}: ", _cg_messages, res.column(j), "stable")
    u = _from_columns(res.x, N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


def multi_load_pcg_solver(K, elements, F, M_inv, u_init=None, tol=1e-8, max_iter=1000, device="cuda:0",
                          dtype=torch.float32, return_info=False):
    """`preconditioned_conjugate_gradient_solver` for L load cases F [L, N, dpn] on one matrix and one M_inv [N, dpn],
    solved in lock-step (fp64 arithmetic whatever `dtype`, as the single solver). `tol` is a float or one value per
    load case. Prints, per load case in order, the single solver's message led by "Load case j: ". Returns
    u [L, N, dpn] (with return_info also the MultiPcgResult)."""
    what = "multi_load_pcg_solver"
    dpn = _ke_dpn(what, K, elements)
    L, N = _check_loads(what, F, _max_node(elements), dpn, u_init)
    if M_inv.numel() != N * dpn:
        raise ValueError(f"{what}: M_inv must be [{N}, {dpn}], got {tuple(M_inv.shape)}")
    dev = _dev(device)
    A = assemble(K, elements, N, dev)
    w = M_inv.to(device=dev, dtype=F64).reshape(-1)
    x0 = None if u_init is None else _to_columns(u_init, dev)
    res = A.pcg_multi(_to_columns(F, dev), x0, w=w, mode=C.MODE_PCG, tol=tol, max_iter=max_iter)
    for j in range(L):
        _prefixed(f"Load case {j}: ", _pcg_messages, res.column(j))
    u = _from_columns(res.x, N, A.bs).to(device=torch.device(device), dtype=dtype)
    return (u, res) if return_info else u


def solve_tet4_multi(coords, elements, f, fixed, kind="poisson", E=1.0, nu=0.0, tol=1e-8, max_iter=10000,
                     device="cuda:0", rtol=None):
    """`solve_tet4` for L load cases f [L, N, dpn] (assembled operator only): one assembly, one exact Jacobi M_inv with
    zeros on the `fixed` nodes, the load cases solved in lock-step. `rtol` scales each load case's tolerance by its
    own sqrt(r0.z0). Returns (u [L, N, dpn], MultiPcgResult, SellMatrix)."""
    what = "solve_tet4_multi"
    if kind not in ("poisson", "elastic"):
        raise ValueError(f"{what}: unknown kind {kind!r} ('poisson' or 'elastic')")
    dpn = 1 if kind == "poisson" else 3
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"{what}: coords must be [N, 3], got {tuple(coords.shape)}")
    L, N = _check_loads(what, f, max(_max_node(elements), coords.shape[0]), dpn, None)
    if N != coords.shape[0]:
        raise ValueError(f"{what}: f has {N} nodes but coords {coords.shape[0]}")
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    elements = elements.to(device=dev, dtype=LONG).contiguous()
    A = _sys.assemble_tet4_system(coords, elements, kind, E, nu)
    A.check_singular()
    mask = torch.zeros((N, A.bs), dtype=torch.uint8, device=dev)
    mask[torch.as_tensor(fixed).to(device=dev)] = 1
    w = A.jacobi(mask.view(-1))
    B = _to_columns(f, dev)
    if rtol is not None:
        tol = [float(rtol) * float(t) for t in torch.sqrt((B * (w[:, None] * B)).sum(0)).cpu()]
    res = A.pcg_multi(B, None, w=w, mode=C.MODE_PCG, tol=tol, max_iter=max_iter)
    return _from_columns(res.x, N, A.bs), res, A


# ============================================================================ modal analysis (`solver/solver.py:1084-1313`)
# The reference's routine iterates M^-1 K forward from torch.randn, orthonormalises in the Euclidean norm and solves
# the small problem with 30 Jacobi rotations on a non-symmetric matrix: it drifts to the LARGEST eigenvalues although
# its docstring promises the smallest. These solvers deliver what the docstring promises -- the lowest eigenpairs of the
# clamped structure, M-orthonormal -- by block LOBPCG on the assembled matrices (SellMatrix.eig_lowest, csrc/modal.hip);
# parity is pinned against a dense generalised eigensolve, not against the reference's iterates.
def _check_modal(what, K, M, elements, num_nodes, k, mass_dims):
    """ValueError for element matrices that do not fit the mesh -- before any device call. Returns dofs per node."""
    dpn = _ke_dpn(what, K, elements)
    if dpn not in (1, 3):
        raise ValueError(f"{what}: {dpn} dofs per node unsupported (1 or 3)")
    npe = elements.shape[1]
    if K.shape[0] != elements.shape[0] or K.shape[1] != K.shape[2]:
        raise ValueError(f"{what}: K {tuple(K.shape)} does not fit elements {tuple(elements.shape)}")
    if M.dim() != 3 or M.shape[0] != elements.shape[0] or M.shape[1] != M.shape[2] or \
            M.shape[1] not in [npe * d for d in mass_dims(dpn)]:
        raise ValueError(f"{what}: M {tuple(M.shape)} does not fit elements {tuple(elements.shape)} "
                         f"with {dpn} dofs per node")
    if not 1 <= int(k) <= 8:
        raise ValueError(f"{what}: 1 to 8 eigenpairs per solve, got {k}")
    if _max_node(elements) > num_nodes:
        raise ValueError(f"{what}: the mesh references node {_max_node(elements) - 1} but num_nodes is {num_nodes}")
    return dpn


def _fixed_ids(what, fixed, num_nodes):
    ids = torch.as_tensor(fixed).to(LONG).reshape(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= num_nodes):
        raise ValueError(f"{what}: a fixed node lies outside [0, {num_nodes})")
    return ids


def _jacobi_weights(A, ids, dev):
    mask = torch.zeros((A.g.n_nodes, A.bs), dtype=torch.uint8, device=dev)
    mask[ids.to(dev)] = 1
    return A.jacobi(mask.view(-1))


def vectorized_modal_solver(K_local, M_local, elements, rbe2_node_ids, num_nodes, num_eigs=5, max_iter=20,
                            device="cuda:0", dtype=torch.float32, tol=1e-8, return_info=False):
    """The `num_eigs` lowest eigenpairs of K u = lambda M u with the nodes `rbe2_node_ids` clamped: signature and
    returns of the reference (`solver/solver.py:1084-1313`: lam [num_eigs], modes [3 num_nodes, num_eigs], in `dtype`),
    fp64 arithmetic. The mass is lumped the reference's way -- the sum of the element matrices' diagonals, clamped at
    1e-12 (`:1126-1134`) -- and applied as a diagonal. `max_iter` caps the LOBPCG iterations; when it is hit one line
    `Modal solver: reached max_iter (N) with residual R` is printed and the current Ritz pairs are returned. The
    modes are M-orthonormal with zeros on the clamped dofs. A free-free structure (nothing clamped) is out of scope:
    the solve stops with PCG_BREAKDOWN (see SellMatrix.eig_lowest). With return_info also the ModalResult."""
    what = "vectorized_modal_solver"
    dpn = _check_modal(what, K_local, M_local, elements, num_nodes, num_eigs, lambda d: (d,))
    if dpn != 3:
        raise ValueError(f"{what}: 3 dofs per node (the reference's layout), got {dpn}")
    ids = _fixed_ids(what, rbe2_node_ids, num_nodes)
    dev = _dev(device)
    A = assemble(K_local, elements, num_nodes, dev)
    el = elements.to(device=dev, dtype=LONG)
    dofs = (el.unsqueeze(-1) * 3 + torch.arange(3, device=dev).view(1, 1, 3)).reshape(-1)
    md = torch.zeros(3 * num_nodes, dtype=F64, device=dev)
    md.index_add_(0, dofs, M_local.to(device=dev, dtype=F64).diagonal(dim1=1, dim2=2).reshape(-1))
    md.clamp_(min=1e-12)
    res = A.eig_lowest(md, int(num_eigs), _jacobi_weights(A, ids, dev), tol=tol, max_iter=max_iter)
    if res.status == C.PCG_MAXITER:
        print(f"Modal solver: reached max_iter ({max_iter}) with residual {float(res.residuals.max()):.3e}")
    elif res.status == C.PCG_BREAKDOWN:
        print(f"Modal solver: breakdown at iteration {res.iterations} (K is not positive definite on the free dofs)")
    lam = res.lam.to(device=torch.device(device), dtype=dtype)
    modes = res.X.to(device=torch.device(device), dtype=dtype)
    return (lam, modes, res) if return_info else (lam, modes)


def modal_solver(K, M, elements, fixed, num_nodes, num_modes=6, tol=1e-8, max_iter=2000, block=None, seed=0,
                 device="cuda:0", dtype=torch.float64, return_info=False):
    """Natural frequencies with the consistent mass: the `num_modes` lowest eigenpairs of K u = lambda M u with the
    nodes `fixed` clamped. K [Me, d, d] (d = dpn npe, dpn 1 or 3); M is the scalar factor [Me, npe, npe]
    (compute_M_matrix(..., scalar=True)) or the full [Me, dpn npe, dpn npe] of compute_c3d4_M_matrix / compute_M_matrix,
    from which the factor M[:, ::dpn, ::dpn] is taken. Both matrices are assembled on one cached graph. Returns
    (freq_hz = sqrt(lam) / 2 pi [num_modes], lam [num_modes], modes [num_modes, N, dpn]) in `dtype` and prints one
    line per mode; with return_info also the ModalResult."""
    return _modal_solve("modal_solver", K, M, elements, fixed, num_nodes, num_modes, tol, max_iter, block, seed, device,
                        dtype, return_info)


def _modal_solve(what, K, M, elements, fixed, num_nodes, num_modes, tol, max_iter, block, seed, device, dtype,
                 return_info, Gs=None, load_factor=0.0):
    """modal_solver; with Gs [Me, npe, npe] on K + load_factor K_g (stress_stiffened_modal_solver)."""
    dpn = _check_modal(what, K, M, elements, num_nodes, num_modes, lambda d: (1, d))
    if Gs is not None:
        npe = elements.shape[1]
        if dpn != 3:
            raise ValueError(f"{what}: 3 dofs per node needed, got {dpn}")
        if not torch.is_tensor(Gs) or tuple(Gs.shape) != (elements.shape[0], npe, npe):
            shape = list(Gs.shape) if torch.is_tensor(Gs) else type(Gs).__name__
            raise ValueError(f"{what}: Gs must be the scalar factor [{elements.shape[0]}, {npe}, {npe}], got {shape}")
    ids = _fixed_ids(what, fixed, num_nodes)
    _sys.modal_block(num_modes, block)
    dev = _dev(device)
    el = elements.to(device=dev, dtype=LONG).contiguous()
    npe = el.shape[1]
    Ke = K.to(device=dev, dtype=F64).contiguous()
    Ms = M.to(device=dev, dtype=F64)
    if Ms.shape[1] != npe:
        Ms = Ms[:, ::dpn, ::dpn]
    Ms = Ms.contiguous()
    g = cached_graph(el, num_nodes)
    A, Mg = _sys.SellMatrix(g, dpn), _sys.SellMatrix(g, 1)
    if dpn == 3:
        A.add_stiffness_and_mass(Ke, Ms, el, Mg)
    else:
        A.add_element_matrices(Ke, el)
        Mg.add_element_matrices(Ms, el)
    if Gs is not None:   # K + load_factor K_g, K_g = G (x) I3 with G assembled like the scalar mass
        Gg = _sys.SellMatrix(g, 1).add_element_matrices(Gs.to(device=dev, dtype=F64).contiguous(), el)
        A = A.scaled_add_mass(Gg, 1.0, float(load_factor))
    res = A.eig_lowest(Mg, int(num_modes), _jacobi_weights(A, ids, dev), block=block, tol=tol, max_iter=max_iter,
                       seed=seed)
    if res.status == C.PCG_MAXITER:
        print(f"Modal solver: reached max_iter ({max_iter}) with residual {float(res.residuals.max()):.3e}")
    elif res.status == C.PCG_BREAKDOWN:
        print(f"Modal solver: breakdown at iteration {res.iterations} (K is not positive definite on the free dofs)")
    freq = torch.sqrt(res.lam.clamp(min=0.0)) / (2.0 * torch.pi)
    for j in range(int(num_modes)):
        print(f"Mode {j + 1}: f = {float(freq[j]):.6e} Hz, lambda = {float(res.lam[j]):.6e}, "
              f"residual {float(res.residuals[j]):.3e}")
    out = torch.device(device)
    modes = res.X.T.reshape(int(num_modes), num_nodes, dpn)
    ret = (freq.to(device=out, dtype=dtype), res.lam.to(device=out, dtype=dtype), modes.to(device=out, dtype=dtype))
    return ret + (res,) if return_info else ret


# ============================================================================ linear buckling
# The reference has no stability analysis. Linear (eigenvalue) buckling of the solid elements: the reference state
# K u_ref = F (or a given prestress), its geometric stiffness K_g = G (x) I3 from csrc/buckling.hip, and the load factors
# lambda of (K + lambda K_g) phi = 0 by SellMatrix.buckling_lowest.
_BUCKLING_NPE = {"c3d4": 4, "c3d6": 6, "c3d8": 8, "c3d10": 10}
_CENTROID = {"c3d8": (0.0, 0.0, 0.0), "c3d6": (1.0 / 3.0, 1.0 / 3.0, 0.0), "c3d10": (0.25, 0.25, 0.25)}


def _buckling_families(what, elements, element_type):
    """[(type, connectivity)] of `elements` / `element_type` (one family, or a dict {type: connectivity})."""
    if isinstance(elements, dict):
        fams = [(str(t).lower(), el) for t, el in elements.items()]
    elif isinstance(element_type, dict):
        fams = [(str(t).lower(), el) for t, el in element_type.items()]
    else:
        fams = [(str(element_type).lower(), elements)]
    if not fams:
        raise ValueError(f"{what}: no element family given")
    for et, el in fams:
        if et not in _BUCKLING_NPE:
            raise ValueError(f"Unsupported element type: {et}")
        if not torch.is_tensor(el) or el.dim() != 2 or el.shape[1] != _BUCKLING_NPE[et] or el.shape[0] < 1:
            shape = list(el.shape) if torch.is_tensor(el) else type(el).__name__
            raise ValueError(f"{what}: {et} connectivity must be [M, {_BUCKLING_NPE[et]}] with M >= 1, got {shape}")
    return fams


def _check_buckling(what, coords, fams, F, fixed, E, nu, k, prestress, u_ref, tol, max_iter, linear_tol,
                    linear_max_iter, block):
    """ValueError for arguments that do not fit -- before any device call. Returns the fixed node ids."""
    if not torch.is_tensor(coords) or coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"{what}: coords must be [N, 3]")
    N = coords.shape[0]
    if max(_max_node(el) for _, el in fams) > N:
        raise ValueError(f"{what}: the mesh references a node outside the {N} coordinates")
    if F is None and prestress is None and u_ref is None:
        raise ValueError(f"{what}: a load F, a reference displacement u_ref or a prestress is needed")
    if F is not None and tuple(F.shape) != (N, 3):
        raise ValueError(f"{what}: F must be [{N}, 3], got {list(F.shape)}")
    if u_ref is not None and tuple(u_ref.shape) != (N, 3):
        raise ValueError(f"{what}: u_ref must be [{N}, 3], got {list(u_ref.shape)}")
    if prestress is not None:
        ps = prestress if isinstance(prestress, dict) else {fams[0][0]: prestress}
        if len(fams) > 1 and not isinstance(prestress, dict):
            raise ValueError(f"{what}: a mixed mesh takes prestress as a dict {{type: [M, 3, 3]}}")
        for et, el in fams:
            p = ps.get(et)
            if p is not None and tuple(p.shape) != (el.shape[0], 3, 3):
                raise ValueError(f"{what}: prestress of {et} must be [{el.shape[0]}, 3, 3], got {list(p.shape)}")
        if set(ps) - {et for et, _ in fams}:
            raise ValueError(f"{what}: prestress for a family that is not in the mesh: {sorted(set(ps))}")
    if not (float(E) > 0.0 and -1.0 < float(nu) < 0.5):
        raise ValueError(f"{what}: E > 0 and -1 < nu < 0.5 needed, got E = {E}, nu = {nu}")
    _sys.modal_block(k, block)
    if not (tol > 0 and linear_tol > 0 and int(max_iter) >= 0 and int(linear_max_iter) >= 1):
        raise ValueError(f"{what}: tol, linear_tol > 0, max_iter >= 0 and linear_max_iter >= 1 needed")
    ids = _fixed_ids(what, fixed, N)
    if ids.numel() == 0:
        raise ValueError(f"{what}: at least one fixed node is needed (K must be positive definite)")
    return ids


def _buckling_ke(coords, el, et, E, nu, dev):
    """Stiffness [M, 3 npe, 3 npe] of one solid family for the buckling pencil, integrated with |detJ| over a rule
    whose weights sum to the reference element's volume: c3d4 closed form, c3d8 the 2x2x2 rule, c3d6 / c3d10 the rules
    of mass_integration_points (the reference's own c3d6 / c3d10 stiffness rules sum to 2 and 0.45, Q3 / Q2, and its
    signed detJ makes K negative on VTK-positive quadratic tets: neither gives a physical load factor)."""
    if et == "c3d4":
        return compute_c3d4_K_matrix(coords, el, E, nu, device=dev, dtype=F64)
    if et == "c3d8":
        Ke = compute_c3d8_K_matrix(coords, el, E, nu, device=dev, dtype=F64)
    else:
        p, w = mass_integration_points(et)
        ip = torch.cat([p, w[:, None]], dim=1)
        fn = compute_c3d6_K_matrix if et == "c3d6" else compute_c3d10_K_matrix
        Ke = fn(coords, el, E, nu, integral_point=ip, single=(et == "c3d10"), device=dev, dtype=F64)
    J = compute_Jacobian(coords, el, et, torch.tensor(_CENTROID[et], dtype=F64), device=dev).to(F64)
    return Ke * torch.sign(torch.linalg.det(J)).view(-1, 1, 1)


def linear_buckling_solver(coords, elements, element_type, F, fixed, E, nu, num_modes=4, prestress=None, u_ref=None,
                           tol=1e-8, max_iter=200, linear_tol=1e-10, linear_max_iter=10000, block=None, seed=0,
                           device="cuda:0", dtype=torch.float64, return_info=False):
    """Linear (eigenvalue) buckling of a solid mesh with the nodes `fixed` clamped: the `num_modes` load factors lambda
    of smallest magnitude by which the reference load may be scaled before (K + lambda K_g) phi = 0 has a solution, and
    their shapes. The reference state is K u_ref = F [N, 3] by Jacobi-PCG (to `linear_tol` relative, `linear_max_iter`),
    or `u_ref` [N, 3] when supplied; `prestress` [M, 3, 3] (per-element stress, e.g. of compute_thermal_element_stress)
    is added to its stress, and with F = None and no u_ref it is the whole reference state. `elements` is one
    connectivity with `element_type` in c3d4 / c3d6 / c3d8 / c3d10, or a dict {type: connectivity} of a mixed mesh
    (`prestress` then a dict too); every family adds into the same K and G. A negative factor means the load buckles
    the structure when reversed. Returns (load_factors [num_modes] signed, ascending in magnitude, modes
    [num_modes, N, 3] K-orthonormal, u_ref [N, 3]) in `dtype` and prints one line per mode; with return_info also the
    BucklingResult. Never raises on non-convergence: one line tells the outer cap from a failed inner solve, and a
    state without prestress (G = 0) is reported as a breakdown."""
    what = "linear_buckling_solver"
    fams = _buckling_families(what, elements, element_type)
    ids = _check_buckling(what, coords, fams, F, fixed, E, nu, num_modes, prestress, u_ref, tol, max_iter, linear_tol,
                          linear_max_iter, block)
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    N = coords.shape[0]
    fams = [(et, el.to(device=dev, dtype=LONG).contiguous()) for et, el in fams]
    if len(fams) == 1:
        g = cached_graph(fams[0][1], N)
    else:
        g = _sys.build_graph(_sys.pad_connectivity([el for _, el in fams], max(el.shape[1] for _, el in fams)), N)
    incs = [None if len(fams) == 1 else _sys.incidence(el, N) for _, el in fams]
    A, G = _sys.SellMatrix(g, 3), _sys.SellMatrix(g, 1)
    for (et, el), inc in zip(fams, incs):
        A.add_element_matrices(_buckling_ke(coords, el, et, E, nu, dev), el, inc=inc)
    w = _jacobi_weights(A, ids, dev)
    if u_ref is not None:
        u = u_ref.to(device=dev, dtype=F64).contiguous()
    elif F is not None:
        b = (F.to(device=dev, dtype=F64) * (w.view(N, 3) != 0)).reshape(-1).contiguous()
        scale = float(torch.sqrt(torch.dot(b, w * b)))
        if scale > 0.0:
            res0 = A.pcg(b, None, w=w, mode=C.MODE_PCG, tol=float(linear_tol) * scale, max_iter=int(linear_max_iter))
            if res0.status != C.PCG_CONVERGED:
                print(f"Buckling solver: the reference solve did not converge in {linear_max_iter} iterations")
            u = res0.x.view(N, 3)
        else:   # no load on a free dof: the reference state is zero
            u = torch.zeros((N, 3), dtype=F64, device=dev)
    else:
        u = None
    ps = {} if prestress is None else (prestress if isinstance(prestress, dict) else {fams[0][0]: prestress})
    for (et, el), inc in zip(fams, incs):
        Gs = compute_geometric_stiffness(coords, el, et, displacement=u, E=E, nu=nu, prestress=ps.get(et), device=dev,
                                         dtype=F64) if (u is not None or ps.get(et) is not None) else \
            torch.zeros((el.shape[0], el.shape[1], el.shape[1]), dtype=F64, device=dev)
        G.add_element_matrices(Gs, el, inc=inc)
    res = A.buckling_lowest(G, int(num_modes), w, block=block, tol=tol, max_iter=max_iter, linear_tol=linear_tol,
                            linear_max_iter=linear_max_iter, seed=seed)
    if res.status == C.PCG_MAXITER and res.inner_failed:
        print(f"Buckling solver: an inner solve did not converge in {linear_max_iter} iterations "
              f"(outer iteration {res.iterations + 1})")
    elif res.status == C.PCG_MAXITER:
        print(f"Buckling solver: reached max_iter ({max_iter}) with residual {float(res.residuals.max()):.3e}")
    elif res.status == C.PCG_BREAKDOWN:
        print(f"Buckling solver: breakdown at iteration {res.iterations} (no prestress, or K is not positive definite "
              "on the free dofs)")
    for j in range(int(num_modes)):
        print(f"Mode {j + 1}: load factor = {float(res.factors[j]):.6e}, theta = {float(res.theta[j]):.6e}, "
              f"residual {float(res.residuals[j]):.3e}")
    out = torch.device(device)
    modes = res.X.T.reshape(int(num_modes), N, 3)
    u_out = torch.zeros((N, 3), dtype=F64, device=dev) if u is None else u
    ret = (res.factors.to(device=out, dtype=dtype), modes.to(device=out, dtype=dtype),
           u_out.to(device=out, dtype=dtype))
    return ret + (res,) if return_info else ret


def stress_stiffened_modal_solver(K, M, Gs, elements, fixed, num_nodes, load_factor=1.0, num_modes=6, tol=1e-8,
                                  max_iter=2000, block=None, seed=0, device="cuda:0", dtype=torch.float64,
                                  return_info=False):
    """Natural frequencies of a prestressed structure: modal_solver on K + load_factor K_g in the place of K, with
    Gs [Me, npe, npe] the scalar factor of the geometric stiffness at the reference load
    (compute_geometric_stiffness(..., scalar=True)); K [Me, 3 npe, 3 npe], M, elements, fixed, num_nodes and the keyword
    arguments as modal_solver's, same returns and prints. The effective stiffness is
    SellMatrix.scaled_add_mass(G, 1, load_factor): no kernel of its own. Compression softens: the frequencies go to zero
    as `load_factor` approaches the first buckling factor of linear_buckling_solver (beyond it K + load_factor K_g is
    indefinite and the solve reports a breakdown); tension stiffens."""
    return _modal_solve("stress_stiffened_modal_solver", K, M, elements, fixed, num_nodes, num_modes, tol, max_iter,
                        block, seed, device, dtype, return_info, Gs=Gs, load_factor=load_factor)


# ============================================================================ transient dynamics
# The reference stops at modes; the response in time M a + C v + K u = f(t) is integrated here by the implicit Newmark
# scheme on the assembled matrices (system.NewmarkIntegrator, csrc/transient.hip).
def _check_transient(what, K, M, elements, F, fixed, num_nodes, dt, steps, amplitude, u0, v0, beta, gamma, damping,
                     record, energy_every, rtol):
    """Every ValueError of transient_solver -- before any device call. Returns (dpn, fixed ids, record ids, history)."""
    dpn = _check_modal(what, K, M, elements, num_nodes, 1, lambda d: (1, d))
    if int(steps) < 1:
        raise ValueError(f"{what}: steps must be >= 1, got {steps}")
    _sys.newmark_constants(dt, beta, gamma, damping)
    if rtol is not None and not float(rtol) > 0.0:
        raise ValueError(f"{what}: rtol must be > 0, got {rtol}")
    if int(energy_every) < 0:
        raise ValueError(f"{what}: energy_every must be >= 0, got {energy_every}")
    shape = tuple(F.shape) if torch.is_tensor(F) else None
    history = shape is not None and len(shape) == 3
    if shape not in ((num_nodes, dpn), (int(steps) + 1, num_nodes, dpn)):
        raise ValueError(f"{what}: F must be [{num_nodes}, {dpn}] or the history [{int(steps) + 1}, {num_nodes}, {dpn}]"
                         f", got {shape}")
    if amplitude is not None:
        if history:
            raise ValueError(f"{what}: a load history [steps + 1, N, dpn] takes no amplitude")
        if torch.is_tensor(amplitude):
            if amplitude.dim() != 1 or amplitude.numel() != int(steps) + 1:
                raise ValueError(f"{what}: amplitude must hold steps + 1 = {int(steps) + 1} values (t_0 .. t_steps), "
                                 f"got {tuple(amplitude.shape)}")
        elif not callable(amplitude):
            raise ValueError(f"{what}: amplitude must be None, a tensor [steps + 1] or a callable of t")
    for name, x in (("u0", u0), ("v0", v0)):
        if x is not None and (not torch.is_tensor(x) or tuple(x.shape) != (num_nodes, dpn)):
            raise ValueError(f"{what}: {name} must be [{num_nodes}, {dpn}]")
    ids = _fixed_ids(what, fixed, num_nodes)
    rec = None
    if record is not None:
        rec = torch.as_tensor(record).to(LONG).reshape(-1)
        if rec.numel() and (int(rec.min()) < 0 or int(rec.max()) >= num_nodes):
            raise ValueError(f"{what}: a recorded node lies outside [0, {num_nodes})")
    return dpn, ids, rec, history


def transient_solver(K, M, elements, F, fixed, num_nodes, dt, steps, amplitude=None, u0=None, v0=None,
                     beta=0.25, gamma=0.5, damping=(0.0, 0.0), lumped=False, tol=1e-8, rtol=None, max_iter=1000,
                     record=None, energy_every=0, callback=None, predictor=False,
                     device="cuda:0", dtype=torch.float64, return_info=False):
    """Response in time of M a + C v + K u = f(t), C = alpha M + beta_R K with damping = (alpha, beta_R), over `steps`
    steps of `dt` by implicit Newmark-beta (default: average acceleration) with the nodes `fixed` held at zero.
    K and M as in modal_solver (M the scalar factor or the full element mass; dpn 1 or 3; both assembled on the cached
    graph); lumped=True uses the reference's lumped diagonal (the element matrices' diagonals summed per dof, clamped
    at 1e-12, `solver/solver.py:1126-1134`). F is [N, dpn] scaled by `amplitude` (None: constant, i.e. suddenly
    applied; a tensor [steps + 1] of the values at t_0 .. t_steps; or a callable of t), or the history [steps + 1, N,
    dpn]. Every step solves K_eff u = b by Jacobi-PCG on one solver context, warm-started from u_n (predictor: from
    u_n + dt v_n), to `tol` absolute on sqrt(r.z) or, with `rtol`, to rtol sqrt(b.(w o b)) of the step.
    record: node ids whose u, v, a come back as [steps + 1, len(record), dpn]; callback(step, t, u, v, a) gets views of
    the device state ([N dpn]); the full field history is the caller's choice. A step that does not converge stops
    the run with one printed line; the state of the last converged step is returned.
    Returns (u, v, a) [N, dpn] at the last step in `dtype`; with return_info also a system.TransientResult whose
    recorded rows are shaped [steps done + 1, len(record), dpn]."""
    what = "transient_solver"
    dpn, ids, rec, history = _check_transient(what, K, M, elements, F, fixed, num_nodes, dt, steps, amplitude, u0, v0,
                                              beta, gamma, damping, record, energy_every, rtol)
    steps = int(steps)
    dev = _dev(device)
    el = elements.to(device=dev, dtype=LONG).contiguous()
    npe = el.shape[1]
    Ke = K.to(device=dev, dtype=F64).contiguous()
    Mf = M.to(device=dev, dtype=F64)
    g = cached_graph(el, num_nodes)
    A = _sys.SellMatrix(g, dpn)
    if lumped:
        md = Mf.diagonal(dim1=1, dim2=2)                      # [Me, npe] or [Me, dpn npe]
        if Mf.shape[1] == npe and dpn > 1:
            md = md.repeat_interleave(dpn, dim=1)
        dofs = (el.unsqueeze(-1) * dpn + torch.arange(dpn, device=dev).view(1, 1, dpn)).reshape(-1)
        mass = torch.zeros(dpn * num_nodes, dtype=F64, device=dev)
        mass.index_add_(0, dofs, md.reshape(-1))
        mass.clamp_(min=1e-12)
        A.add_element_matrices(Ke, el)
    else:
        Ms = (Mf if Mf.shape[1] == npe else Mf[:, ::dpn, ::dpn]).contiguous()
        mass = _sys.SellMatrix(g, 1)
        if dpn == 3:
            A.add_stiffness_and_mass(Ke, Ms, el, mass)
        else:
            A.add_element_matrices(Ke, el)
            mass.add_element_matrices(Ms, el)
    mask = torch.zeros((num_nodes, dpn), dtype=torch.uint8, device=dev)
    mask[ids.to(dev)] = 1
    integ = _sys.NewmarkIntegrator(A, mass, mask.view(-1), dt, beta, gamma, damping, tol=tol, rtol=rtol,
                                   max_iter=max_iter, predictor=predictor)
    try:
        Fd = F.to(device=dev, dtype=F64).reshape(-1, num_nodes * dpn).contiguous()
        if history:
            amps = [1.0] * (steps + 1)
        elif amplitude is None:
            amps = [1.0] * (steps + 1)
        elif torch.is_tensor(amplitude):
            amps = [float(x) for x in amplitude.to(dtype=F64).cpu()]
        else:
            amps = [float(amplitude(k * float(dt))) for k in range(steps + 1)]
        vec = lambda x: None if x is None else x.reshape(-1)
        integ.start(vec(u0), vec(v0), amps[0] * Fd[0])
        load = (lambda k: (Fd[k], 1.0)) if history else (lambda k: (Fd[0], amps[k]))
        rdofs = None
        if rec is not None:
            rdofs = (rec.to(dev).unsqueeze(-1) * dpn + torch.arange(dpn, device=dev)).reshape(-1)
        res = integ.run(steps, load, record=rdofs, energy_every=int(energy_every), callback=callback)
        if rec is not None:
            res.rec_u, res.rec_v, res.rec_a = (r.reshape(r.shape[0], -1, dpn) for r in (res.rec_u, res.rec_v, res.rec_a))
        out = torch.device(device)
        ret = tuple(x.view(num_nodes, dpn).to(device=out, dtype=dtype).clone() for x in (integ.u, integ.v, integ.a))
    finally:
        integ.close()
    return ret + (res,) if return_info else ret


# ============================================================================ explicit dynamics
# Impact, wave propagation and fast large-deformation loading: central differences with the lumped mass on the element
# chunks (system.ExplicitDynamics, csrc/explicit.hip). No matrix, no linear solve; the step size comes from
# the mesh. No counterpart in the reference.
def _check_explicit(what, coords, elements, F, fixed, rho, E, nu, steps, dt, safety, material, amplitude, u0, v0,
                    damping, record, energy_every):
    """Every ValueError of explicit_dynamics_solver -- before any device call. Returns (fixed-dof mask [N,3] bool on
    the host, record node ids or None)."""
    N, _ = _sys.check_explicit_mesh(what, coords, elements, rho, E, nu)
    if elements.numel() and (int(elements.min()) < 0 or _max_node(elements) > N):
        raise ValueError(f"{what}: the mesh references a node outside [0, {N})")
    if material not in C.EXPLICIT_MATERIALS:
        raise ValueError(f"{what}: unknown material {material!r} (supported: "
                         f"{', '.join(sorted(C.EXPLICIT_MATERIALS))})")
    _sys.check_explicit_run(what, steps, dt)
    steps = int(steps)
    if dt is None and not 0.0 < float(safety) <= 1.0:
        raise ValueError(f"{what}: safety must lie in (0, 1], got {safety}")
    if not float(damping) >= 0.0:
        raise ValueError(f"{what}: damping must be >= 0, got {damping}")
    if int(energy_every) < 0:
        raise ValueError(f"{what}: energy_every must be >= 0, got {energy_every}")
    if not torch.is_tensor(F) or tuple(F.shape) != (N, 3):
        raise ValueError(f"{what}: F must be [{N}, 3], got {tuple(getattr(F, 'shape', ()))}")
    if amplitude is not None:
        if torch.is_tensor(amplitude):
            if amplitude.dim() != 1 or amplitude.numel() != steps + 1:
                raise ValueError(f"{what}: amplitude must hold steps + 1 = {steps + 1} values (t_0 .. t_steps), "
                                 f"got {tuple(amplitude.shape)}")
        elif not callable(amplitude):
            raise ValueError(f"{what}: amplitude must be None, a tensor [steps + 1] or a callable of t")
    for name, x in (("u0", u0), ("v0", v0)):
        if x is not None and (not torch.is_tensor(x) or tuple(x.shape) != (N, 3)):
            raise ValueError(f"{what}: {name} must be [{N}, 3]")
    mask = _fixed_mask(what, fixed, N)
    rec = None
    if record is not None:
        rec = torch.as_tensor(record).to(LONG).reshape(-1)
        if rec.numel() and (int(rec.min()) < 0 or int(rec.max()) >= N):
            raise ValueError(f"{what}: a recorded node lies outside [0, {N})")
    return mask, rec


def explicit_dynamics_solver(coords, elements, F, fixed, rho, E, nu, steps, dt=None, safety=0.9, material="linear",
                             amplitude=None, u0=None, v0=None, damping=0.0, record=None, energy_every=0,
                             device="cuda:0", dtype=torch.float64, return_info=False, contact=None, penalty=0.5,
                             contact_every=0):
    """Response in time of a c3d4 mesh under M a + alpha M v + f_int(u) = amp(t) F by explicit central differences
    (leapfrog) with the lumped mass, `steps` steps of `dt`. material: "linear" (small strain), "svk" or "neo_hookean"
    (total Lagrangian, as nonlinear_static_solver); uniform rho, E, nu; damping = alpha (mass-proportional).
    fixed: node ids, or a bool / uint8 [N,3] mask of single dofs (rollers). dt=None takes safety x the guaranteed
    stable step of compute_c3d4_stable_time_step (a bound for the linear operator: a stiffening nonlinear response may
    need less); a given dt is used as is. F, amplitude (None: suddenly applied; a tensor [steps + 1] of the values at
    t_0 .. t_steps; a callable of t), u0, v0 and record (node ids -> [steps + 1, len(record), 3]) as transient_solver.
    An element that inverts (det F <= 0: it then carries no force) or a non-finite value does not stop the run: one line
    `Explicit solver: ...` is printed and the state reached is returned; system.ExplicitResult.status tells.
    contact: a list of up to 8 system.RigidSurface (planes, spheres, cylinders, solid or cavity, fixed or translating)
    the nodes may not penetrate: frictional penalty contact with the normal stiffness penalty x m_i / dt^2 (DESIGN
    §8v). With dt=None penalty may not exceed 4 (1 - safety^2), which keeps the step stable. contact_every = m > 0
    keeps each surface's reaction, contact count and largest penetration every m-th step in the ExplicitResult.
    Returns (u, v, a) [N,3] at the last step in `dtype`; with return_info also the system.ExplicitResult (with `dt`)."""
    what = "explicit_dynamics_solver"
    mask, rec = _check_explicit(what, coords, elements, F, fixed, rho, E, nu, steps, dt, safety, material, amplitude,
                                u0, v0, damping, record, energy_every)
    steps = int(steps)
    if contact is not None:
        contact = _sys.check_contact(what, contact, penalty, coords.shape[0], safety if dt is None else None)
    if int(contact_every) < 0 or (int(contact_every) > 0 and not contact):
        raise ValueError(f"{what}: contact_every must be >= 0 and needs contact surfaces, got {contact_every}")
    dev = _dev(device)
    cd = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    N = cd.shape[0]
    xd = _sys.ExplicitDynamics(cd, el, rho, E, nu, material, mask.to(dev), damping)
    try:
        if dt is None:
            dt = float(safety) * xd.stable_dt()[0]
            if not dt < float("inf"):
                dt = 1.0   # no element: nothing moves, any step will do
        dt = float(dt)
        if amplitude is None:
            amps = [1.0] * (steps + 1)
        elif torch.is_tensor(amplitude):
            amps = [float(x) for x in amplitude.to(dtype=F64).cpu()]
        else:
            amps = [float(amplitude(k * dt)) for k in range(steps + 1)]
        Fd = F.to(device=dev, dtype=F64).reshape(-1).contiguous()
        if contact:
            xd.set_contact(contact, penalty, dt=dt)
        xd.start(u0, v0, Fd, amps[0])
        rdofs = None
        if rec is not None:
            rdofs = (rec.to(dev).unsqueeze(-1) * 3 + torch.arange(3, device=dev)).reshape(-1)
        res = xd.run(steps, dt, Fd, amps, record=rdofs, energy_every=int(energy_every),
                     contact_every=int(contact_every))
        if res.status != _sys.XD_OK:
            print(f"Explicit solver: status {res.status} at step {res.stop_step} (dt = {dt:.6e}); the state after "
                  f"{steps} steps is returned")
        if rec is not None:   # rows 0 .. steps - 1 from the run, row `steps` the state reached
            last = (xd.u[rdofs], xd.v[rdofs], xd.a[rdofs])
            res.rec_u, res.rec_v, res.rec_a = (torch.cat((r, x.view(1, -1))).reshape(steps + 1, -1, 3)
                                               for r, x in zip((res.rec_u, res.rec_v, res.rec_a), last))
        out = torch.device(device)
        ret = tuple(x.view(N, 3).to(device=out, dtype=dtype).clone() for x in (xd.u, xd.v, xd.a))
    finally:
        xd.close()
    return ret + (res,) if return_info else ret


# ============================================================================ nonlinear statics
# Large-displacement statics of c3d4 meshes: Newton's method on the total-Lagrangian residual with the hyperelastic
# tangent of csrc/nonlinear.hip, the matrix refilled in place every iteration (system.NewtonStatics).
# The reference's own newton_raphson_solver (`solver/solver.py:978-1065`, secant form on a caller's K(u)) follows.
_LS_HALVINGS = 10
_LS_C1 = 1e-4
# elastoplastic solves: a trial taken for its smaller residual may raise the potential by no more than this share of
# (|internal energy| + |load work|), the rounding of the potential's two sums
_LS_POT_ROUND = 1e-13


def _check_nonlinear(what, coords, elements, F, fixed, material, load_steps, tol, atol, max_iter, linear_rtol,
                     linear_max_iter, u_init):
    """Every ValueError of nonlinear_static_solver -- before any device call. Returns the fixed node ids."""
    if not torch.is_tensor(coords) or coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"{what}: coords must be [N, 3], got {tuple(getattr(coords, 'shape', ()))}")
    N = coords.shape[0]
    if not torch.is_tensor(elements) or elements.dim() != 2 or elements.shape[1] != 4:
        raise ValueError(f"{what}: c3d4 connectivity [M, 4] expected, got {tuple(getattr(elements, 'shape', ()))}")
    if elements.numel() and (int(elements.min()) < 0 or _max_node(elements) > N):
        raise ValueError(f"{what}: the mesh references a node outside [0, {N})")
    if not torch.is_tensor(F) or tuple(F.shape) != (N, 3):
        raise ValueError(f"{what}: F must be [{N}, 3], got {tuple(getattr(F, 'shape', ()))}")
    if u_init is not None and (not torch.is_tensor(u_init) or tuple(u_init.shape) != (N, 3)):
        raise ValueError(f"{what}: u_init must be [{N}, 3]")
    if material not in C.MATERIALS:
        raise ValueError(f"{what}: unknown material {material!r} (supported: {', '.join(sorted(C.MATERIALS))})")
    if int(load_steps) < 1:
        raise ValueError(f"{what}: load_steps must be >= 1, got {load_steps}")
    if int(max_iter) < 1 or int(linear_max_iter) < 1:
        raise ValueError(f"{what}: max_iter and linear_max_iter must be >= 1")
    if not float(tol) >= 0.0 or not float(atol) >= 0.0 or not float(linear_rtol) > 0.0:
        raise ValueError(f"{what}: tol and atol must be >= 0 and linear_rtol > 0")
    return _fixed_ids(what, fixed, N)


def _newton_statics_loop(ns, Fd, u, load_steps, tol, atol, max_iter, linear_rtol, linear_max_iter, on_iteration=None,
                         load_factors=None, after_step=None, potential_round=None, first_tangent=None):
    """The load-stepped Newton iteration of nonlinear_static_solver on a system.NewtonStatics -> NonlinearResult (u
    left on the device). on_iteration(dict): per-iteration record hook of tools/bench_nonlinear.py.
    load_factors: the load factor of every step in order (default s / load_steps); the stop rule then scales with
    max |load factor|, so that a step to a zero load keeps a tolerance. after_step(s, u): called after every converged
    step (the elastoplastic solver commits its state there). potential_round: a trial accepted for its smaller residual
    must also keep the potential within potential_round (|internal energy| + |load work|) of the iterate's; a
    potential that is convex but only piecewise smooth can otherwise cycle under full Newton steps. first_tangent():
    fills the matrix in the first iteration of every step in place of ns.tangent()."""
    free = ns.mask == 0
    stop = max(float(tol) * float(torch.linalg.vector_norm(Fd[free])), float(atol))
    if load_factors is not None:
        load_factors = [float(f) for f in load_factors]
        stop = max(float(tol) * max(abs(f) for f in load_factors) * float(torch.linalg.vector_norm(Fd[free])),
                   float(atol))
    res = _sys.NonlinearResult(u, False, _sys.NL_OK, "", [], [], [], [])
    S = int(load_steps) if load_factors is None else len(load_factors)
    for s in range(1, S + 1):
        lf = s / S if load_factors is None else load_factors[s - 1]
        print(f"Load step {s}/{S}")
        norms, pits, alphas = [], [], []
        res.newton_iterations.append(0)
        res.residual_norms.append(norms)
        res.pcg_iterations.append(pits)
        res.step_lengths.append(alphas)
        done = False
        for k in range(1, int(max_iter) + 1):
            own = first_tangent is not None and k == 1
            r, en, rn, inv = ns.evaluate(u, lf, Fd, tangent=not own)
            if inv is not None:   # only a caller's u_init can be inverted here: trial points are rejected below
                en = float("inf")
            print(f"Iteration {k}, Residual Norm: {rn}")
            norms.append(rn)
            if inv is None and rn <= stop:
                print(f"Converged after {k} iterations.")
                done = True
                break
            pot = en - lf * ns.work
            if own:
                first_tangent()
            else:
                ns.tangent()
            w = ns.jacobi()
            delta, it, stt = ns.solve_increment(r, w, linear_rtol, linear_max_iter)
            slope = float(torch.dot(r, delta))
            if stt in (C.PCG_BREAKDOWN, C.PCG_ALPHA_NAN, C.PCG_BETA_NAN) or not slope > 0.0 or slope == float("inf"):
                delta = w * r   # preconditioned steepest descent: an indefinite tangent gave no descent direction
                slope = float(torch.dot(r, delta))
            pits.append(it)
            if not slope > 0.0 or slope == float("inf"):
                res.status = _sys.NL_LINEAR_SOLVE_FAILED
                res.message = f"No descent direction at load step {s}, iteration {k} (PCG status {stt})."
                print(res.message)
                res.u = u
                return res
            delta = delta.clone()
            alpha, accepted, evals = 1.0, False, 0
            for _ in range(_LS_HALVINGS + 1):
                ut = u + alpha * delta
                _, en_t, rn_t, inv_t = ns.evaluate(ut, lf, Fd, tangent=False)
                evals += 1
                pot_t = en_t - lf * ns.work
                lower = rn_t < rn and (potential_round is None or
                                       pot_t <= pot + potential_round * (abs(en_t) + abs(lf * ns.work)))
                if inv_t is None and (pot_t <= pot - _LS_C1 * alpha * slope or lower):
                    accepted = True
                    break
                alpha *= 0.5
            if on_iteration is not None:
                on_iteration({"step": s, "iteration": k, "residual": rn, "pcg_iterations": it, "pcg_status": stt,
                              "line_search_evaluations": evals, "alpha": alpha if accepted else 0.0})
            if not accepted:
                res.status = _sys.NL_LINE_SEARCH_FAILED
                res.message = (f"Line search failed at load step {s}, iteration {k}: no step length down to "
                               f"{alpha * 2.0:.3e} reduced the potential or the residual.")
                print(res.message)
                res.u = u
                return res
            u = ut
            alphas.append(alpha)
            res.newton_iterations[-1] = k
        if not done:
            print("Newton-Raphson did not converge within the maximum number of iterations.")
            res.status = _sys.NL_MAX_ITER
            res.message = f"Load step {s} did not converge within {int(max_iter)} iterations."
            res.u = u
            return res
        if after_step is not None:
            after_step(s, u)
    res.u = u
    res.converged = True
    return res


def nonlinear_static_solver(coords, elements, F, fixed, E, nu, material="svk", load_steps=1, tol=1e-8, atol=0.0,
                            max_iter=25, linear_rtol=1e-6, linear_max_iter=10000, u_init=None, device="cuda:0",
                            dtype=torch.float64, return_info=False):
    """Large-displacement statics of a c3d4 mesh: u [N, 3] with f_int(u) = F, the nodes `fixed` held at zero, for the
    hyperelastic materials of compute_c3d4_tangent_K_matrix ("svk", "neo_hookean"). The load is applied in `load_steps`
    equal steps; each step runs Newton's method from the previous step's u:
      1. r = load factor * F - f_int(u) on the free dofs; stop when ||r||_2 <= max(tol ||F_free||_2 (full load), atol);
      2. the tangent is assembled in place (system.NewtonStatics) and K_T delta = r solved by Jacobi-PCG to
         sqrt(r.z) <= linear_rtol sqrt(r0.z0); a breakdown of the PCG (an indefinite tangent) or r.delta <= 0 falls back
         to the preconditioned steepest descent delta = w o r; an iterate stopped by linear_max_iter is kept while it is
         a descent direction;
      3. backtracking alpha = 1, 1/2, ... (at most 10 halvings): a trial with an inverted element is rejected; one is
         accepted when the potential Pi = internal energy - load factor * F.u falls by 1e-4 alpha r.delta or the
         residual norm falls (near convergence the predicted decrease is below the rounding of Pi).
    Prints `Load step s/S`, `Iteration k, Residual Norm: x` and `Converged after k iterations.` in the style of the
    reference's newton_raphson_solver (`solver/solver.py:1012-1025`). Never raises on non-convergence: the last accepted
    u is returned and NonlinearResult.status is MAX_ITER or LINE_SEARCH_FAILED.
    Limits: homogeneous Dirichlet conditions on whole nodes, one GPU, the assembled operator, c3d4. Out of scope:
    non-zero prescribed displacements, arc-length control (limit points), other element types, a matrix-free tangent.
    Returns u in `dtype` on `device`; with return_info also the system.NonlinearResult."""
    what = "nonlinear_static_solver"
    ids = _check_nonlinear(what, coords, elements, F, fixed, material, load_steps, tol, atol, max_iter, linear_rtol,
                           linear_max_iter, u_init)
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    N = coords.shape[0]
    mask = torch.zeros((N, 3), dtype=torch.uint8, device=dev)
    mask[ids.to(dev)] = 1
    Fd = F.to(device=dev, dtype=F64).reshape(-1).contiguous()
    u = torch.zeros(3 * N, dtype=F64, device=dev) if u_init is None else \
        u_init.to(device=dev, dtype=F64).reshape(-1).clone()
    u[mask.view(-1) != 0] = 0.0
    ns = _sys.NewtonStatics(coords, el, E, nu, material, mask.view(-1), graph=cached_graph(el, N))
    try:
        res = _newton_statics_loop(ns, Fd, u, load_steps, tol, atol, max_iter, linear_rtol, linear_max_iter)
    finally:
        ns.close()
    res.u = res.u.view(N, 3).to(device=torch.device(device), dtype=dtype)
    return (res.u, res) if return_info else res.u


# ============================================================================ elastoplastic statics
# Small-strain von Mises plasticity with linear isotropic hardening on c3d4 meshes: the same Newton loop on
# system.PlasticStatics (the return-mapping kernel of csrc/plasticity.hip). No counterpart in the reference.
def _fixed_mask(what, fixed, N):
    """[N,3] bool of the dofs held at zero, from node ids or from a bool / uint8 [N,3] mask (per-dof supports)."""
    if torch.is_tensor(fixed) and fixed.dim() == 2 and fixed.dtype in (torch.bool, torch.uint8):
        if tuple(fixed.shape) != (N, 3):
            raise ValueError(f"{what}: a fixed-dof mask must be [{N}, 3], got {tuple(fixed.shape)}")
        return fixed.to("cpu") != 0
    mask = torch.zeros((N, 3), dtype=torch.bool)
    mask[_fixed_ids(what, fixed, N)] = True
    return mask


def elastoplastic_static_solver(coords, elements, F, fixed, E, nu, yield_stress, hardening, load_path=None,
                                load_steps=1, state=None, tol=1e-8, atol=0.0, max_iter=25, linear_rtol=1e-6,
                                linear_max_iter=10000, u_init=None, device="cuda:0", dtype=torch.float64,
                                return_info=False):
    """Elastoplastic statics of a c3d4 mesh: small-strain, rate-independent von Mises (J2) plasticity with linear
    isotropic hardening (yield stress `yield_stress` + `hardening` x accumulated plastic strain), associative flow,
    integrated by the radial return with its consistent tangent (csrc/plasticity.hip).
    load_path: load factors applied in order, e.g. [0.5, 1.0, 0.0] for load and unload (default k / load_steps,
    k = 1..load_steps). Each factor runs the Newton iteration of nonlinear_static_solver from the previous u on the
    incremental potential of the step, then commits the material state; `state` (a PlasticState) is the state before
    the first step (default virgin). fixed: node ids, or a bool / uint8 [N,3] mask of single dofs held at zero
    (rollers). The stop rule is nonlinear_static_solver's with the scale max |load factor| ||F_free||_2. In the line
    search a trial taken for its smaller residual must not raise the potential beyond its rounding. The first
    iteration of every step takes the elastic tangent: at the displacement just committed every yielded element has
    f_tr = 0 up to rounding, so the branch of its consistent tangent is noise there, and a plastic tangent on elements
    that unload overshoots; from the second iteration on the consistent tangent is used.
    Never raises on non-convergence: NonlinearResult.status is MAX_ITER / LINE_SEARCH_FAILED / LINEAR_SOLVE_FAILED,
    failed_step names the step, u is the last accepted iterate and state the committed state of the last converged
    step. hardening = 0 (perfect plasticity) is accepted but may stall at the limit load: the tangent is then only
    semi-definite there and the PCG has no positive definite matrix.
    Limits: c3d4 only, small strains, isotropic linear hardening, associative J2 flow, homogeneous Dirichlet data, one
    GPU, the assembled operator, one material for the whole mesh. Out of scope: other element types, finite-strain
    plasticity, kinematic or nonlinear hardening, arc-length control, a matrix-free tangent, multi-GPU, per-element
    yield data.
    Returns u in `dtype` on `device`; with return_info also the system.NonlinearResult with state (the final
    PlasticState), stress [M,6] at u (xx, yy, zz, xy, yz, xz) and plastic_fraction per converged step."""
    what = "elastoplastic_static_solver"
    if load_path is not None:
        load_path = [float(f) for f in load_path]
        if not load_path or not all(f == f and abs(f) != float("inf") for f in load_path):
            raise ValueError(f"{what}: load_path must hold at least one finite load factor")
    _check_nonlinear(what, coords, elements, F, [], "svk", load_steps, tol, atol, max_iter, linear_rtol,
                     linear_max_iter, u_init)
    N, M = coords.shape[0], elements.shape[0]
    mask = _fixed_mask(what, fixed, N)
    _sys.check_plastic_material(what, E, nu, yield_stress, hardening)
    _sys.check_plastic_state(what, state, M)
    if load_path is None:
        load_path = [k / int(load_steps) for k in range(1, int(load_steps) + 1)]
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    mask = mask.to(device=dev, dtype=torch.uint8).contiguous()
    Fd = F.to(device=dev, dtype=F64).reshape(-1).contiguous()
    u = torch.zeros(3 * N, dtype=F64, device=dev) if u_init is None else \
        u_init.to(device=dev, dtype=F64).reshape(-1).clone()
    u[mask.view(-1) != 0] = 0.0
    if state is not None:
        state = _sys.PlasticState(state.plastic_strain.to(device=dev, dtype=F64),
                                  state.equivalent_plastic_strain.to(device=dev, dtype=F64))
    ns = _sys.PlasticStatics(coords, el, E, nu, yield_stress, hardening, mask.view(-1), graph=cached_graph(el, N),
                             state=state)
    fractions = []

    def after_step(s, u_s):
        fractions.append(ns.plastic_fraction())
        ns.commit()

    try:
        res = _newton_statics_loop(ns, Fd, u, len(load_path), tol, atol, max_iter, linear_rtol, linear_max_iter,
                                   load_factors=load_path, after_step=after_step, potential_round=_LS_POT_ROUND,
                                   first_tangent=ns.elastic_tangent)
        out = torch.device(device)
        res.state = _sys.PlasticState(*(x.to(out) for x in (ns.state().plastic_strain,
                                                           ns.state().equivalent_plastic_strain)))
        res.stress = ns.stress(res.u).to(out) if M else torch.zeros((0, 6), dtype=F64, device=out)
        res.plastic_fraction = fractions
        if not res.converged:
            res.failed_step = len(res.newton_iterations)
    finally:
        ns.close()
    res.u = res.u.view(N, 3).to(device=torch.device(device), dtype=dtype)
    return (res.u, res) if return_info else res.u


# ============================================================================ topology optimisation
# Density-based (SIMP) compliance minimisation on c3d4 meshes with an optimality-criteria update: the design loop of
# system.TopOpt (csrc/topopt.hip and the scaled assembly). No counterpart in the reference.
def topology_optimization_solver(coords, elements, F, fixed, E, nu, volume_fraction, penal=3.0, s_min=1e-3,
                                 rho_min=1e-3, filter_passes=1, move=0.2, max_iter=100, change_tol=1e-2,
                                 linear_rtol=1e-8, linear_max_iter=10000, rho0=None, passive=None, callback=None,
                                 device="cuda:0"):
    """Minimise the compliance F.u of a c3d4 mesh over the element densities rho in [rho_min, 1] at the volume
    sum_e V_e rho_e = volume_fraction sum_e V_e. Per design iteration: rho_t = the node-average filter applied
    filter_passes times, s = s_min + (1 - s_min) rho_t^penal, K(s) = sum_e s_e K_e(E, nu) refilled in place, K u = F by
    Jacobi-PCG from the previous u to sqrt(r.z) <= linear_rtol sqrt(F.w F), dc = filter^T (-penal (1 - s_min)
    rho_t^(penal-1) E ce), and the optimality-criteria update rho_e <- clamp(rho_e sqrt(-dc_e / (V_e l))) within the
    move limit, its multiplier l found by 60 bisection steps on the device. Starts from rho = volume_fraction (or
    rho0 [M]); stops at max |rho_new - rho| <= change_tol or after max_iter iterations (status MAX_ITER).
    fixed: node ids, or a bool / uint8 [N,3] mask of single dofs held at zero. passive: int8 [M], 0 free, 1 solid
    (pinned to 1), -1 void (pinned to rho_min). callback(iteration, record): called after every design iteration with
    system.TopOpt.step's record. A linear solve that does not converge ends the run with the last accepted density
    and status LINEAR_SOLVE_FAILED (no exception).
    Limits: c3d4, one load case, compliance under one volume constraint, the node-average filter, Jacobi-PCG on the
    assembled operator, one GPU. Not built: radius or Helmholtz filters, projection, MMA, stress or several
    constraints, other element types, per-element nu, the scale in the matrix-free operator, the two-level
    preconditioner inside the loop, multi-GPU.
    Returns a system.TopOptResult (tensors on `device`)."""
    what = "topology_optimization_solver"
    _sys.check_topopt_parameters(what, volume_fraction, penal, s_min, rho_min, move, filter_passes)
    if not torch.is_tensor(coords) or coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"{what}: coords must be [N, 3], got {tuple(getattr(coords, 'shape', ()))}")
    N = coords.shape[0]
    if not torch.is_tensor(elements) or elements.dim() != 2 or elements.shape[1] != 4:
        raise ValueError(f"{what}: c3d4 connectivity [M, 4] expected, got {tuple(getattr(elements, 'shape', ()))}")
    M = elements.shape[0]
    if elements.numel() and (int(elements.min()) < 0 or _max_node(elements) > N):
        raise ValueError(f"{what}: the mesh references a node outside [0, {N})")
    if not torch.is_tensor(F) or tuple(F.shape) != (N, 3):
        raise ValueError(f"{what}: F must be [{N}, 3], got {tuple(getattr(F, 'shape', ()))}")
    if int(max_iter) < 1 or int(linear_max_iter) < 1:
        raise ValueError(f"{what}: max_iter and linear_max_iter must be >= 1")
    if not float(change_tol) >= 0.0 or not float(linear_rtol) > 0.0:
        raise ValueError(f"{what}: change_tol must be >= 0 and linear_rtol > 0")
    if rho0 is not None and (not torch.is_tensor(rho0) or rho0.numel() != M):
        raise ValueError(f"{what}: rho0 must hold {M} values")
    if passive is not None and (not torch.is_tensor(passive) or passive.numel() != M):
        raise ValueError(f"{what}: passive must hold {M} values")
    mask = _fixed_mask(what, fixed, N)
    if not bool((F.detach().to("cpu", F64)[~mask] != 0).any()):
        raise ValueError(f"{what}: the load is zero on the free dofs")
    dev = _dev(device)
    coords = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    rho = (torch.full((M,), float(volume_fraction), dtype=F64, device=dev) if rho0 is None
           else rho0.to(device=dev, dtype=F64).reshape(-1).clone())
    to = _sys.TopOpt(coords, el, F, mask.to(device=dev, dtype=torch.uint8).view(-1), E, nu, volume_fraction, penal,
                     s_min, rho_min, filter_passes, move, passive=passive, graph=cached_graph(el, N))
    res = _sys.TopOptResult(rho, None, None, None, False, _sys.TOPOPT_MAX_ITER, "", [], [], [], [], [])
    try:
        for k in range(1, int(max_iter) + 1):
            rec = to.step(rho, linear_rtol, linear_max_iter)
            res.filtered_density, res.modulus_scale, res.u = rec["rho_t"].clone(), rec["s"].clone(), \
                rec["u"].view(N, 3).clone()
            res.pcg_iterations.append(rec["pcg_iterations"])
            if rec["rho_new"] is None:
                res.status = _sys.TOPOPT_LINEAR_SOLVE_FAILED
                res.message = (f"The linear solve of design iteration {k} did not converge within "
                               f"{int(linear_max_iter)} iterations (PCG status {rec['status']}).")
                break
            res.compliance.append(rec["compliance"])
            res.load_work.append(rec["load_work"])
            res.volume_fraction.append(rec["volume_fraction"])
            res.change.append(rec["change"])
            rho = rec["rho_new"].clone()
            res.density = rho
            if callback is not None:
                callback(k, rec)
            if rec["change"] <= float(change_tol):
                res.converged, res.status = True, _sys.TOPOPT_OK
                break
        else:
            res.message = f"The design did not settle within {int(max_iter)} iterations."
    finally:
        to.close()
    out = torch.device(device)
    res.density = res.density.to(out)
    for name in ("filtered_density", "modulus_scale", "u"):
        setattr(res, name, getattr(res, name).to(out))
    return res


def newton_raphson_solver(K_func, elements, F_ext, u_init=None, tol=1e-8, max_iter=50, device="cuda:0",
                          dtype=torch.float32):
    """The reference's Newton-Raphson on K(u) u = F_ext (`solver/solver.py:978-1065`), same signature and semantics:
    K_func(u [N, 3]) -> element matrices [M, d, d] on the device; F_int = K(u) u (the secant form); R = F_ext - F_int;
    `Iteration k, Residual Norm: ||R||` is printed and the loop stops at ||R|| < tol with `Converged after k
    iterations.`; otherwise delta from plain CG on K(u) delta = R from zero, stopped at sqrt(r.r) < tol or after 100
    iterations (then `CG did not converge within the maximum number of iterations.` and the iterate is used), and
    u += delta. No boundary conditions: the caller's K_func carries them. On the device K(u) is assembled in place on a
    graph built once and the inner CG is the device PCG with unit weights (the same recurrences and stop). Arithmetic
    is fp64; `dtype` is that of the u handed to K_func and returned."""
    dev = _dev(device)
    N = F_ext.shape[0]
    el = elements.to(device=dev, dtype=LONG).contiguous()
    Fd = F_ext.to(device=dev, dtype=F64).reshape(-1).contiguous()
    dpn = F_ext.shape[1] if F_ext.dim() == 2 else 3
    u = torch.zeros(N * dpn, dtype=F64, device=dev) if u_init is None else \
        u_init.to(device=dev, dtype=F64).reshape(-1).clone()
    A = _sys.SellMatrix(cached_graph(el, N), dpn)
    ones = torch.ones(N * dpn, dtype=F64, device=dev)
    for iteration in range(int(max_iter)):
        K = K_func(u.view(N, dpn).to(dtype))
        if _ke_dpn("newton_raphson_solver", K, el) != dpn:
            raise ValueError(f"newton_raphson_solver: K_func returned {tuple(K.shape)} for {dpn} dofs per node")
        A.reset().add_element_matrices(K.to(device=dev, dtype=F64), el)
        R = Fd - A.matvec(u)
        norm_R = float(torch.linalg.vector_norm(R))
        print(f"Iteration {iteration + 1}, Residual Norm: {norm_R}")
        if norm_R < tol:
            print(f"Converged after {iteration + 1} iterations.")
            break
        res = A.pcg(R, None, w=ones, mode=C.MODE_PCG, tol=tol, max_iter=100)
        if res.status != C.PCG_CONVERGED:
            print("CG did not converge within the maximum number of iterations.")
        u = u + res.x
    else:
        print("Newton-Raphson did not converge within the maximum number of iterations.")
    return u.view(N, dpn).to(device=torch.device(device), dtype=dtype)


# every public function runs in the scope of the device its `device` argument names (_capi.on_device)
C.scope_module(globals())
