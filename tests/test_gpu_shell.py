"""GPU tier of the shell elements (csrc/shell.hip, shell.py, system.SixDofMap, the s3 / s4 path of
static_structure_solver) against the fixtures recorded from the reference (tests/golden/shell_cells.npz,
shell_static.npz) and, where no fixture exists, against the restatement tests/shell_ref.py that
tests/test_shell_cpu.py pins to those fixtures."""
import re

import pytest
import torch

import shell_ref as SR
from conftest import load_golden, rel

pytestmark = pytest.mark.gpu
F64 = torch.float64
TOL = 1e-12    # the project's element / operator tolerance against the reference
TOL_U = 1e-10  # the project's solver tolerance on u, relative to max|u|


def _mods():
    from fem355 import element, shell, solver, system
    return element, shell, solver, system


@pytest.fixture(scope="module")
def cells():
    return load_golden("shell_cells")


@pytest.fixture(scope="module")
def static():
    return load_golden("shell_static")


def _material(g):
    return {"E": float(g["E"]), "nu": float(g["nu"]), "membrane": g["membrane"], "bending": g["bending"]}


def rel_each(a, b):
    """Largest per-element error relative to that element's largest reference entry."""
    a, b = a.detach().cpu().to(F64), b.detach().cpu().to(F64)
    M = b.shape[0]
    return float(((a - b).abs().reshape(M, -1).max(1).values / b.abs().reshape(M, -1).max(1).values).max())


# ----------------------------------------------------------------------------- element parity
def test_s3_elements_vs_golden(gpu, cells):
    _, sh, _, _ = _mods()
    c, s3, mem, ben = cells["coords"], cells["s3"], cells["membrane"], cells["bending"]
    kw = dict(device=gpu, dtype=F64)
    K = sh.compute_s3_K_matrix(c, s3, mem, ben, **kw)
    assert tuple(K.shape) == (8, 18, 18) and rel_each(K, cells["s3_K"]) < TOL
    unit = sh.compute_s3_local_unitvector(c, s3, device=gpu)
    assert rel(unit, cells["s3_unit"]) < TOL
    assert rel(sh.compute_s3_global_to_local_coordinates(c, s3, unit, **kw), cells["s3_local"]) < TOL
    assert rel_each(sh.compute_s3_jacobian(c, s3, **kw), cells["s3_J"]) < TOL
    assert rel_each(sh.compute_s3_shape_gradient(c, s3, **kw), cells["s3_grads"]) < TOL
    assert rel_each(sh.compute_s3_B_matrix(c, s3, **kw), cells["s3_B"]) < TOL
    assert rel(sh.compute_kirchoff_D_matrix(mem, ben, **kw), cells["D"]) < TOL
    _structure(K.cpu(), 3)


def _structure(K, npe):
    """Exact zeros in the rows and columns of w and thz and between the membrane and bending blocks; symmetric."""
    dof = torch.arange(6 * npe) % 6
    dead = (dof == 2) | (dof == 5)
    assert bool((K[:, dead] == 0).all()) and bool((K[:, :, dead] == 0).all())
    mem, ben = dof < 2, (dof == 3) | (dof == 4)
    assert bool((K[:, mem][:, :, ben] == 0).all()) and bool((K[:, ben][:, :, mem] == 0).all())
    assert bool((K[:, mem][:, :, mem] != 0).any()) and bool((K[:, ben][:, :, ben] != 0).any())
    assert torch.equal(K, K.transpose(1, 2))


def test_s4_elements_vs_golden(gpu, cells):
    _, sh, _, _ = _mods()
    c, s4, mem, ben = cells["coords"], cells["s4"], cells["membrane"], cells["bending"]
    kw = dict(device=gpu, dtype=F64)
    K = sh.compute_s4_K_matrix(c, s4, mem, ben, **kw)
    assert tuple(K.shape) == (8, 24, 24) and rel_each(K, cells["s4_K"]) < TOL
    Kp = sh.compute_s4_K_matrix(c, s4, mem, ben, single=False, **kw)
    assert tuple(Kp.shape) == (8, 24, 24, 4) and rel_each(Kp, cells["s4_K_points"]) < TOL
    assert rel_each(Kp.sum(-1), K) < 1e-14
    unit = sh.compute_s4_local_unitvector(c, s4, device=gpu)
    assert rel(unit, cells["s4_unit"]) < TOL
    assert rel(sh.compute_s4_global_to_local_coordinates(c, s4, unit, **kw), cells["s4_local"]) < TOL
    for p in range(4):
        xi, eta = (float(v) for v in cells["s4_points"][p])
        assert rel_each(sh.compute_s4_jacobian(c, s4, xi, eta, **kw), cells["s4_J"][..., p]) < TOL
        assert rel_each(sh.compute_s4_shape_gradient(c, s4, xi, eta, **kw), cells["s4_grads"][..., p]) < TOL
        assert rel_each(sh.compute_s4_B_matrix_single(c, s4, xi, eta, **kw), cells["s4_B"][..., p]) < TOL
    B = sh.compute_s4_B_matrix(c, s4, **kw)
    assert tuple(B.shape) == (8, 6, 24) and rel_each(B, cells["s4_B_sum"]) < TOL
    assert tuple(sh.compute_s4_B_matrix(c, s4, single=False, **kw).shape) == (8, 6, 24, 4)
    _structure(K.cpu(), 4)
    for p in range(4):
        _structure(Kp[..., p].cpu(), 4)


def test_s4_gauss_point_is_the_float32_rounded_one(gpu, cells):
    """The reference's abscissa is 1/sqrt(3) rounded to float32; with the double value K differs at 1e-8."""
    _, sh, _, _ = _mods()
    c, s4, mem, ben = cells["coords"], cells["s4"], cells["membrane"], cells["bending"]
    K = sh.compute_s4_K_matrix(c, s4, mem, ben, device=gpu, dtype=F64)
    assert rel_each(K, SR.s4_K(c, s4, mem, ben, g=SR.G32)) < TOL
    assert rel(K, SR.s4_K(c, s4, mem, ben, g=SR.G64)) > 1e-10


def test_s4_negative_detj_point_keeps_its_sign(gpu, cells):
    """An inverted region stays valid: the dart's point with detJ < 0 contributes a negated term, as recorded."""
    _, sh, _, _ = _mods()
    c, s4, mem, ben = cells["coords"], cells["s4"], cells["membrane"], cells["bending"]
    dets = torch.det(cells["s4_J"].permute(0, 3, 1, 2))
    e, p = (int(v) for v in torch.nonzero(dets < 0)[0])
    Kp = sh.compute_s4_K_matrix(c, s4, mem, ben, single=False, device=gpu, dtype=F64).cpu()
    want = cells["s4_K_points"][e, :, :, p]
    assert float((Kp[e, :, :, p] - want).abs().max() / want.abs().max()) < TOL
    d = torch.diagonal(Kp[e, :, :, p])
    assert bool((d <= 0).all()) and bool((d < 0).any())
    other = torch.diagonal(Kp[e, :, :, (p + 1) % 4])
    assert bool((other >= 0).all()) and bool((other > 0).any())


# ----------------------------------------------------------------------------- degenerate elements, wave and tail
def _tiled(cells, key, reps):
    conn = cells[key].repeat(reps, 1)
    return cells["coords"], conn


def _with_bad_last(cells, key, pts):
    """64 good elements and one made of the new points `pts`, last."""
    c, conn = _tiled(cells, key, 8)
    n0 = c.shape[0]
    c = torch.cat([c, torch.tensor(pts, dtype=F64)], 0)
    bad = torch.arange(n0, n0 + len(pts)).view(1, -1)
    return c, torch.cat([conn, bad], 0)


P0 = [0.3, -0.2, 0.7]
D1 = [0.31, 0.17, -0.23]   # a direction off every axis, so the collinear cases leave rounding residue


def _along(t):
    return [P0[k] + t * D1[k] for k in range(3)]


DEGENERATE = {
    "s3_zero_edge": ("s3", [P0, P0, [0.9, 0.1, 0.2]]),
    "s3_collinear": ("s3", [P0, _along(1.0), _along(2.5)]),
    "s4_zero_edge": ("s4", [P0, P0, [0.9, 0.1, 0.2], [0.2, 0.8, 0.1]]),
    "s4_node3_on_edge01": ("s4", [P0, _along(1.0), [0.9, 0.1, 0.2], _along(0.4)]),
}


@pytest.mark.parametrize("case", sorted(DEGENERATE))
def test_degenerate_element_last_of_65_is_named(gpu, cells, case):
    _, sh, _, _ = _mods()
    key, pts = DEGENERATE[case]
    c, conn = _with_bad_last(cells, key, pts)
    assert conn.shape[0] == 65
    fn = sh.compute_s3_K_matrix if key == "s3" else sh.compute_s4_K_matrix
    with pytest.raises(ValueError, match=r"element 64\b"):
        fn(c, conn, cells["membrane"], cells["bending"], device=gpu, dtype=F64)
    K = fn(c, conn[:64], cells["membrane"], cells["bending"], device=gpu, dtype=F64)   # the others are fine
    assert rel_each(K[:8], cells[key + "_K"]) < TOL


@pytest.mark.parametrize("key", ["s3", "s4"])
def test_element_counts_around_the_wave(gpu, cells, key):
    """M = 1, 63, 64, 65: identical bits to slicing a larger batch, in the local and the global frame."""
    _, sh, _, _ = _mods()
    c, conn = _tiled(cells, key, 17)   # 136 elements
    mem, ben = cells["membrane"], cells["bending"]
    fn = sh.compute_s3_K_matrix if key == "s3" else sh.compute_s4_K_matrix
    K = fn(c, conn, mem, ben, device=gpu, dtype=F64)
    Kg, unit = sh.shell_global_K(c, conn, mem, ben, device=gpu)
    assert rel_each(K[:8], cells[key + "_K"]) < TOL and torch.equal(K[:8], K[128:136])
    for M in (1, 63, 64, 65):
        assert torch.equal(fn(c, conn[:M], mem, ben, device=gpu, dtype=F64), K[:M])
        kg, un = sh.shell_global_K(c, conn[:M], mem, ben, device=gpu)
        assert torch.equal(kg, Kg[:M]) and torch.equal(un, unit[:M])
    # the global-frame matrices are T^T K T in the assembly's block order
    order = SR.block_order(conn.shape[1])
    want = SR.global_K(cells[key + "_K"], cells[key + "_unit"])[:, order][:, :, order]
    assert rel_each(Kg[:8], want) < TOL
    assert torch.equal(Kg[:8].cpu(), Kg[:8].cpu().transpose(1, 2))


# ----------------------------------------------------------------------------- operator
@pytest.mark.parametrize("key", ["s3", "s4"])
def test_shell_nodal_forces_vs_golden(gpu, cells, key):
    _, sh, _, _ = _mods()
    conn = cells[key]
    kw = dict(device=gpu, dtype=F64)
    y = sh.compute_shell_nodal_forces(cells[key + "_K"], conn, cells["u"], cells[key + "_unit"], **kw)
    assert tuple(y.shape) == tuple(cells["u"].shape) and rel(y, cells[key + "_forces"]) < TOL
    y2 = sh.compute_shell_nodal_forces(cells[key + "_K"], conn, cells["u"], cells[key + "_unit"], **kw)
    assert torch.equal(y, y2)


def test_shell_nodal_forces_fan_of_12(gpu, cells):
    """One node shared by 12 triangles (a shallow cone), against the restatement; two calls give the same bits."""
    _, sh, _, _ = _mods()
    ang = torch.arange(12, dtype=F64) * (2 * torch.pi / 12)
    rim = torch.stack([torch.cos(ang), torch.sin(ang), 0.2 + 0.05 * torch.cos(3 * ang)], 1)
    c = torch.cat([torch.zeros(1, 3, dtype=F64), rim], 0)
    fan = torch.tensor([[0, 1 + k, 1 + (k + 1) % 12] for k in range(12)])
    mem, ben = cells["membrane"], cells["bending"]
    u = torch.randn(13, 6, dtype=F64, generator=torch.Generator().manual_seed(12))
    K = sh.compute_s3_K_matrix(c, fan, mem, ben, device=gpu, dtype=F64)
    unit = sh.compute_s3_local_unitvector(c, fan, device=gpu)
    assert rel_each(K, SR.s3_K(c, fan, mem, ben)) < TOL and rel(unit, SR.frame(c, fan)) < TOL
    y = sh.compute_shell_nodal_forces(K, fan, u, unit, device=gpu, dtype=F64)
    assert rel(y, SR.nodal_forces(SR.s3_K(c, fan, mem, ben), fan, u, SR.frame(c, fan))) < TOL
    assert torch.equal(y, sh.compute_shell_nodal_forces(K, fan, u, unit, device=gpu, dtype=F64))


def _assemble(gpu, g, system, sh, el):
    dev = torch.device(gpu)
    c = g["coords"].to(dev)
    mat = _material(g)
    shells = [g[k].to(dev) for k in ("s3", "s4")]
    N = c.shape[0]
    dm = system.SixDofMap(N, shells)
    solids = [(el.compute_c3d4_K_matrix(c, g["c3d4"], mat["E"], mat["nu"], device=gpu, dtype=F64), g["c3d4"].to(dev)),
              (el.compute_c3d8_K_matrix(c, g["c3d8"], mat["E"], mat["nu"], device=gpu, dtype=F64), g["c3d8"].to(dev)),
              (el.compute_c3d6_K_matrix(c, g["c3d6"], mat["E"], mat["nu"], device=gpu, dtype=F64), g["c3d6"].to(dev))]
    conns = [e for _, e in solids] + [dm.shell_connectivity(s) for s in shells]
    graph = system.build_graph(system.pad_connectivity(conns, 8), dm.n_blocks)
    A = system.SellMatrix(graph, 3)
    for K, e in solids:
        A.add_element_matrices(K, e, inc=system.incidence(e, dm.n_blocks))
    for s in shells:
        A.add_shell_matrices(sh.shell_global_K(c, s, mat["membrane"], mat["bending"], device=gpu)[0], s, dm)
    return A, dm, solids, shells, c, mat


def test_assembled_6dof_matrix_equals_ebe_operators(gpu, static):
    """A p on the block numbering == shell EBE + solid EBE == the recorded product, fin free: covers shell-only nodes
    (the fin's outer nodes), solid-only nodes (no rotation rows) and nodes with both."""
    el, sh, _, system = _mods()
    A, dm, solids, shells, c, mat = _assemble(gpu, static, system, sh, el)
    N = c.shape[0]
    p = static["p"].to(c.device)
    y = dm.from_blocks(A.matvec(dm.to_blocks(p).view(-1)))
    ebe = torch.zeros((N, 6), dtype=F64, device=c.device)
    for K, e in solids:
        ebe[:, :3] += el.compute_nodal_forces(K, e, p[:, :3], device=gpu, dtype=F64)
    for s in shells:
        fn = sh.compute_s3_K_matrix if s.shape[1] == 3 else sh.compute_s4_K_matrix
        unitfn = sh.compute_s3_local_unitvector if s.shape[1] == 3 else sh.compute_s4_local_unitvector
        ebe += sh.compute_shell_nodal_forces(fn(c, s, mat["membrane"], mat["bending"], device=gpu, dtype=F64), s, p,
                                             unitfn(c, s, device=gpu), device=gpu, dtype=F64)
    assert rel(y, ebe) < TOL and rel(ebe, static["Kp"]) < TOL and rel(y, static["Kp"]) < TOL
    assert bool((y[~dm.has_shell, 3:] == 0).all()) and bool((static["Kp"][~dm.has_shell.cpu(), 3:] == 0).all())
    # rows with a zero diagonal (the planar fin has no stiffness along z) get Jacobi weight 0, not inf
    w = A.jacobi()
    assert bool(torch.isfinite(w).all()) and bool((w == 0).any())


def test_rotation_dof_without_a_shell(gpu, static, capsys):
    """It has no rows: it keeps its u_init value, and a load on it is refused."""
    _, _, solver, system = _mods()
    g = static
    N = g["coords"].shape[0]
    dm = system.SixDofMap(N, [g["s3"], g["s4"]])
    lone = int(torch.nonzero(~dm.has_shell)[0])
    assert lone not in g["fixed"].tolist()
    u0 = torch.zeros((N, 6), dtype=F64)
    u0[lone, 3:] = torch.tensor([0.125, -0.5, 2.0], dtype=F64)
    kw = dict(c3d4=g["c3d4"], c3d6=g["c3d6"], c3d8=g["c3d8"], s3=g["s3"], s4=g["s4"], material=_material(g),
              tol=float(g["tol"]), device=gpu)
    u = solver.static_structure_solver(g["coords"], g["force"], g["fixed"], u_init=u0, max_iter=3, **kw)
    assert "did not converge" in capsys.readouterr().out
    assert torch.equal(u[lone, 3:].cpu(), u0[lone, 3:])
    assert bool((u[g["fixed"]] == 0).all())
    load = g["force"].clone()
    load[lone, 4] = 1.0
    with pytest.raises(ValueError, match="rotational loads"):
        solver.static_structure_solver(g["coords"], load, g["fixed"], max_iter=3, **kw)


# ----------------------------------------------------------------------------- driver
@pytest.fixture(scope="module")
def cpu_operator(static):
    blocks = {k: static[k] for k in ("c3d4", "c3d6", "c3d8", "s3", "s4")}
    return SR.operator(static["coords"].shape[0], *SR.families(static["coords"], blocks, _material(static)))


def _normalised(text):
    text = re.sub(r"\d+ iterations", "N iterations", text)
    return re.sub(r"Residual norm: \S+", "Residual norm: R", text)


def test_static_structure_solver_with_shells_vs_golden(gpu, static, cpu_operator, capsys):
    _, _, solver, _ = _mods()
    g = static
    tol = float(g["tol"])
    capsys.readouterr()
    u, res = solver.static_structure_solver(g["coords"], g["force"], g["fixed"], c3d4=g["c3d4"], c3d6=g["c3d6"],
                                            c3d8=g["c3d8"], s3=g["s3"], s4=g["s4"], material=_material(g), tol=tol,
                                            max_iter=20000, device=gpu, return_info=True)
    out = capsys.readouterr().out
    r = g["force"] - cpu_operator(u.cpu())
    r[g["fixed"]] = 0.0
    err, resid = rel(u, g["u"]), float(torch.linalg.norm(r))
    print(f"shell static: {res.iterations} it (reference {int(g['n_iter'])}), rel err {err:.3e}, "
          f"masked true residual {resid:.3e}")
    assert tuple(u.shape) == tuple(g["u"].shape)
    assert abs(res.iterations - int(g["n_iter"])) <= 2
    assert err < TOL_U
    assert resid <= tol
    assert _normalised(out) == _normalised(str(g["stdout"]))


@pytest.mark.parametrize("which", ["s3", "s4"])
def test_static_structure_solver_one_shell_family(gpu, static, which, capsys):
    """Solids with only the s3 skin, and with only the s4 skin and fin, against the restatement's driver."""
    _, _, solver, _ = _mods()
    g = static
    N = g["coords"].shape[0]
    # a node on one element of the family (or two nearly coplanar ones) has no stiffness about the normal: the
    # rotation block is singular there and the reference's CG count then hangs on rounding. Such nodes are held,
    # as are the recorded fixed nodes; the rest of the skin keeps its moments
    count = torch.bincount(g[which].reshape(-1), minlength=N)
    fixed = torch.unique(torch.cat([g["fixed"], torch.nonzero((count > 0) & (count < 3)).view(-1)]))
    force = g["force"].clone()
    force[count == 0, 3:] = 0.0
    held = torch.zeros(N, dtype=torch.bool)
    held[fixed] = True
    assert bool((force[~held, 3:] != 0).any())
    blocks = {k: g[k] for k in ("c3d4", "c3d6", "c3d8", which)}
    tol = float(g["tol"])
    u_ref, it_ref, status, msg = SR.static_structure(g["coords"], force, fixed, blocks, _material(g), tol=tol,
                                                     max_iter=20000)
    assert status == "converged"
    shells = {which: g[which]}
    u, res = solver.static_structure_solver(g["coords"], force, fixed, c3d4=g["c3d4"], c3d6=g["c3d6"], c3d8=g["c3d8"],
                                            material=_material(g), tol=tol, max_iter=20000, device=gpu,
                                            return_info=True, **shells)
    out = capsys.readouterr().out
    print(f"{which} only: {res.iterations} it (restatement {it_ref}), rel err {rel(u, u_ref):.3e}")
    assert abs(res.iterations - it_ref) <= 2 and rel(u, u_ref) < TOL_U
    assert _normalised(out) == _normalised("Preprocessing done.\n\n " + msg + "\n")


def test_static_structure_solver_without_shells_is_unchanged(gpu, capsys):
    _, _, solver, _ = _mods()
    m = load_golden("mixed_static")
    mat = {"E": 113.8e9, "nu": 0.342}
    kw = dict(c3d4=m["c3d4"], c3d6=m["c3d6"], c3d8=m["c3d8"], material=mat, tol=1e-6, max_iter=3000, device=gpu)
    u, res = solver.static_structure_solver(m["coords"], m["force"], m["fixed"], return_info=True, **kw)
    assert abs(res.iterations - int(m["n_iter"])) <= 2 and rel(u, m["u"]) < TOL_U
    load = m["force"].clone()
    load[5, 4] = 1.0
    with pytest.raises(ValueError, match=r"rotational loads need shell elements \(out of scope\)"):
        solver.static_structure_solver(m["coords"], load, m["fixed"], **kw)
    capsys.readouterr()


# ----------------------------------------------------------------------------- stress
def test_shell_stress_vs_golden(gpu, cells):
    _, sh, _, _ = _mods()
    c, u, mem, ben = cells["coords"], cells["u"], cells["membrane"], cells["bending"]
    kw = dict(device=gpu, dtype=F64)
    n3 = sh.compute_s3_shell_stress(c, cells["s3"], mem, ben, u, **kw)
    n4 = sh.compute_s4_shell_stress(c, cells["s4"], mem, ben, u, **kw)
    assert tuple(n3.shape) == (8, 6) and rel_each(n3, cells["s3_nmq"]) < TOL
    assert tuple(n4.shape) == (8, 6) and rel_each(n4, cells["s4_nmq"]) < TOL
    t = float(mem[2])
    pp = sh.compute_shell_postprocess_values(cells["s4_nmq"], t, z=t / 2, **kw)   # from the recorded resultants
    for k, v in pp.items():
        assert v.device.type == "cuda" and rel(v, cells[f"s4_post_zt_{k}"]) < TOL, k
