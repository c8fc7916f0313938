"""CPU tier of the shell elements: the restatement tests/shell_ref.py agrees with the fixtures recorded from the
reference (tools/gen_golden_shell.py), the 6-dof block numbering of system.SixDofMap round-trips and maps element
matrices onto the dense 6N assembly, and `solver` exposes the reference's shell names under both loading routes."""
import os
import re
import subprocess
import sys

import pytest
import torch

import fem355  # noqa: F401
import shell_ref as SR
from conftest import ROOT, load_golden, rel

TOL = 1e-12   # the project's float tolerance against the reference, relative to the array's largest entry

# the public names of the reference's solver/shell.py
SHELL_NAMES = [
    "compute_kirchoff_D_matrix", "compute_global_to_local_displacement", "compute_shell_nodal_forces",
    "compute_shell_postprocess_values", "compute_s3_normal", "identify_s3_shared_edges",
    "compute_triangle_surface_faces_with_third_node", "compute_s3_local_unitvector",
    "compute_s3_global_to_local_coordinates", "compute_s3_jacobian", "compute_s3_shape_gradient",
    "compute_s3_B_matrix", "compute_s3_K_matrix", "compute_s3_shell_stress", "compute_s4_normal",
    "identify_s4_shared_edges", "compute_square_surface_faces_with_fourth_node", "compute_s4_local_unitvector",
    "compute_s4_global_to_local_coordinates", "s4_integration_points", "compute_s4_jacobian",
    "compute_s4_shape_gradient", "compute_s4_B_matrix_single", "compute_s4_B_matrix", "compute_s4_K_matrix",
    "compute_s4_shell_stress", "shell_extrude",
]


@pytest.fixture(scope="module")
def cells():
    return load_golden("shell_cells")


@pytest.fixture(scope="module")
def static():
    return load_golden("shell_static")


def test_fixture_integers_and_sizes(cells, static):
    assert cells["s3"].dtype == torch.int64 and tuple(cells["s3"].shape) == (8, 3)
    assert cells["s4"].dtype == torch.int64 and tuple(cells["s4"].shape) == (8, 4)
    for name in ("shell_cells", "shell_static"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 2 * 2 ** 20
    N = static["coords"].shape[0]
    shells = torch.cat([static["s3"].reshape(-1), static["s4"].reshape(-1)])
    solids = torch.cat([static[k].reshape(-1) for k in ("c3d4", "c3d6", "c3d8")])
    on_shell = torch.zeros(N, dtype=torch.bool)
    on_shell[shells] = True
    on_solid = torch.zeros(N, dtype=torch.bool)
    on_solid[solids] = True
    assert torch.equal(torch.nonzero(on_shell & ~on_solid).view(-1), static["fin_outer"])   # the fin's outer nodes only
    assert bool((~on_shell & on_solid).any())                                               # interior: solids only
    assert torch.equal(static["fixed"], torch.cat([static["fixed_box"], static["fin_outer"]]))


def test_restatement_s3_cells(cells):
    c, s3, mem, ben = cells["coords"], cells["s3"], cells["membrane"], cells["bending"]
    unit, loc = SR.geometry(c, s3)
    assert rel(unit, cells["s3_unit"]) < TOL and rel(loc, cells["s3_local"]) < TOL
    assert rel(SR.jacobian(loc), cells["s3_J"]) < TOL
    g = SR.gradients(loc)
    assert rel(g, cells["s3_grads"]) < TOL and rel(SR.B_matrix(g), cells["s3_B"]) < TOL
    K = SR.s3_K(c, s3, mem, ben)
    assert rel(K, cells["s3_K"]) < TOL
    assert rel(SR.D_matrix(mem, ben), cells["D"]) < TOL
    assert rel(SR.nodal_forces(K, s3, cells["u"], unit), cells["s3_forces"]) < TOL
    assert rel(SR.stress(c, s3, mem, ben, cells["u"]), cells["s3_nmq"]) < TOL


def test_restatement_s4_cells(cells):
    c, s4, mem, ben = cells["coords"], cells["s4"], cells["membrane"], cells["bending"]
    unit, loc = SR.geometry(c, s4)
    assert rel(unit, cells["s4_unit"]) < TOL and rel(loc, cells["s4_local"]) < TOL
    # the fixture's points are the float32-rounded abscissa widened to double
    assert torch.equal(cells["s4_points"], torch.tensor(SR.SIGNS, dtype=torch.float64) * SR.G32)
    for p, f in enumerate(SR.k_factors()):
        assert rel(SR.jacobian(loc, f), cells["s4_J"][..., p]) < TOL
        g = SR.gradients(loc, f)
        assert rel(g, cells["s4_grads"][..., p]) < TOL and rel(SR.B_matrix(g), cells["s4_B"][..., p]) < TOL
    Kp = SR.s4_K_points(c, s4, mem, ben)
    assert rel(Kp, cells["s4_K_points"]) < TOL and rel(Kp.sum(-1), cells["s4_K"]) < TOL
    assert rel(SR.s4_B_points(c, s4).sum(-1), cells["s4_B_sum"]) < TOL
    assert rel(SR.nodal_forces(Kp.sum(-1), s4, cells["u"], unit), cells["s4_forces"]) < TOL
    assert rel(SR.stress(c, s4, mem, ben, cells["u"]), cells["s4_nmq"]) < TOL
    # the quirk is visible: a double-precision abscissa gives another matrix
    assert rel(SR.s4_K(c, s4, mem, ben, g=SR.G64), cells["s4_K"]) > 1e-10


def test_restatement_postprocess(cells):
    t = float(cells["membrane"][2])
    for tag in ("s3", "s4"):
        for ztag, z in (("z0", 0.0), ("zt", t / 2)):
            pp = SR.postprocess(cells[f"{tag}_nmq"], t, z)
            for k, v in pp.items():
                assert rel(v, cells[f"{tag}_post_{ztag}_{k}"]) < TOL, (tag, ztag, k)


def _blocks(static):
    return {k: static[k] for k in ("c3d4", "c3d6", "c3d8", "s3", "s4")}


def _material(static):
    return {"E": float(static["E"]), "nu": float(static["nu"]), "membrane": static["membrane"],
            "bending": static["bending"]}


@pytest.fixture(scope="module")
def static_families(static):
    return SR.families(static["coords"], _blocks(static), _material(static))


def test_restatement_operator_product(static, static_families):
    N = static["coords"].shape[0]
    y = SR.operator(N, *static_families)(static["p"])
    assert rel(y, static["Kp"]) < TOL


def test_restatement_driver(static):
    u, it, status, msg = SR.static_structure(static["coords"], static["force"], static["fixed"], _blocks(static),
                                             _material(static), tol=float(static["tol"]), max_iter=20000)
    assert status == "converged"
    assert abs(it - int(static["n_iter"])) <= 2
    assert rel(u, static["u"]) < TOL
    text = str(static["stdout"])
    assert text.startswith("Preprocessing done.\n")
    assert re.sub(r"\d+ iterations", "N iterations", msg.split("Residual")[0]) in \
        re.sub(r"\d+ iterations", "N iterations", text)


def test_block_numbering_round_trip(static):
    from fem355 import system
    N = static["coords"].shape[0]
    dm = system.SixDofMap(N, [static["s3"], static["s4"]])
    on_shell = torch.zeros(N, dtype=torch.bool)
    on_shell[static["s3"].reshape(-1)] = True
    on_shell[static["s4"].reshape(-1)] = True
    ns = int(on_shell.sum())
    assert dm.n_blocks == N + ns and 0 < ns < N
    assert torch.equal(dm.rot_block[on_shell], N + torch.arange(ns))
    assert bool((dm.rot_block[~on_shell] == -1).all())
    x = torch.randn(N, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    xb = dm.to_blocks(x)
    assert tuple(xb.shape) == (dm.n_blocks, 3)
    back = dm.from_blocks(xb, base=x)
    assert torch.equal(back, x)
    zeroed = dm.from_blocks(xb)
    assert torch.equal(zeroed[on_shell], x[on_shell]) and torch.equal(zeroed[:, :3], x[:, :3])
    assert bool((zeroed[~on_shell, 3:] == 0).all())
    w = dm.free_mask(static["fixed"]).view(dm.n_blocks, 3)
    full = torch.ones(N, 6, dtype=torch.float64)
    full[static["fixed"]] = 0.0
    assert torch.equal(w, dm.to_blocks(full))
    load = torch.zeros(N, 6, dtype=torch.float64)
    assert not dm.rowless_load(load)
    load[torch.nonzero(on_shell)[0], 4] = 1.0
    assert not dm.rowless_load(load)
    load[torch.nonzero(~on_shell)[0], 4] = 1.0
    assert dm.rowless_load(load)


def test_block_assembly_equals_dense_6n(static, static_families):
    """Element matrices in the global frame and block order, scattered through the block connectivities, give the
    dense 6N assembly under the dof map (n, c) -> 3 block + c % 3."""
    from fem355 import system
    N = static["coords"].shape[0]
    solids, shells = static_families
    dm = system.SixDofMap(N, [static["s3"], static["s4"]])
    nb = dm.n_blocks
    A = torch.zeros((3 * nb, 3 * nb), dtype=torch.float64)

    def scatter(K, conn):
        dofs = (conn.unsqueeze(-1) * 3 + torch.arange(3)).reshape(conn.shape[0], -1)
        for e in range(conn.shape[0]):
            A[dofs[e].unsqueeze(1), dofs[e].unsqueeze(0)] += K[e]

    for K, el in solids:
        scatter(K, el)
    for K, el, unit in shells:
        order = SR.block_order(el.shape[1])
        scatter(SR.global_K(K, unit)[:, order][:, :, order], dm.shell_connectivity(el))
    dense = SR.dense_K(N, solids, shells)
    node = torch.arange(N)
    rows = torch.cat([(3 * node.unsqueeze(1) + torch.arange(3)).reshape(-1),
                      (3 * dm.rot_block[dm.shell_nodes].unsqueeze(1) + torch.arange(3)).reshape(-1)])
    dofs6 = torch.cat([(6 * node.unsqueeze(1) + torch.arange(3)).reshape(-1),
                       (6 * dm.shell_nodes.unsqueeze(1) + 3 + torch.arange(3)).reshape(-1)])
    assert torch.equal(torch.sort(rows).values, torch.arange(3 * nb))
    assert rel(A[rows][:, rows], dense[dofs6][:, dofs6]) < TOL
    # what the block system leaves out has no rows in the dense matrix either
    rest = torch.ones(6 * N, dtype=torch.bool)
    rest[dofs6] = False
    assert bool((dense[rest] == 0).all()) and bool((dense[:, rest] == 0).all())
    # and the dense matrix is the operator
    p = static["p"]
    assert rel((dense @ p.reshape(-1)).view(N, 6), static["Kp"]) < TOL


def test_small_functions_against_brute_force(cells):
    from fem355 import shell
    tri = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 1, 4], [5, 2, 3]])
    got = shell.identify_s3_shared_edges(tri, device="cpu")
    want = {frozenset([(0, 1), (1, 0)]), frozenset([(1, 1), (2, 0)]), frozenset([(1, 2), (3, 1)])}
    assert {frozenset((int(a), int(b)) for a, b in pair) for pair in got} == want
    edges, third = shell.compute_triangle_surface_faces_with_third_node(tri, device="cpu")
    assert edges.shape[0] == 12 - 2 * 3 and third.shape[0] == edges.shape[0]
    for e, t in zip(edges.tolist(), third.tolist()):
        assert any(set(e) | {t} == set(row) for row in tri.tolist())
    quad = torch.tensor([[0, 1, 4, 3], [1, 2, 5, 4]])
    got = shell.identify_s4_shared_edges(quad, device="cpu")
    assert got.tolist() == [[[0, 1], [1, 3]]]
    edges, fourth = shell.compute_square_surface_faces_with_fourth_node(quad, device="cpu")
    assert edges.shape[0] == 6 and fourth.tolist() == [3, 4, 1, 1, 2, 4]
    assert shell.identify_s3_shared_edges(tri[:1], device="cpu").shape == (0, 2, 2)
    c = cells["coords"]
    x = c[cells["s4"]]
    assert rel(shell.compute_s4_normal(c, cells["s4"], device="cpu"),
               torch.cross(x[:, 1] - x[:, 0], x[:, 3] - x[:, 0], dim=1)) == 0
    x = c[cells["s3"]]
    assert rel(shell.compute_s3_normal(c, cells["s3"], device="cpu"),
               0.5 * torch.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], dim=1)) == 0
    assert rel(shell.compute_kirchoff_D_matrix(cells["membrane"], cells["bending"], device="cpu",
                                               dtype=torch.float64), cells["D"]) < TOL
    pts, w = shell.s4_integration_points(device="cpu")
    assert pts.dtype == torch.float32 and torch.equal(pts.double(), cells["s4_points"]) and w.tolist() == [1.0] * 4
    t = float(cells["membrane"][2])
    pp = shell.compute_shell_postprocess_values(cells["s4_nmq"], t, z=t / 2, device="cpu", dtype=torch.float64)
    for k, v in pp.items():
        assert rel(v, cells[f"s4_post_zt_{k}"]) < TOL, k
    # extrusion of a flat square (two triangles + one quad): normals +z, layers at -+ thickness / 2
    flat = torch.tensor([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0]])
    c3, wedges, hexes = shell.shell_extrude(flat, torch.tensor([[0, 1, 2], [0, 2, 3]]), torch.tensor([[1, 4, 5, 2]]),
                                            0.2, device="cpu", dtype=torch.float64)
    assert torch.allclose(c3[:6, 2], torch.full((6,), -0.1, dtype=torch.float64), atol=1e-7)
    assert torch.allclose(c3[6:, 2], torch.full((6,), 0.1, dtype=torch.float64), atol=1e-7)
    assert wedges.tolist() == [[0, 1, 2, 6, 7, 8], [0, 2, 3, 6, 8, 9]] and hexes.tolist() == [[1, 4, 5, 2, 7, 10, 11, 8]]


def test_solver_exposes_shell_names_package_route():
    from fem355 import shell, solver
    assert sorted(shell.__all__) == sorted(SHELL_NAMES)
    for n in SHELL_NAMES:
        assert callable(getattr(solver, n)), n


def test_solver_exposes_shell_names_flat_route():
    """The reference's loading style: the package directory on sys.path and `import solver`."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import solver; "
            "missing = [n for n in sys.argv[2:] if not callable(getattr(solver, n, None))]; "
            "assert not missing, missing; assert callable(solver.compute_c3d4_K_matrix)")
    out = subprocess.run([sys.executable, "-c", code, fem355.PKG_DIR] + SHELL_NAMES, capture_output=True, text=True,
                         cwd=os.path.join(ROOT, "tests"))
    assert out.returncode == 0, out.stderr[-2000:]
