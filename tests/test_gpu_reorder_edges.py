"""Node renumbering on the device (system.rcm_order, fem_rcm of csrc/reorder.hip) on the graphs its machinery needs:
frontiers wider than the 256 workgroups (chunks of 1, 2, 3, more than 1024 and more than 4096 nodes that all carry
children), sweeps that end just before, on and after a 48-launch batch, components far apart in a sparse id range,
nodes without elements around the scan tile, the degenerate sizes of the C ABI, and the solves that go through
solve_tet4(reorder="rcm") with 3 dofs per node, the matrix-free operator and a per-element modulus.

Every permutation is compared exactly with oracle/rcm_ref.py, or, for the two widest cases, with its level-by-level
restatement tests/rcm_levels_ref.py (pinned to the oracle in tests/test_reorder_cpu.py). Before a case touches the
device, rcm_levels_ref.assert_regime asserts on the reference's level structure that the input reaches the path it is
there for; the kernel's constants it needs (CM_G 256, CM_NT 1024, CM_CHUNK 4096, the cursor stride 16384, BATCH 48) are
copied there. Solves: the contract of test_gpu_reorder.py, rel(u, oracle PCG on the caller's numbering) < 1e-10 and
iterations within +-2.

fem_rcm loops on the host until the device reports that it is done: a counting bug can show as a run that never comes
back rather than as a failure."""
import numpy as np
import pytest
import torch

import rcm_levels_ref as L
import topopt_ref as TR
from conftest import rel
from oracle import ref_cpu as R
from oracle import rcm_ref

pytestmark = pytest.mark.gpu
F64, I32 = torch.float64, torch.int32
E, NU = 113.8e9, 0.342


def _mods():
    import fem355  # noqa: F401
    from fem355 import mesh, solver, system
    return mesh, solver, system


# ---------------------------------------------------------------- every family against the reference
@pytest.mark.parametrize("name", L.NAMES)
def test_device_rcm_on_edge_families(gpu, name):
    _, _, system = _mods()
    t, N, rp, ci, s = L.case(name)
    L.assert_regime(name, N, rp, s)
    print(f"{name}: N {N}, {s.components} components, widths {[w[:6] for w in s.widths[:3]]}, widest "
          f"{max(map(max, s.widths))}, {s.launches} count launches")
    if name in L.LARGE:
        operm, oinv = s.perm, s.inv
    else:
        operm, oinv = rcm_ref.rcm(rp, ci, N)
    td = t.to(gpu)
    perm, inv = system.rcm_order(td, N)
    assert np.array_equal(perm.cpu().numpy(), operm) and np.array_equal(inv.cpu().numpy(), oinv), name
    perm2, inv2 = system.rcm_order(td, N)
    assert torch.equal(perm, perm2) and torch.equal(inv, inv2)        # deterministic under another arrival order


# ---------------------------------------------------------------- the C ABI's degenerate sizes
def _lib():
    import fem355  # noqa: F401
    from fem355 import _capi as C
    return C, C.lib()


def _raw_rcm(C, lib, rowptr, colidx, N, gpu, fill=-7):
    rp = torch.tensor(rowptr, dtype=I32, device=gpu)
    ci = torch.tensor(colidx, dtype=I32, device=gpu)
    perm = torch.full((max(N, 1),), fill, dtype=I32, device=gpu)
    inv = torch.full((max(N, 1),), fill, dtype=I32, device=gpu)
    work = torch.empty(int(lib.fem_rcm_work_len(N)), dtype=I32, device=gpu)
    rc = lib.fem_rcm(C.ptr(rp), C.ptr(ci), N, C.ptr(perm), C.ptr(inv), C.ptr(work), None, C.stream(gpu))
    torch.cuda.synchronize()
    return rc, perm.tolist(), inv.tolist()


@pytest.mark.parametrize("N", [5, 1])
def test_abi_no_edges_is_the_identity(gpu, N):
    """A rowptr of zeros: k_cm_reset finds no start node and the sweep is done before it begins; every node is
    numbered by the scan of the nodes without neighbours."""
    C, lib = _lib()
    rc, perm, inv = _raw_rcm(C, lib, [0] * (N + 1), [0], N, gpu)
    C.check(rc, "fem_rcm")
    assert perm == inv == list(range(N))


def test_abi_one_node_with_a_self_edge(gpu):
    C, lib = _lib()
    rc, perm, inv = _raw_rcm(C, lib, [0, 1], [0], 1, gpu)
    C.check(rc, "fem_rcm")
    assert perm == inv == [0]


def test_abi_no_nodes_touches_nothing(gpu):
    C, lib = _lib()
    assert int(lib.fem_rcm_work_len(0)) > 0
    rc, perm, inv = _raw_rcm(C, lib, [0], [0], 0, gpu)
    assert rc == C.FEM_OK and perm == inv == [-7]


def test_abi_misaligned_work_is_refused(gpu):
    C, lib = _lib()
    N = 5
    rp = torch.zeros(N + 1, dtype=I32, device=gpu)
    ci = torch.zeros(1, dtype=I32, device=gpu)
    perm = torch.full((N,), -7, dtype=I32, device=gpu)
    inv = torch.full((N,), -7, dtype=I32, device=gpu)
    work = torch.empty(int(lib.fem_rcm_work_len(N)) + 2, dtype=I32, device=gpu)
    assert work.data_ptr() % 8 == 0
    rc = lib.fem_rcm(C.ptr(rp), C.ptr(ci), N, C.ptr(perm), C.ptr(inv), C.ptr(work[1:]), None, C.stream(gpu))
    assert rc == C.FEM_EARG and "8-byte aligned" in lib.fem_last_error().decode()
    with pytest.raises(C.FemError, match="8-byte aligned"):
        C.check(rc, "fem_rcm")
    torch.cuda.synchronize()
    assert perm.tolist() == inv.tolist() == [-7] * N


# ---------------------------------------------------------------- reordered solves
UNUSED = 7


def _renumbered_cube():
    """kuhn_cube(8, jitter=0.1) under a random renumbering, plus UNUSED node ids no element touches (placed inside the
    cube, away from every face the load cases select)."""
    mesh, _, _ = _mods()
    c, t = mesh.kuhn_cube(8, jitter=0.1)
    n = c.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(9))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    c = torch.cat([c[perm], torch.full((UNUSED, 3), 0.5, dtype=F64)])
    return c, inv[t]


@pytest.mark.parametrize("config", ["elastic", "elastic-matfree", "poisson-modulus"])
def test_reordered_solve_configurations(gpu, config):
    """solve_tet4(reorder="rcm") where it also permutes a [N, 3] load and mask (elastic), runs the matrix-free operator,
    and keeps a per-element modulus in element order. Load case and stop: the unreordered tests of the same
    configuration -- the bench's elasticity case at rtol 1e-8 (test_gpu_matfree.test_pcg_vs_oracle_and_assembled), the
    cantilever's z load as a scalar source at rtol 1e-13 (test_gpu_topopt.test_solve_tet4_with_a_modulus_scale).
    The UNUSED nodes stay in: their rows are empty, their Jacobi weight is 0 and u stays 0 there."""
    mesh, solver, system = _mods()
    c, t = _renumbered_cube()
    N = c.shape[0]
    scale = None
    if config == "poisson-modulus":
        dpn, kw, rtol = 1, dict(kind="poisson", E=1.0, nu=0.0), 1e-13
        F, mask = TR.cantilever(c)
        f, fixed = F[:, 2:3].clone(), torch.nonzero(mask[:, 0]).view(-1)
        scale = (1 + torch.arange(t.shape[0]) % 3).to(F64)
        kw["modulus_scale"] = scale.to(gpu)
        K = R.tet4_poisson_K(c, t) * scale.view(-1, 1, 1)
    else:
        dpn, kw, rtol = 3, dict(kind="elastic", E=E, nu=NU), 1e-8
        f, fixed = mesh.cube_elasticity_case(c)
        if config == "elastic-matfree":
            kw["operator"] = "matfree"
        K = R.tet4_K(c, t, E, NU)
    dinv = R.diag_preconditioner(K, t, N, dpn=dpn)
    dinv[fixed] = 0.0
    b = f.reshape(N, dpn).to(F64)
    tol = rtol * float(torch.sqrt((b * dinv * b).sum()))
    u_ref, it_ref, status = R.pcg(K, t, b, dinv, tol=tol, max_iter=5000)
    assert status == "converged" and float(u_ref[-UNUSED:].abs().max()) == 0.0
    u, res, A = solver.solve_tet4(c, t, f, fixed, rtol=rtol, device=gpu, reorder="rcm", **kw)
    d = rel(u.cpu().reshape(N, dpn), u_ref)
    print(f"reordered solve {config}: {res.iterations} iterations (oracle {it_ref}), rel {d:.2e} (bound 1e-10)")
    assert bool(getattr(A, "is_matfree", False)) == (config == "elastic-matfree")
    assert d < 1e-10 and abs(res.iterations - it_ref) <= 2
    assert float(u[-UNUSED:].abs().max()) == 0.0
    _, inv = system.rcm_order(t.to(gpu), N)
    assert torch.equal(u, res.x.view(N, dpn)[inv])
