"""CPU tier of the modal solver: the dense reference LOBPCG of tests/modal_ref.py meets the dense eigenvalues on every
case of the GPU tests, the host Rayleigh-Ritz of the device driver agrees with it, the block width rule, and every
argument check of the new API fires before a device call."""
import pytest
import torch

import fem355  # noqa: F401
import modal_ref as MR
from fem355 import _capi as C
from fem355 import mesh, solver, system

F64 = torch.float64


@pytest.mark.parametrize("name", list(MR.CASES))
def test_reference_lobpcg_meets_the_dense_eigenvalues(name):
    """Worst relative eigenvalue error <= 1e-9 (a cap: the recipe gives 1e-13 .. 5e-12 on these meshes)."""
    cs = MR.case(name)
    lam, X, it, status, rel, restarts = cs.lobpcg
    err = cs.eig_error(lam)
    print(f"{name}: n={cs.n} k={cs.k} m={cs.m}: {it} iterations, {restarts} restarts, eigenvalue error {err:.2e}, "
          f"residual {float(rel.max()):.2e}")
    assert status == MR.CONVERGED
    assert err <= 1e-9, err
    assert float(cs.residuals(lam, X).max()) <= 2e-8
    G = X.T @ cs.M @ X
    assert float((G - torch.eye(cs.k, dtype=F64)).abs().max()) <= 1e-10
    assert bool((X[~cs.free] == 0).all())


def test_rayleigh_ritz_on_the_host():
    g = torch.Generator().manual_seed(3)
    Q = torch.randn(12, 12, dtype=F64, generator=g)
    GM = Q @ Q.T + 12 * torch.eye(12, dtype=F64)
    GK = torch.randn(12, 12, dtype=F64, generator=g)
    GK = GK @ GK.T + torch.eye(12, dtype=F64)
    theta, Cm = system.rayleigh_ritz(GK, GM, 4)
    t2, C2 = MR._ritz(GK, GM, 4)
    assert Cm.shape == (12, 4) and torch.allclose(theta, t2, rtol=1e-13) and bool((theta[1:] >= theta[:-1]).all())
    assert float((Cm.T @ GM @ Cm - torch.eye(4, dtype=F64)).abs().max()) < 1e-12
    assert float((GK @ Cm - GM @ Cm * theta).abs().max()) < 1e-10 * float(GK.abs().max())
    # an unsafe mass Gram matrix is refused: rank deficient, a non-positive diagonal, non-finite entries
    v = torch.randn(12, 1, dtype=F64, generator=g)
    assert system.rayleigh_ritz(GK, v @ v.T, 4) is None
    assert system.rayleigh_ritz(GK, GM - 2 * torch.diag(GM.diagonal()), 4) is None
    assert system.rayleigh_ritz(GK * float("nan"), GM, 4) is None
    assert (system.MODAL_COND, system.MODAL_THETA_FLOOR) == (MR.COND, MR.THETA_FLOOR)


def test_block_width():
    assert [system.modal_block(k) for k in range(1, 9)] == [4, 4, 8, 8, 8, 8, 8, 8]
    assert system.modal_block(1, 1) == 2 and system.modal_block(2, 2) == 2 and system.modal_block(3, 3) == 4
    assert system.modal_block(3, 4) == 4 and system.modal_block(4, 5) == 8 and system.modal_block(8, 8) == 8
    for k, block in ((0, None), (9, None), (4, 3), (4, 9)):
        with pytest.raises(ValueError):
            system.modal_block(k, block)


@pytest.fixture()
def no_device(monkeypatch):
    """Any device call fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("a device call was made before the argument check")
    monkeypatch.setattr(C, "lib", boom)
    monkeypatch.setattr(C, "ptr", boom)
    monkeypatch.setattr(solver, "_dev", boom)
    monkeypatch.setattr(solver, "assemble", boom)
    monkeypatch.setattr(solver, "cached_graph", boom)


def _matrix(graph, bs):
    A = system.SellMatrix.__new__(system.SellMatrix)
    A.g, A.bs, A.device = graph, bs, None
    return A


def test_sell_matrix_checks(no_device):
    g1, g2 = type("G", (), {"n_nodes": 5})(), type("G", (), {"n_nodes": 5})()
    A, M1, M3, Mother = _matrix(g1, 3), _matrix(g1, 1), _matrix(g1, 3), _matrix(g2, 1)
    X = torch.zeros((15, 2), dtype=F64)
    w = torch.ones(15, dtype=F64)
    for fn in (lambda mass: A.matvec_km_multi(mass, X), lambda mass: A.eig_lowest(mass, 2, w)):
        with pytest.raises(ValueError, match="same Graph"):
            fn(Mother)
        with pytest.raises(ValueError, match="bs = 1"):
            fn(M3)
        with pytest.raises(ValueError, match="length 15"):
            fn(torch.ones(14, dtype=F64))
        with pytest.raises(ValueError, match="length 15"):
            fn(torch.ones((15, 1), dtype=F64))
    with pytest.raises(ValueError, match="X must be"):
        A.matvec_km_multi(M1, torch.zeros(15, dtype=F64))
    with pytest.raises(ValueError, match="X must be"):
        A.matvec_km_multi(M1, torch.zeros((14, 2), dtype=F64))
    with pytest.raises(ValueError):
        A.matvec_km_multi(M1, X, max_cols=9)
    for k, block in ((0, None), (9, None), (4, 2), (2, 9)):
        with pytest.raises(ValueError):
            A.eig_lowest(M1, k, w, block=block)
    with pytest.raises(ValueError, match="w must hold"):
        A.eig_lowest(M1, 2, w[:-1])
    with pytest.raises(ValueError, match="X0"):
        A.eig_lowest(M1, 2, w, X0=torch.zeros((14, 2), dtype=F64))
    with pytest.raises(ValueError, match="X0"):
        A.eig_lowest(M1, 2, w, X0=torch.zeros((15, 5), dtype=F64))     # more columns than the block of 4
    with pytest.raises(ValueError, match="max_iter"):
        A.eig_lowest(M1, 2, w, max_iter=-1)


def test_public_solver_checks(no_device):
    c, t = mesh.kuhn_cube(2)
    N, Me = c.shape[0], t.shape[0]
    K = torch.zeros((Me, 12, 12), dtype=F64)
    M = torch.zeros((Me, 12, 12), dtype=F64)
    Ms = torch.zeros((Me, 4, 4), dtype=F64)
    fixed = torch.tensor([0])
    for fn in (solver.vectorized_modal_solver, solver.modal_solver):
        with pytest.raises(ValueError, match="does not fit"):
            fn(K[:, :11, :11], M, t, fixed, N)
        with pytest.raises(ValueError, match="does not fit"):
            fn(K, M[:-1], t, fixed, N)
        with pytest.raises(ValueError, match="does not fit"):
            fn(K, torch.zeros((Me, 8, 8), dtype=F64), t, fixed, N)
        with pytest.raises(ValueError, match="eigenpairs"):
            fn(K, M, t, fixed, N, 0)
        with pytest.raises(ValueError, match="eigenpairs"):
            fn(K, M, t, fixed, N, 9)
        with pytest.raises(ValueError, match="references node"):
            fn(K, M, t, fixed, N - 1)
        with pytest.raises(ValueError, match="fixed node"):
            fn(K, M, t, torch.tensor([N]), N)
    with pytest.raises(ValueError, match="does not fit"):
        solver.vectorized_modal_solver(K, Ms, t, fixed, N)               # the reference takes the full mass only
    with pytest.raises(ValueError, match="3 dofs per node"):
        solver.vectorized_modal_solver(Ms, Ms, t, fixed, N)
    with pytest.raises(ValueError, match="block"):
        solver.modal_solver(K, Ms, t, fixed, N, num_modes=4, block=2)


def test_no_cpu_fallback():
    """With good arguments and no device the first device call fails exactly as the static solvers' does."""
    if torch.cuda.is_available():
        return
    c, t = mesh.kuhn_cube(2)
    N = c.shape[0]
    K = torch.zeros((t.shape[0], 12, 12), dtype=F64)
    with pytest.raises(Exception) as single:
        solver.preconditioned_conjugate_gradient_solver(K, t, torch.zeros((N, 3), dtype=F64), torch.ones((N, 3), dtype=F64))
    for fn in (solver.modal_solver, solver.vectorized_modal_solver):
        with pytest.raises(Exception) as modal:
            fn(K, K, t, torch.tensor([0]), N)
        assert type(modal.value) is type(single.value) and not isinstance(modal.value, ValueError)
