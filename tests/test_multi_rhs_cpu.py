"""CPU tier of the multi-load-case solvers: argument checks that must fire before any device call, the split of L
right-hand sides into lock-step passes, and the per-column view of a MultiPcgResult."""
import pytest
import torch

import fem355  # noqa: F401
from fem355 import _capi as C
from fem355 import mesh, solver, system


@pytest.fixture(scope="module")
def case():
    c, t = mesh.kuhn_cube(2)
    N = c.shape[0]
    K = torch.zeros((t.shape[0], 12, 12), dtype=torch.float64)
    return c, t, N, K


@pytest.fixture()
def no_device(monkeypatch):
    """Any device call fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("a device call was made before the argument check")
    monkeypatch.setattr(C, "lib", boom)
    monkeypatch.setattr(solver, "_dev", boom)
    monkeypatch.setattr(solver, "assemble", boom)


def _solvers(K, t, N):
    minv = torch.ones((N, 3), dtype=torch.float64)
    return [
        ("cg", lambda F, **kw: solver.multi_load_cg_solver(K, t, F, torch.tensor([0]), **kw)),
        ("pcg", lambda F, **kw: solver.multi_load_pcg_solver(K, t, F, minv, **kw)),
    ]


@pytest.mark.parametrize("which", [0, 1])
def test_bad_loads_raise_before_any_device_call(case, no_device, which):
    c, t, N, K = case
    _, call = _solvers(K, t, N)[which]
    with pytest.raises(ValueError, match=r"\[L, N, dpn\]"):
        call(torch.zeros((N, 3), dtype=torch.float64))                     # not 3-D
    with pytest.raises(ValueError, match="no load case"):
        call(torch.zeros((0, N, 3), dtype=torch.float64))                  # L = 0
    with pytest.raises(ValueError, match="dofs per node"):
        call(torch.zeros((2, N, 1), dtype=torch.float64))                  # dpn does not match K / elements
    with pytest.raises(ValueError, match="references node"):
        call(torch.zeros((2, N - 1, 3), dtype=torch.float64))              # N does not match elements
    with pytest.raises(ValueError, match="u_init"):
        call(torch.zeros((2, N, 3), dtype=torch.float64), u_init=torch.zeros((N, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="u_init"):
        call(torch.zeros((2, N, 3), dtype=torch.float64), u_init=torch.zeros((3, N, 3), dtype=torch.float64))


def test_pcg_solver_checks_m_inv(case, no_device):
    c, t, N, K = case
    with pytest.raises(ValueError, match="M_inv"):
        solver.multi_load_pcg_solver(K, t, torch.zeros((2, N, 3), dtype=torch.float64),
                                     torch.ones((N, 1), dtype=torch.float64))


def test_solve_tet4_multi_checks(case, no_device):
    c, t, N, K = case
    fixed = torch.tensor([0])
    with pytest.raises(ValueError, match=r"\[L, N, dpn\]"):
        solver.solve_tet4_multi(c, t, torch.zeros((N, 1), dtype=torch.float64), fixed)
    with pytest.raises(ValueError, match="no load case"):
        solver.solve_tet4_multi(c, t, torch.zeros((0, N, 1), dtype=torch.float64), fixed)
    with pytest.raises(ValueError, match="dofs per node"):
        solver.solve_tet4_multi(c, t, torch.zeros((2, N, 1), dtype=torch.float64), fixed, kind="elastic")
    with pytest.raises(ValueError, match="dofs per node"):
        solver.solve_tet4_multi(c, t, torch.zeros((2, N, 3), dtype=torch.float64), fixed, kind="poisson")
    with pytest.raises(ValueError):
        solver.solve_tet4_multi(c, t, torch.zeros((2, N + 1, 1), dtype=torch.float64), fixed)
    with pytest.raises(ValueError, match="kind"):
        solver.solve_tet4_multi(c, t, torch.zeros((2, N, 1), dtype=torch.float64), fixed, kind="shell")


def test_no_cpu_fallback(case):
    """With good arguments and no device the first device call fails exactly as the single solver's does."""
    if torch.cuda.is_available():
        return
    c, t, N, K = case
    minv = torch.ones((N, 3), dtype=torch.float64)
    with pytest.raises(Exception) as single:
        solver.preconditioned_conjugate_gradient_solver(K, t, torch.zeros((N, 3), dtype=torch.float64), minv)
    with pytest.raises(Exception) as multi:
        solver.multi_load_pcg_solver(K, t, torch.zeros((2, N, 3), dtype=torch.float64), minv)
    assert type(multi.value) is type(single.value) and not isinstance(multi.value, ValueError)


def test_multi_passes():
    assert system.MULTI_NV == (2, 4, 8)
    assert system.multi_passes(11) == [(0, 8, 8), (8, 3, 4)]
    assert system.multi_passes(1) == [(0, 1, 2)]
    assert system.multi_passes(2) == [(0, 2, 2)]
    assert system.multi_passes(3) == [(0, 3, 4)]
    assert system.multi_passes(5) == [(0, 5, 8)]
    assert system.multi_passes(8) == [(0, 8, 8)]
    assert system.multi_passes(9) == [(0, 8, 8), (8, 1, 2)]
    assert system.multi_passes(20) == [(0, 8, 8), (8, 8, 8), (16, 4, 4)]
    for L in range(1, 40):
        p = system.multi_passes(L)
        assert sum(k for _, k, _ in p) == L and all(k <= nv <= 8 and nv in system.MULTI_NV for _, k, nv in p)
        assert [j for j, _, _ in p] == [sum(k for _, k, _ in p[:i]) for i in range(len(p))]
    with pytest.raises(ValueError):
        system.multi_passes(0)
    # bs = 3 takes 4 columns per pass (measured: DESIGN.md); max_cols overrides, up to the widest kernel
    assert system.MULTI_MAX == {1: 8, 3: 4}
    assert system.multi_passes(11, 3) == [(0, 4, 4), (4, 4, 4), (8, 3, 4)]
    assert system.multi_passes(5, 3) == [(0, 4, 4), (4, 1, 2)]
    assert system.multi_passes(8, 3) == [(0, 4, 4), (4, 4, 4)]
    assert system.multi_passes(8, 3, max_cols=8) == [(0, 8, 8)]
    assert system.multi_passes(11, 1, max_cols=4) == system.multi_passes(11, 3)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            system.multi_passes(4, 3, max_cols=bad)


def test_result_column_round_trip():
    x = torch.arange(12, dtype=torch.float64).view(4, 3)
    hist = torch.arange(15, dtype=torch.float64).view(5, 3)
    res = system.MultiPcgResult(x, [5, 2, 1], [C.PCG_MAXITER, C.PCG_CONVERGED, C.PCG_BREAKDOWN], [1.0, 2.0, 3.0],
                                [4.0, 5.0, 6.0], hist)
    for j in range(3):
        c = res.column(j)
        assert isinstance(c, system.PcgResult)
        assert torch.equal(c.x, x[:, j])
        assert (c.iterations, c.status, c.rz, c.pq) == (res.iterations[j], res.status[j], res.rz[j], res.pq[j])
        assert torch.equal(c.history, hist[: res.iterations[j], j])
    assert system.MultiPcgResult(x, [1], [0], [0.0], [0.0]).column(0).history is None


def test_pcg_multi_argument_checks(monkeypatch):
    """SellMatrix.pcg_multi / matvec_multi refuse misshapen input before touching the library."""
    monkeypatch.setattr(C, "lib", lambda: (_ for _ in ()).throw(AssertionError("device call")))
    A = system.SellMatrix.__new__(system.SellMatrix)
    A.g = type("G", (), {"n_nodes": 5})()
    A.bs = 3
    A.device = None
    w = torch.ones(15, dtype=torch.float64)
    with pytest.raises(ValueError):
        A.matvec_multi(torch.zeros(15, dtype=torch.float64))
    with pytest.raises(ValueError):
        A.matvec_multi(torch.zeros((14, 2), dtype=torch.float64))
    with pytest.raises(ValueError):
        A.pcg_multi(torch.zeros((15, 0), dtype=torch.float64), w=w)
    with pytest.raises(ValueError):
        A.pcg_multi(torch.zeros((15, 2), dtype=torch.float64), x0=torch.zeros((15, 3), dtype=torch.float64), w=w)
    with pytest.raises(ValueError):
        A.pcg_multi(torch.zeros((15, 2), dtype=torch.float64), w=w[:-1])
    with pytest.raises(ValueError):
        A.pcg_multi(torch.zeros((15, 2), dtype=torch.float64), w=w, tol=[1e-8, 1e-8, 1e-8])
