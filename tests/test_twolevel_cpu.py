"""CPU tier: the arithmetic of the two-level preconditioner M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T in the dense
restatement (tests/twolevel_ref.py) that the device tests compare against -- no device call."""
import pytest
import torch

import twolevel_ref as TL
from oracle import ref_cpu as R

F64 = torch.float64


def _beam():
    c, t, F, fixed = TL.beam_case()
    A, Aabs, Cnt = TL.dense_matrix([(R.tet4_K(c, t, TL.E_MOD, TL.NU), t)], c.shape[0])
    return c, F, A, TL.jacobi_weights(A, fixed), 6


def _cube():
    from fem355 import mesh
    c, t = mesh.kuhn_cube(6, 0.15)
    F, fixed = mesh.cube_elasticity_case(c)
    A, Aabs, Cnt = TL.dense_matrix([(R.tet4_K(c, t, TL.E_MOD, TL.NU), t)], c.shape[0])
    return c, F, A, TL.jacobi_weights(A, fixed), 8


@pytest.fixture(scope="module", params=["beam", "cube"])
def case(request):
    c, F, A, w, k = _beam() if request.param == "beam" else _cube()
    agg = TL.rcb_aggregates(c, w, k)
    return request.param, c, F, A, w, agg, TL.TwoLevelRef(A, c, w, agg)


def test_preconditioner_is_spd_on_the_free_dofs(case):
    _, c, F, A, w, agg, ref = case
    assert ref.k == (6 if case[0] == "beam" else 8) and ref.dropped == 0
    M = ref.dense_preconditioner()
    assert float((M - M.T).abs().max()) <= 1e-14 * float(M.abs().max())
    ev = torch.linalg.eigvalsh(0.5 * (M + M.T))
    assert float(ev[0]) > 0.0, float(ev[0])


def test_preconditioner_does_not_depend_on_the_centres(case):
    """Another centre per aggregate spans the same space: the operator is the same up to rounding, which is what
    makes iteration counts reproducible."""
    _, c, F, A, w, agg, ref = case
    g = torch.Generator().manual_seed(5)
    shift = torch.rand((ref.k, 3), dtype=F64, generator=g) - 0.5
    other = TL.TwoLevelRef(A, c, w, agg, shift=shift)
    r = torch.randn(A.shape[0], dtype=F64, generator=g)
    z0, z1 = ref.apply(r), other.apply(r)
    assert float((z0 - z1).abs().max()) <= 1e-9 * float(z0.abs().max())
    assert float((ref.E - other.E).abs().max()) > 1e-3 * float(ref.E.abs().max())   # the bases do differ


def test_pcg_reaches_the_direct_solve(case):
    _, c, F, A, w, agg, ref = case
    u, it, hist, status = ref.pcg(F, rtol=1e-12, max_iter=2000)
    ud = ref.direct(F)
    assert status == "converged"
    assert float((u - ud).abs().max()) <= 1e-9 * float(ud.abs().max())


def test_two_level_halves_the_iterations_on_the_beam():
    """Both stopped on the true ||r|| < 1e-8 ||b||: 83 against 366 iterations when the issue was written."""
    c, F, A, w, k = _beam()
    ref = TL.TwoLevelRef(A, c, w, TL.rcb_aggregates(c, w, k))
    _, it2, _, s2 = ref.pcg(F, true_rtol=1e-8, max_iter=5000)
    _, it1, _, s1 = ref.pcg(F, true_rtol=1e-8, max_iter=5000, jacobi=True)
    print(f"beam: Jacobi {it1} iterations, two-level {it2}")
    assert s1 == s2 == "converged"
    assert 2 * it2 <= it1, (it2, it1)


def test_two_node_aggregate_drops_one_direction():
    """A 2-node aggregate cannot carry the rotation about its own axis: exactly that direction goes."""
    c, F, A, w, k = _beam()
    agg = two_node_aggregates(c, w, k)
    ref = TL.TwoLevelRef(A, c, w, agg)
    assert ref.k == k + 1 and ref.dropped == 1
    u, it, _, status = ref.pcg(F, true_rtol=1e-8, max_iter=5000)
    _, it1, _, _ = ref.pcg(F, true_rtol=1e-8, max_iter=5000, jacobi=True)
    assert status == "converged" and 2 * it <= it1, (it, it1)
    ud = ref.direct(F)
    assert float((u - ud).abs().max()) <= 1e-6 * float(ud.abs().max())


def test_route_names_package_and_flat():
    """two_level_pcg_solver and solve_tet4's kwargs through `solver`, as a package and in the reference's loading
    style (the package directory on sys.path and `import solver`); the argument checks need no device."""
    import inspect
    import os
    import subprocess
    import sys

    import fem355
    from fem355 import solver
    sig = inspect.signature(solver.solve_tet4)
    assert sig.parameters["preconditioner"].default == "jacobi" and sig.parameters["n_aggregates"].default is None
    assert list(inspect.signature(solver.two_level_pcg_solver).parameters)[:5] == ["K", "elements", "coords", "F",
                                                                                   "fixed"]
    c = torch.zeros((4, 3), dtype=F64)
    t = torch.tensor([[0, 1, 2, 3]])
    for bad in (dict(kind="poisson"), dict(kind="elastic", operator="matfree")):
        with pytest.raises(ValueError):
            solver.solve_tet4(c, t, c, [0], preconditioner="two-level", device="cpu", **bad)
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import solver, inspect; "
            "assert callable(solver.two_level_pcg_solver); "
            "assert 'preconditioner' in inspect.signature(solver.solve_tet4).parameters")
    out = subprocess.run([sys.executable, "-c", code, fem355.PKG_DIR], capture_output=True, text=True,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert out.returncode == 0, out.stderr[-2000:]


def two_node_aggregates(c, w, k):
    """The RCB aggregates plus one more made of two neighbouring free nodes of the last one."""
    agg = TL.rcb_aggregates(c, w, k)
    last = torch.nonzero(agg == k - 1).view(-1)
    agg[last[-2:]] = k
    return agg
