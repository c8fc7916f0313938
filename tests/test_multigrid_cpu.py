"""CPU tier: the mathematics of the geometric multigrid PCG, on the restatement of tests/multigrid_ref.py alone (no
device, none of the package's multigrid code): the uniform refinement (children volumes, conformity), the Galerkin
identity P^T A_f P = A_c of nested P1 spaces with a constant material, symmetry and definiteness of the V-cycle, PCG
against a direct solve, the guard on an underestimated lmax and the iteration counts over the mesh size.

Counts to rtol 1e-8 on the jittered elasticity cube (z = 0 clamped, z = 1 loaded), hierarchy from n = 4, defaults
(degree 2, ratio 30, boost 1.1, 10 power iterations), as this file measures and prints them:
    fine n = 8  (2 levels): multigrid 13, Jacobi 201
    fine n = 16 (3 levels): multigrid 13, Jacobi 450"""
import numpy as np
import pytest
import torch

import multigrid_ref as MG
from twolevel_ref import kuhn_box

F64 = torch.float64
EPS = MG.EPS


def _cube(n, jitter=0.15):
    from fem355 import mesh
    return mesh.kuhn_cube(n, jitter)


def _faces(tets):
    f = torch.stack([tets[:, [0, 1, 2]], tets[:, [0, 1, 3]], tets[:, [1, 2, 3]], tets[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return torch.unique(torch.sort(f, 1).values, dim=0, return_counts=True)[1]


@pytest.mark.parametrize("shape", ["cube2", "beam", "single"])
def test_children_volumes_and_conformity(shape):
    if shape == "cube2":
        c, t = _cube(2)
    elif shape == "beam":
        c, t = kuhn_box(2, 2, 6, (1.0, 1.0, 3.0), 0.15)
    else:
        c = torch.tensor([[0.1, 0.2, 0.0], [1.3, 0.1, 0.2], [0.2, 1.1, 0.1], [0.3, 0.2, 0.9]], dtype=F64)
        t = torch.tensor([[0, 1, 2, 3]])
    cf, tf, parents = MG.refine_ref(c, t)
    vp, vc = MG.tet_volumes(c, t), MG.tet_volumes(cf, tf).view(-1, 8)
    assert bool((vc * vp[:, None] > 0).all()), "a child is oriented against its parent"
    err = (vc.sum(1) - vp).abs() / vp.abs()   # relative to the parent's volume
    print(f"{shape}: volume sum relative err / 2^-52 max {float((err / EPS).max()):.2f}")
    assert bool((err <= 8 * EPS).all())
    # mid nodes are the rounded midpoints of their parents, carried nodes are their parent
    pa, pb = parents[:, 0], parents[:, 1]
    assert torch.equal(cf, 0.5 * (c[pa] + c[pb]))
    counts_c, counts_f = _faces(t), _faces(tf)
    assert int(counts_f.max()) <= 2
    assert int((counts_f == 1).sum()) == 4 * int((counts_c == 1).sum())


@pytest.mark.parametrize("kind", ["poisson", "elastic"])
def test_rediscretised_coarse_matrix_is_the_galerkin_product(kind):
    """E = const, no fixed node: P^T A_f P = A_c entry by entry. Bound per entry: 64 x 2^-52 x the sum of |terms|
    (|P|^T sum|K_e fine| |P| + sum|K_e coarse|): each entry of an element matrix carries a few tens of roundings of its
    own (a 3 x 3 inverse of a Jacobian with condition <= ~10, B^T D B, the volume) relative to the element's terms,
    and the sums add at most the number of terms (<= ~30 per entry), so 64 covers both; an entry without terms must be
    exactly zero."""
    c, t = _cube(2)
    bs = 1 if kind == "poisson" else 3
    cf, tf, parents = MG.refine_ref(c, t)
    Kc, Kf = (MG.element_matrices(x, y, kind, MG.E_MOD, MG.NU) for x, y in ((c, t), (cf, tf)))
    Ac, Af = MG.sparse_matrix(Kc, t, c.shape[0], bs), MG.sparse_matrix(Kf, tf, cf.shape[0], bs)
    Sc, Sf = (MG.sparse_matrix(Kc, t, c.shape[0], bs, True), MG.sparse_matrix(Kf, tf, cf.shape[0], bs, True))
    P = MG.prolongation(parents, c.shape[0], bs)
    G = (P.T @ Af @ P).toarray()
    S = (P.T @ Sf @ P).toarray() + Sc.toarray()
    err = np.abs(G - Ac.toarray())
    ratio = err[S > 0] / (EPS * S[S > 0])
    print(f"{kind}: max |P^T A_f P - A_c| / (2^-52 sum|terms|) = {ratio.max():.2f}")
    assert (err <= 64 * EPS * S).all()


@pytest.fixture(scope="module")
def small():
    """2 -> 4 elasticity cube, clamped at z = 0, loaded at z = 1."""
    from fem355 import mesh
    c, t = _cube(2)
    hier = MG.hierarchy_ref(c, t, 1)
    cf = hier[-1][0]
    F, fixed = mesh.cube_elasticity_case(cf)
    mask = torch.zeros(cf.shape[0], dtype=torch.bool)
    mask[fixed] = True
    return hier, F.reshape(-1), mask


def test_cycle_is_symmetric_positive_definite(small):
    hier, _, mask = small
    ref = MG.MultigridRef(hier, "elastic", fixed=mask)
    M = ref.dense_preconditioner()
    asym = float((M - M.T).abs().max() / M.abs().max())
    lam = torch.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"asymmetry {asym:.2e}, eigenvalues {float(lam[0]):.3e} .. {float(lam[-1]):.3e}")
    assert asym <= 1e-12
    assert float(lam[0]) > 0


def test_pcg_reaches_the_direct_solve(small):
    hier, b, mask = small
    ref = MG.MultigridRef(hier, "elastic", fixed=mask)
    u, it, hist, status = ref.pcg(b, rtol=1e-12, max_iter=200)
    ud = ref.direct(b)
    err = float((u - ud).abs().max() / ud.abs().max())
    print(f"{it} iterations, {status}, u err {err:.2e}")
    assert status == "converged" and err <= 1e-9
    assert bool((u.view(-1, 3)[mask] == 0).all())


def test_halved_lmax_breaks_down_or_converges(small):
    hier, b, mask = small
    for degree in (1, 2, 3):
        ref = MG.MultigridRef(hier, "elastic", fixed=mask, degree=degree, lmax_scale=0.5)
        u, it, hist, status = ref.pcg(b, rtol=1e-8, max_iter=500)
        print(f"degree {degree}: {status} after {it}")
        assert status in ("breakdown", "converged")
        assert bool(torch.isfinite(u).all())


def test_iteration_counts_do_not_grow_with_the_mesh():
    from fem355 import mesh
    c, t = _cube(4)
    hier = MG.hierarchy_ref(c, t, 2)
    counts = {}
    for n, levels in ((8, hier[:2]), (16, hier[:3])):
        cf = levels[-1][0]
        assert cf.shape[0] == (n + 1) ** 3
        F, fixed = mesh.cube_elasticity_case(cf)
        mask = torch.zeros(cf.shape[0], dtype=torch.bool)
        mask[fixed] = True
        ref = MG.MultigridRef(levels, "elastic", fixed=mask)
        b = F.reshape(-1)
        _, it, _, st = ref.pcg(b, rtol=1e-8, max_iter=2000)
        _, itj, _, stj = ref.pcg(b, rtol=1e-8, max_iter=5000, jacobi=True)
        assert st == stj == "converged"
        counts[n] = (it, itj)
        print(f"fine n = {n} ({len(levels)} levels): multigrid {it}, Jacobi {itj}")
    assert counts[16][0] - counts[8][0] <= 3
    assert 2 * counts[16][0] < counts[16][1]
