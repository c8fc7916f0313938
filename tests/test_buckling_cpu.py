"""CPU tier: the dense buckling reference of tests/buckling_ref.py pinned against identities that do not depend on it.

  * patch identity: for a uniform stress S and linear nodal fields f = p.x, g = q.x the geometric stiffness gives
    f^T Gs g = V p^T S q exactly (the gradients of linear fields are reproduced at every point and the rule integrates
    |detJ| exactly), summed over a jittered mesh: 1e-12 relative;
  * rows of Gs_e sum to zero (the shape functions sum to one) and Gs_e is symmetric;
  * a slender hex column (2 x 3 x 8 hexes, 1 x 1.5 x 10, clamped at z = 0, unit axial compression, E = 1000,
    nu = 0.3): lambda = 5.1096, 8.9466, 44.722, a spectrum mixed in sign, subspace_ref equal to the dense eigh, and
    tension giving the negated factors."""
import pytest
import torch

import buckling_ref as B

F64 = torch.float64
KINDS = [("tet", 3), ("hex", 3), ("wedge", 3), ("tet10", 2)]


def _mesh(kind, n):
    from fem355 import mesh
    gen = {"tet": mesh.kuhn_cube, "hex": mesh.hex_box, "wedge": mesh.wedge_box, "tet10": mesh.tet10_cube}[kind]
    et = {"tet": "c3d4", "hex": "c3d8", "wedge": "c3d6", "tet10": "c3d10"}[kind]
    c, el = gen(n, jitter=0.15)
    return c * B.SCALE, el, et


@pytest.mark.parametrize("kind,n", KINDS)
def test_patch_identity(kind, n):
    c, el, et = _mesh(kind, n)
    _, det = B.jacobians(c, el, et)
    assert bool((det > 0).all()) or bool((det < 0).all())          # the jitter inverts nothing
    g = torch.Generator().manual_seed(3)
    S = torch.randn(3, 3, dtype=F64, generator=g)
    S = S + S.T
    p, q = torch.randn(3, dtype=F64, generator=g), torch.randn(3, dtype=F64, generator=g)
    M = el.shape[0]
    s0 = S.expand(M, 3, 3).clone()
    s0[:, 1, 0] = 7.0                                              # the lower triangle is not read
    Gs = B.geo_scalar(c, el, et, sigma0=s0)
    f, h = (c @ p)[el], (c @ q)[el]
    got = torch.einsum("ma,mab,mb->", f, Gs, h)
    V = float(B.SCALE.prod())                                      # the jitter moves interior nodes only
    want = V * float(p @ S @ q)
    scale = V * float(p.norm() * S.norm() * q.norm())
    print(f"{et}: f^T Gs g = {float(got):.15e}, V p^T S q = {want:.15e}, error {abs(float(got) - want) / scale:.2e}")
    assert abs(float(got) - want) <= 1e-12 * scale


@pytest.mark.parametrize("kind,n", KINDS)
def test_rows_sum_to_zero_and_symmetry(kind, n):
    c, el, et = _mesh(kind, n)
    g = torch.Generator().manual_seed(5)
    u = 1e-3 * torch.randn(c.shape[0], 3, dtype=F64, generator=g)
    s0 = torch.randn(el.shape[0], 3, 3, dtype=F64, generator=g)
    for kw in ({"u": u, "E_": B.E, "nu": B.NU}, {"sigma0": s0}, {"u": u, "E_": B.E, "nu": B.NU, "sigma0": s0}):
        Gs = B.geo_scalar(c, el, et, **kw)
        top = float(Gs.abs().max())
        assert float(Gs.sum(dim=2).abs().max()) <= 1e-12 * top
        assert float((Gs - Gs.transpose(1, 2)).abs().max()) <= 1e-14 * top
    both = B.geo_scalar(c, el, et, u, B.E, B.NU, s0)
    parts = B.geo_scalar(c, el, et, u, B.E, B.NU) + B.geo_scalar(c, el, et, sigma0=s0)
    assert float((both - parts).abs().max()) <= 1e-13 * float(both.abs().max())    # linear in the stress


def test_c3d4_is_the_closed_form():
    """One point, weight 1/6: Gs = V g_a^T sigma g_b with the oracle's P1 gradients."""
    from oracle import ref_cpu as R
    c, el, et = _mesh("tet", 3)
    s0 = torch.randn(el.shape[0], 3, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    s0 = s0 + s0.transpose(1, 2)
    g = R.tet4_gradients(c, el)
    want = torch.einsum("m,mai,mik,mbk->mab", R.tet_volumes(c, el), g, s0, g)
    got = B.geo_scalar(c, el, et, sigma0=s0)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_slender_column_factors():
    cs = B.slender_hex_column()
    theta, U = cs.pairs
    lam = -1.0 / theta[:3]
    print(f"lambda {lam.tolist()}, largest positive theta {float(theta.max()):.3e}")
    assert torch.allclose(lam, torch.tensor([5.1096, 8.9466, 44.722], dtype=F64), rtol=2e-5)
    assert float(theta.min()) < 0.0 < float(theta.max()) and abs(float(theta.max()) - 2e-5) < 1e-6
    gram = U[:, :3].T @ cs.K @ U[:, :3]
    assert float((gram - torch.eye(3, dtype=F64)).abs().max()) <= 1e-10


@pytest.mark.parametrize("m", [4, 8])
def test_subspace_ref_against_dense(m):
    cs = B.slender_hex_column()
    theta, U = cs.pairs
    lam, th, X, its, status, rel = B.subspace_ref(cs.K, cs.G, cs.free, 3, m)
    err = float(((th - theta[:3]).abs() / theta[:3].abs()).max())
    print(f"m = {m}: {its} outer iterations, eigenvalue error {err:.2e}, residuals {rel.tolist()}")
    assert status == B.CONVERGED and float(rel.max()) <= 1e-8
    assert its <= {8: 14, 4: 25}[m]          # 12 and 22 here
    assert err <= 1e-10
    assert float(cs.residuals(th, X).max()) <= 2e-8
    assert float((X.T @ cs.K @ X - torch.eye(3, dtype=F64)).abs().max()) <= 1e-10
    assert bool((X[~cs.free] == 0).all())
    assert bool((lam.abs()[1:] >= lam.abs()[:-1]).all())
    for j in range(3):                        # the mode is the dense eigenvector up to sign
        assert abs(abs(float(U[:, j] @ cs.K @ X[:, j])) - 1.0) <= 1e-6


def test_reversed_load_negates_the_factors():
    a, b = B.slender_hex_column(), B.slender_hex_column(-1.0)
    la, lb = -1.0 / a.pairs[0][:3], -1.0 / b.pairs[0][:3]
    assert float(((la + lb).abs() / la.abs()).max()) <= 1e-12
    r = B.subspace_ref(b.K, b.G, b.free, 3, 8)
    assert r[4] == B.CONVERGED and float(((r[0] - lb).abs() / lb.abs()).max()) <= 1e-9 and bool((r[0] < 0).all())


def test_no_prestress_breaks_down():
    cs = B.slender_hex_column()
    r = B.subspace_ref(cs.K, torch.zeros_like(cs.G), cs.free, 3, 4)
    assert r[4] == B.BREAKDOWN and r[3] == 0
