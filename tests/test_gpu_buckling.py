"""Linear buckling on the device: the geometric stiffness kernel (csrc/buckling.hip), its use as the `mass` operand of
the fused kernels, the block subspace iteration SellMatrix.buckling_lowest, and the public solvers
linear_buckling_solver / stress_stiffened_modal_solver -- against the dense CPU reference of tests/buckling_ref.py.

Meshes: mesh.kuhn_cube(3), hex_box(4), wedge_box(3), tet10_cube(2) with the coordinates scaled by (1, 1.5, 8); the
kernel tests jitter the interior nodes by 0.15 h (every detJ keeps its sign: checked on the CPU). E = 1000, nu = 0.3.
Tolerances: max|dG| <= 1e-12 max|G| (the project's yardstick for element kernels); 1e-12 for the operator products
(test_gpu_modal._check_product); for the eigenpairs at tol = 1e-8: recomputed residuals <= 2 tol, |X^T K X - I| <=
1e-10, eigenvalue error <= 8 x subspace_ref's with a floor of 1e-12 relative, K-sine to the dense eigenvector <=
rho_j / gap_j + 1e-10 (Davis-Kahan in the K inner product), outer iterations within 2 of subspace_ref's.

Measured on the MI355X: kernel against the reference 9e-17 to 8.3e-16 of max|G| over the four types, three input
combinations and M = 1, 5, all, 300; K X and G X 3.8e-16 to 1.7e-15; eigenpairs (outer iterations device / subspace_ref,
eigenvalue error device / subspace_ref):
    hex   m 4   20 / 20   5.5e-12 / 3.6e-12        hex   m 8   14 / 14   4.3e-12 / 2.7e-12
    tet10 m 4   12 / 12   1.4e-11 / 8.6e-12        tet10 m 8   10 / 10   1.7e-11 / 1.3e-11
reference solve by PCG against the dense direct solve 1.1e-12; thermal prestress factors 2068.79, 2137.95 (dense equal to
6e-14); mixed c3d8 + c3d6 column 4.0e-12; stress-stiffened lowest eigenvalue 7.11 -> 3.76 (dense equal to 8.4e-12)."""
import pytest
import torch

import buckling_ref as B
from conftest import rel

pytestmark = pytest.mark.gpu

F64 = torch.float64
TOL = 1e-8
KINDS = {"c3d4": ("tet", 3), "c3d8": ("hex", 4), "c3d6": ("wedge", 3), "c3d10": ("tet10", 2)}
BIG = 300     # elements of the tiled mesh: two 256-element blocks, the second one partial


# ---------------------------------------------------------------- 1. the element kernel
class KernelCase:
    """A jittered mesh with gaps in its node ids (node i of the mesh is node 2 i + 1), seeded inputs, and the
    reference blocks of the three input combinations, formed once."""

    def __init__(self, et):
        from fem355 import mesh
        kind, n = KINDS[et]
        gen = {"tet": mesh.kuhn_cube, "hex": mesh.hex_box, "wedge": mesh.wedge_box, "tet10": mesh.tet10_cube}[kind]
        c, el = gen(n, jitter=0.15)
        c = c * B.SCALE
        det = B.jacobians(c, el, et)[1]
        assert bool((det > 0).all()) or bool((det < 0).all())
        g = torch.Generator().manual_seed(11 + len(et))
        N, M = c.shape[0], el.shape[0]
        self.et, self.M = et, M
        self.c = torch.full((2 * N + 2, 3), float("nan"), dtype=F64)
        self.c[1:2 * N:2] = c
        self.u = torch.zeros_like(self.c)
        self.u[1:2 * N:2] = 1e-2 * torch.randn(N, 3, dtype=F64, generator=g)
        self.el = 2 * el + 1
        self.s0 = torch.randn(M, 3, 3, dtype=F64, generator=g)       # not symmetric: only the upper triangle counts
        u = self.u[1:2 * N:2]
        self.ref = {"u": B.geo_scalar(c, el, et, u, B.E, B.NU), "s0": B.geo_scalar(c, el, et, sigma0=self.s0),
                    "both": B.geo_scalar(c, el, et, u, B.E, B.NU, self.s0)}
        self.plain = (c, el)

    def args(self, mode, idx, dev):
        kw = {}
        if mode in ("u", "both"):
            kw.update(displacement=self.u.to(dev), E=B.E, nu=B.NU)
        if mode in ("s0", "both"):
            kw.update(prestress=self.s0[idx].to(dev))
        return kw


_KC = {}


def kcase(et):
    if et not in _KC:
        _KC[et] = KernelCase(et)
    return _KC[et]


@pytest.mark.parametrize("mode", ["u", "s0", "both"])
@pytest.mark.parametrize("et", list(KINDS))
def test_kernel_against_reference(gpu, et, mode):
    from fem355 import element
    kc = kcase(et)
    ref = kc.ref[mode]
    top = float(ref.abs().max())
    for count in (1, 5, kc.M, BIG):
        idx = torch.arange(count) % kc.M
        if count == 5:
            idx = idx + (kc.M - 5)                      # the last five: not the ones the single-element case takes
        G = element.compute_geometric_stiffness(kc.c.to(gpu), kc.el[idx].to(gpu), et, device=gpu, dtype=F64,
                                                **kc.args(mode, idx, gpu))
        assert G.shape == (count, B.NPE[et], B.NPE[et]) and G.dtype == F64 and G.is_cuda
        err = float((G.cpu() - ref[idx]).abs().max()) / top
        print(f"{et} {mode} M={count}: max|dG| / max|G| = {err:.2e}")
        assert torch.equal(G, G.transpose(1, 2))        # symmetric bit for bit
        assert err <= 1e-12, (et, mode, count, err)


@pytest.mark.parametrize("et", list(KINDS))
def test_patch_identity_on_the_device(gpu, et):
    """Uniform stress S, linear fields f = p.x and g = q.x: f^T Gs g = V p^T S q, V = 1 x 1.5 x 8."""
    from fem355 import element
    c, el = kcase(et).plain
    g = torch.Generator().manual_seed(2)
    S = torch.randn(3, 3, dtype=F64, generator=g)
    S = S + S.T
    p, q = torch.randn(3, dtype=F64, generator=g), torch.randn(3, dtype=F64, generator=g)
    Gs = element.compute_geometric_stiffness(c, el, et, prestress=S.expand(el.shape[0], 3, 3), device=gpu,
                                             dtype=F64).cpu()
    got = float(torch.einsum("ma,mab,mb->", (c @ p)[el], Gs, (c @ q)[el]))
    V = float(B.SCALE.prod())
    want, scale = V * float(p @ S @ q), V * float(p.norm() * S.norm() * q.norm())
    print(f"{et}: {got:.15e} vs {want:.15e} ({abs(got - want) / scale:.2e})")
    assert abs(got - want) <= 1e-12 * scale
    assert float(Gs.sum(dim=2).abs().max()) <= 1e-12 * float(Gs.abs().max())


@pytest.mark.parametrize("et", list(KINDS))
def test_degenerate_element_raises(gpu, et):
    from fem355 import element
    c, el = kcase(et).plain
    s0 = torch.ones(2, 3, 3, dtype=F64)
    flat = c.clone()
    flat[el[1]] = 0.0                                   # every node of element 1 at the origin: J = 0 exactly
    with pytest.raises(ValueError, match="Singular matrix"):
        element.compute_geometric_stiffness(flat, el[:2], et, prestress=s0, device=gpu)
    nanc = c.clone()
    nanc[el[0, 0], 1] = float("nan")
    with pytest.raises(ValueError, match="Singular matrix"):
        element.compute_geometric_stiffness(nanc, el[:2], et, prestress=s0, device=gpu)
    ok = element.compute_geometric_stiffness(c, el[:2], et, prestress=s0, device=gpu)   # the healthy pair passes
    assert ok.dtype == torch.float32 and bool(torch.isfinite(ok).all())


def test_full_matrix_is_the_kronecker_product(gpu):
    from fem355 import element
    kc = kcase("c3d8")
    idx = torch.arange(kc.M)
    kw = kc.args("both", idx, gpu)
    Gs = element.compute_geometric_stiffness(kc.c.to(gpu), kc.el.to(gpu), "c3d8", device=gpu, dtype=F64, **kw)
    Gf = element.compute_geometric_stiffness(kc.c.to(gpu), kc.el.to(gpu), "c3d8", device=gpu, dtype=F64, scalar=False,
                                             **kw)
    assert Gf.shape == (kc.M, 24, 24)
    assert torch.equal(Gf.cpu(), B.kron3(Gs.cpu()))


# ---------------------------------------------------------------- 2. the operator
class Dev:
    """Device matrices of a one-family reference column: K from the device element kernels, G from the kernel at the
    dense reference state, the Jacobi weights."""

    def __init__(self, dev, cs):
        from fem355 import element, solver, system
        self.cs, self.dev = cs, dev
        c, el, et = cs.c.to(dev), cs.el.to(dev), cs.et
        self.g = system.build_graph(el, cs.N)
        self.A, self.G = system.SellMatrix(self.g, 3), system.SellMatrix(self.g, 1)
        self.A.add_element_matrices(solver._buckling_ke(c, el, et, B.E, B.NU, dev), el)
        self.G.add_element_matrices(element.compute_geometric_stiffness(c, el, et, cs.u.to(dev), B.E, B.NU, device=dev,
                                                                        dtype=F64), el)
        mask = torch.zeros((cs.N, 3), dtype=torch.uint8, device=dev)
        mask[cs.fixed.to(dev)] = 1
        self.w = self.A.jacobi(mask.view(-1))


_DEV = {}


@pytest.fixture(scope="module")
def devcase(gpu):
    def get(kind, n):
        if (kind, n) not in _DEV:
            _DEV[(kind, n)] = Dev(gpu, B.column(kind, n))
        return _DEV[(kind, n)]
    yield get
    _DEV.clear()


COLUMNS = [("hex", 4), ("tet10", 2)]


@pytest.mark.parametrize("kind,n", COLUMNS)
def test_fused_product_with_g_as_the_mass(devcase, kind, n):
    dc = devcase(kind, n)
    cs = dc.cs
    X = torch.randn(cs.n, 8, dtype=F64, generator=torch.Generator().manual_seed(9))
    refK, refG = cs.K @ X, cs.G @ X
    for L in (1, 3, 4, 8):
        Y, Z = dc.A.matvec_km_multi(dc.G, X[:, :L].contiguous().to(dc.dev))
        eK = max(rel(Y[:, j], refK[:, j]) for j in range(L))
        eG = max(rel(Z[:, j], refG[:, j]) for j in range(L))
        print(f"{kind} L={L}: K X {eK:.2e}, G X {eG:.2e}")
        assert eK < 1e-12 and eG < 1e-12, (L, eK, eG)


@pytest.mark.parametrize("kind,n", COLUMNS)
def test_scaled_add_of_g(devcase, kind, n):
    dc = devcase(kind, n)
    cs = dc.cs
    s = 0.37 * float(-1.0 / cs.pairs[0][0])
    rp, ci, bv = dc.A.scaled_add_mass(dc.G, 1.0, s).csr()
    rp, ci, bv = rp.cpu().long(), ci.cpu().long(), bv.cpu()
    rows = torch.repeat_interleave(torch.arange(cs.N), rp[1:] - rp[:-1])
    dense = torch.zeros((cs.N, 3, cs.N, 3), dtype=F64)
    dense[rows, :, ci, :] = bv
    want = cs.K + s * cs.G
    err = float((dense.view(cs.n, cs.n) - want).abs().max() / want.abs().max())
    print(f"{kind}: K + s K_g against the dense sum {err:.2e}")
    assert err <= 1e-12


# ---------------------------------------------------------------- 3. the solve
@pytest.mark.parametrize("m", [4, 8])
@pytest.mark.parametrize("kind,n", COLUMNS)
def test_eigenpairs(devcase, kind, n, m):
    from fem355 import _capi as C
    dc = devcase(kind, n)
    cs = dc.cs
    k = 3
    res = dc.A.buckling_lowest(dc.G, k, dc.w, block=m, tol=TOL)
    theta_d, U = cs.pairs
    ref = B.subspace_ref(cs.K, cs.G, cs.free, k, m, tol=TOL)
    assert ref[4] == B.CONVERGED
    ref_err = float(((ref[1] - theta_d[:k]).abs() / theta_d[:k].abs()).max())
    err = float(((res.theta - theta_d[:k]).abs() / theta_d[:k].abs()).max())
    X = res.X.cpu()
    rec = cs.residuals(res.theta, X)
    orth = float((X.T @ cs.K @ X - torch.eye(k, dtype=F64)).abs().max())
    print(f"{kind} m={m}: factors {res.factors.tolist()}; {res.iterations} outer iterations (subspace_ref {ref[3]}), "
          f"{res.linear_iterations} inner; eigenvalue error {err:.2e} vs subspace_ref {ref_err:.2e}; residuals "
          f"reported {float(res.residuals.max()):.2e} recomputed {float(rec.max()):.2e}; |X^T K X - I| {orth:.2e}")
    assert res.status == C.PCG_CONVERGED and not res.inner_failed
    assert res.factors.shape == res.theta.shape == (k,) and res.X.shape == (cs.n, k)
    assert bool((res.factors.abs()[1:] >= res.factors.abs()[:-1]).all())
    assert torch.equal(res.factors, -1.0 / res.theta)
    assert float(rec.max()) <= 2 * TOL, rec
    assert orth <= 1e-10, orth
    assert bool((X[~cs.free] == 0).all())
    f = cs.free
    Lk = torch.linalg.cholesky(cs.K[f][:, f])
    Rr = ((cs.G @ X) - (cs.K @ X) * res.theta)[f]
    rho = torch.linalg.solve_triangular(Lk, Rr, upper=False).norm(dim=0)      # ||r||_{K^-1}, x K-normalised
    for j in range(k):
        others = torch.cat([theta_d[:j], theta_d[j + 1:]])
        gap = float((others - res.theta[j]).abs().min())
        x, u = X[:, j], U[:, j]
        d = x - u * float(u @ (cs.K @ x))
        sine = float(torch.sqrt(d @ (cs.K @ d)) / torch.sqrt(x @ (cs.K @ x)))
        print(f"  mode {j}: lambda {float(res.factors[j]):.6e} sine {sine:.2e} bound {float(rho[j]) / gap:.2e}")
        assert sine <= float(rho[j]) / gap + 1e-10, (j, sine, float(rho[j]) / gap)
    assert err <= max(8 * ref_err, 1e-12), (err, ref_err)
    assert abs(res.iterations - ref[3]) <= 2, (res.iterations, ref[3])


# ---------------------------------------------------------------- 4. behaviour
def test_same_seed_same_bits(devcase):
    dc = devcase("hex", 4)
    a = dc.A.buckling_lowest(dc.G, 3, dc.w, block=4, tol=TOL, history=True)
    b = dc.A.buckling_lowest(dc.G, 3, dc.w, block=4, tol=TOL, history=True)
    assert a.iterations == b.iterations and a.linear_iterations == b.linear_iterations
    assert torch.equal(a.theta, b.theta) and torch.equal(a.X, b.X) and torch.equal(a.residuals, b.residuals)
    assert a.history.shape == (a.iterations + 1, 3) and torch.equal(a.history, b.history)
    assert torch.equal(a.history[-1], a.residuals)
    c = dc.A.buckling_lowest(dc.G, 3, dc.w, block=4, tol=TOL, seed=1)
    assert not torch.equal(c.X, a.X) and rel(c.theta, a.theta) < 1e-9


def test_public_solver_and_reversed_load(gpu, capsys):
    """linear_buckling_solver from the load: its own reference solve (Jacobi-PCG to 1e-10 of sqrt(b.w b)) against the
    dense direct solve. The factors are linear in 1 / u_ref, and the PCG's error in u_ref is bounded by
    sqrt(cond(W K)) times its residual bound -- below 1e-6 relative on these 375-dof columns."""
    from fem355 import _capi as C
    from fem355 import solver
    cs = B.column("hex", 4)
    capsys.readouterr()
    lam, modes, u, res = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", cs.F, cs.fixed, B.E, B.NU, num_modes=3,
                                                       block=8, tol=TOL, device=gpu, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    want = -1.0 / cs.pairs[0][:3]
    print(f"factors {lam.tolist()} (dense {want.tolist()}), u_ref error {rel(u, cs.u):.2e}")
    assert res.status == C.PCG_CONVERGED
    assert lam.shape == (3,) and modes.shape == (3, cs.N, 3) and u.shape == (cs.N, 3) and lam.dtype == F64
    assert len(lines) == 3 and all(ln.startswith(f"Mode {j + 1}: load factor = ") for j, ln in enumerate(lines))
    assert torch.equal(modes.permute(1, 2, 0).reshape(cs.n, 3), res.X) and torch.equal(lam.cpu(), res.factors)
    assert rel(u, cs.u) < 1e-6 and bool((u[cs.fixed.to(gpu)] == 0).all())
    assert float(((lam.cpu() - want).abs() / want.abs()).max()) < 1e-6
    assert bool((lam > 0).all())                            # compression buckles at a positive factor
    lam2, _, u2 = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", -cs.F, cs.fixed, B.E, B.NU, num_modes=3, block=8,
                                                tol=TOL, device=gpu)
    print(f"reversed load: u_ref against the negated one {rel(u2, -u):.2e}, factors {lam2.tolist()}")
    assert float(((lam2 + lam).abs() / lam.abs()).max()) <= 1e-9
    # the reference state handed in: no solve, the dense state's factors
    lam3, _, u3 = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", None, cs.fixed, B.E, B.NU, num_modes=3, block=8,
                                                tol=TOL, u_ref=cs.u, device=gpu)
    assert torch.equal(u3.cpu(), cs.u) and float(((lam3.cpu() - want).abs() / want.abs()).max()) < 1e-9


def test_thermal_prestress(gpu):
    """A c3d4 column clamped at both ends and heated uniformly: the stress of compute_thermal_element_stress at the
    thermal displacement is the whole reference state (F = None). The factor (on the temperature rise) is positive and
    finite and equals the dense reference's; an eigenvalue converged to a residual of 1e-8 is off by the residual
    squared over the gap, far below the 1e-9 asked here."""
    from fem355 import _capi as C
    from fem355 import loads, solver
    base = B.column("tet", 3)
    c, el = base.c, base.el
    ends = torch.nonzero((c[:, 2].abs() <= 1e-12) | ((c[:, 2] - 8.0).abs() <= 1e-12), as_tuple=True)[0]
    cs = B.Column(c, [("c3d4", el)], torch.zeros((base.N, 3), dtype=F64), fixed=ends)
    alpha, dT = 1e-5, 10.0
    f = loads.compute_thermal_load(c, el, "c3d4", B.E, B.NU, alpha, dT, device=gpu, dtype=F64).cpu()
    u = cs.solve(f)
    sig, _ = loads.compute_thermal_element_stress(c, el, "c3d4", u, B.E, B.NU, alpha, dT, device=gpu, dtype=F64)
    assert float(sig[:, 2, 2].max()) < 0.0                  # axial compression everywhere
    G = cs.geometric(sigma0={"c3d4": sig.cpu()})
    theta_d, _ = B.dense_pairs(cs.K, G, cs.free)
    lam, modes, u0, res = solver.linear_buckling_solver(c, el, "c3d4", None, ends, B.E, B.NU, num_modes=2,
                                                        prestress=sig, tol=TOL, device=gpu, return_info=True)
    want = -1.0 / theta_d[:2]
    print(f"thermal: factors {lam.tolist()} (dense {want.tolist()}) after {res.iterations} iterations")
    assert res.status == C.PCG_CONVERGED and bool((u0 == 0).all())
    assert 0.0 < float(lam[0]) < float("inf")
    assert float(((lam.cpu() - want).abs() / want.abs()).max()) <= 1e-9
    assert float(cs.residuals(res.theta, res.X, G).max()) <= 2 * TOL


def test_zero_load_breaks_down(gpu, capsys):
    from fem355 import _capi as C
    from fem355 import solver
    cs = B.column("hex", 4)
    capsys.readouterr()
    lam, modes, u, res = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", torch.zeros_like(cs.F), cs.fixed, B.E, B.NU,
                                                       num_modes=3, device=gpu, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert res.status == C.PCG_BREAKDOWN and res.iterations == 0
    assert lines[0].startswith("Buckling solver: breakdown at iteration 0")
    assert bool((u == 0).all()) and bool(torch.isfinite(res.X).all())


def test_max_iter_is_reported(devcase, gpu, capsys):
    from fem355 import _capi as C
    from fem355 import solver
    cs = B.column("hex", 4)
    capsys.readouterr()
    lam, _, _, res = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", None, cs.fixed, B.E, B.NU, num_modes=3, block=4,
                                                   u_ref=cs.u, max_iter=1, tol=TOL, device=gpu, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert res.status == C.PCG_MAXITER and res.iterations == 1 and not res.inner_failed
    assert lines[0] == f"Buckling solver: reached max_iter (1) with residual {float(res.residuals.max()):.3e}"
    assert bool(torch.isfinite(lam).all()) and float(res.residuals.max()) > TOL
    # an inner solve that cannot converge is told apart
    capsys.readouterr()
    _, _, _, res = solver.linear_buckling_solver(cs.c, cs.el, "c3d8", None, cs.fixed, B.E, B.NU, num_modes=3, block=4,
                                                 u_ref=cs.u, linear_max_iter=2, tol=TOL, device=gpu, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert res.status == C.PCG_MAXITER and res.inner_failed and res.iterations == 0
    assert lines[0] == "Buckling solver: an inner solve did not converge in 2 iterations (outer iteration 1)"


def _mixed_column():
    """hex_box(4) as a column with the layer of cells i = 1 (a slab normal to x) cut into wedges: the interfaces to the
    hex layers are the wedges' unsplit quadrilateral faces, so the mesh conforms."""
    from fem355 import mesh
    c, el, _ = B.column_mesh("hex", 4)
    layer = (torch.arange(el.shape[0]) // 16) == 1
    wedges = torch.stack([el[layer][:, list(s)] for s in mesh.WEDGE_SPLIT], dim=1).reshape(-1, 6).contiguous()
    return B.Column(c, [("c3d8", el[~layer].contiguous()), ("c3d6", wedges)], B.top_load(c))


def test_mixed_mesh(gpu):
    from fem355 import _capi as C
    from fem355 import solver
    cs = _mixed_column()
    assert cs.fams[0][1].shape == (48, 8) and cs.fams[1][1].shape == (32, 6)
    want = -1.0 / cs.pairs[0][:3]
    lam, modes, u, res = solver.linear_buckling_solver(cs.c, dict(cs.fams), None, None, cs.fixed, B.E, B.NU,
                                                       num_modes=3, block=8, u_ref=cs.u, tol=TOL, device=gpu,
                                                       return_info=True)
    err = float(((lam.cpu() - want).abs() / want.abs()).max())
    print(f"mixed c3d8 + c3d6: factors {lam.tolist()} (dense {want.tolist()}), error {err:.2e}")
    assert res.status == C.PCG_CONVERGED
    assert err <= 1e-9                                      # residual^2 / gap, as in test_thermal_prestress
    assert float(cs.residuals(res.theta, res.X).max()) <= 2 * TOL


def test_stress_stiffened_modes(gpu, capsys):
    """Half the first buckling load: the lowest frequency drops below the unstressed one and equals the dense eigh of
    (K + 0.5 lambda_1 K_g, M) -- a LOBPCG eigenvalue at residual 1e-8 is off by the residual squared over the gap.
    On hex_box(4) scaled by (1, 1.5, 3): on the 8 : 1 column of the other tests modal_solver's Jacobi-preconditioned
    LOBPCG itself needs over 1200 iterations at m = 4 and breaks down at m = 8, stressed or not (the dense restatement
    modal_ref.lobpcg_ref does the same), which is eig_lowest's matter and would only make this test slow."""
    import modal_ref as MR
    from fem355 import _capi as C
    from fem355 import element, mesh, solver
    c, el = mesh.hex_box(4)
    c = c * torch.tensor([1.0, 1.5, 3.0], dtype=F64)
    cs = B.Column(c, [("c3d8", el)], B.top_load(c))
    rho = 2.0
    lam1 = float(-1.0 / cs.pairs[0][0])
    Ms = MR.hex_scalar_mass(cs.c, cs.el, rho)
    Md = B.dense(B.kron3(Ms), cs.el, cs.N, 3)
    f = cs.free

    def lowest(Kd):
        L = torch.linalg.cholesky(Md[f][:, f])
        T = torch.linalg.solve_triangular(L, Kd[f][:, f], upper=False)
        T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)
        return torch.linalg.eigvalsh(0.5 * (T + T.T))[:3]

    want, plain = lowest(cs.K + 0.5 * lam1 * cs.G), lowest(cs.K)
    Ke = solver._buckling_ke(cs.c.to(gpu), cs.el.to(gpu), "c3d8", B.E, B.NU, gpu)
    Gs = element.compute_geometric_stiffness(cs.c, cs.el, "c3d8", cs.u, B.E, B.NU, device=gpu, dtype=F64)
    capsys.readouterr()
    freq, lam, modes, res = solver.stress_stiffened_modal_solver(Ke, Ms, Gs, cs.el, cs.fixed, cs.N,
                                                                 load_factor=0.5 * lam1, num_modes=3, block=8,
                                                                 tol=TOL, device=gpu, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    err = float(((lam.cpu() - want).abs() / want).max())
    print(f"stressed lambda {lam.tolist()} (dense {want.tolist()}, unstressed {plain.tolist()}), error {err:.2e}")
    assert res.status == C.PCG_CONVERGED and len(lines) == 3
    assert freq.shape == (3,) and modes.shape == (3, cs.N, 3)
    assert float(lam[0]) < float(plain[0]) and float(freq[0]) < float(torch.sqrt(plain[0]) / (2 * torch.pi))
    assert err <= 1e-9


def test_bad_arguments_are_refused(gpu, monkeypatch):
    """Every refusal comes before the library is touched."""
    from fem355 import _capi as C
    from fem355 import element, solver, system
    cs = B.column("hex", 4)
    c, el, F, fx = cs.c, cs.el, cs.F, cs.fixed
    dc_g = system.build_graph(el.to(gpu), cs.N)
    A, G1, G3 = system.SellMatrix(dc_g, 3), system.SellMatrix(dc_g, 1), system.SellMatrix(dc_g, 3)
    other = system.SellMatrix(system.build_graph(el.to(gpu), cs.N), 1)
    w = torch.ones(cs.n, dtype=F64, device=gpu)

    def no_library():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(C, "lib", no_library)
    s0 = torch.zeros(el.shape[0], 3, 3, dtype=F64)
    for kw in (dict(), dict(displacement=cs.u), dict(displacement=cs.u, E=1.0), dict(displacement=cs.u[:-1], E=1.0, nu=0.3),
               dict(prestress=s0[:-1]), dict(prestress=s0.view(-1, 9))):
        with pytest.raises(ValueError):
            element.compute_geometric_stiffness(c, el, "c3d8", device=gpu, **kw)
    with pytest.raises(ValueError, match="Unsupported element type"):
        element.compute_geometric_stiffness(c, el, "c3d20", prestress=s0, device=gpu)
    with pytest.raises(ValueError):
        element.compute_geometric_stiffness(c, el[:, :6], "c3d8", prestress=s0, device=gpu)
    for G, k, ww, kw in ((G3, 3, w, {}), (other, 3, w, {}), (w, 3, w, {}), (G1, 9, w, {}), (G1, 3, w[:-1], {}),
                         (G1, 3, w, {"block": 2}), (G1, 3, w, {"max_iter": -1})):
        with pytest.raises(ValueError):
            A.buckling_lowest(G, k, ww, **kw)
    with pytest.raises(ValueError):
        G1.buckling_lowest(G1, 3, w[: cs.N])              # the stiffness must be bs = 3
    good = dict(num_modes=3, device=gpu)
    for args, kw in (((c, el, "c3d20", F, fx, B.E, B.NU), good), ((c, el[:, :6], "c3d8", F, fx, B.E, B.NU), good),
                     ((c, el, "c3d8", F[:-1], fx, B.E, B.NU), good), ((c, el, "c3d8", None, fx, B.E, B.NU), good),
                     ((c, el, "c3d8", F, fx, B.E, 0.5), good), ((c, el, "c3d8", F, fx, -1.0, B.NU), good),
                     ((c, el, "c3d8", F, fx, B.E, B.NU), dict(num_modes=9, device=gpu)),
                     ((c, el, "c3d8", F, fx, B.E, B.NU), dict(num_modes=3, block=2, device=gpu)),
                     ((c, el, "c3d8", F, torch.tensor([cs.N]), B.E, B.NU), good),
                     ((c, el, "c3d8", F, torch.zeros(0, dtype=torch.long), B.E, B.NU), good),
                     ((c, el, "c3d8", F, fx, B.E, B.NU), dict(prestress=s0[:-1], **good)),
                     ((c, el, "c3d8", F, fx, B.E, B.NU), dict(u_ref=cs.u[:-1], **good)),
                     ((c, el, "c3d8", F, fx, B.E, B.NU), dict(tol=0.0, **good)),
                     ((c[:-1], el, "c3d8", F[:-1], fx, B.E, B.NU), good),
                     ((c, {"c3d8": el, "s4": el[:, :4]}, None, F, fx, B.E, B.NU), good)):
        with pytest.raises(ValueError):
            solver.linear_buckling_solver(*args, **kw)
    Ke = torch.zeros(el.shape[0], 24, 24, dtype=F64)
    Ms = torch.zeros(el.shape[0], 8, 8, dtype=F64)
    for args, kw in (((Ke, Ms, Ms[:-1], el, fx, cs.N), {}), ((Ke, Ms, Ke, el, fx, cs.N), {}),
                     ((Ke[:, :8, :8], Ms, Ms, el, fx, cs.N), {}), ((Ke, Ms, Ms, el, fx, cs.N), {"num_modes": 9}),
                     ((Ke, Ms, Ms, el, fx, cs.N), {"block": 2, "num_modes": 3}), ((Ke, Ms, Ms, el, fx, cs.N - 1), {})):
        with pytest.raises(ValueError):
            solver.stress_stiffened_modal_solver(*args, device=gpu, **kw)
