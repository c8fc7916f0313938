"""Modal analysis on the device (csrc/modal.hip): the fused K/M product, the Gram, rotation and residual kernels, and
the block LOBPCG (SellMatrix.eig_lowest, solver.vectorized_modal_solver, solver.modal_solver) against the dense CPU
reference of tests/modal_ref.py.

Meshes: mesh.kuhn_cube(n, jitter=0.15) / mesh.hex_box(n) scaled by (1, 0.7, 2), z = 0 face clamped, E = 113.8e9,
nu = 0.342, rho = 4430 (modal_ref.CASES).
Tolerances: torch.equal against matvec_multi (same sums in the same order), 1e-12 against the oracle's element-by-
element products (the project's operator tolerance), 1e-13 relative to ||a|| ||b|| for the tall-skinny kernels (a dot
product of n <= 3993 terms rounds to about sqrt(n) eps = 1.4e-14 of that), and for the eigenpairs at tol = 1e-8:
recomputed residuals <= 2 tol (rounding of order eps lambda_max / lambda_1 = 1e-11, three orders below tol),
X^T M X = I to 1e-10, eigenvalue error <= 8 x the reference LOBPCG's worst error on the same case (the margin of the
hard-geometry tests), M-sine to the dense eigenvector <= rho_j / gap_j + 1e-10 (Davis-Kahan).

Measured on the MI355X (eigenvalue error against the dense solve: device, reference LOBPCG, ratio; bound 8):
    elastic4  (375 dofs, k 4, m 8)   105 iterations   1.56e-12   1.25e-12   1.24
    elastic6  (1029, 6, 8)           233              3.51e-12   7.65e-12   0.46
    elastic8  (2187, 3, 4)           520              1.55e-11   1.56e-11   0.99
    lumped5   (648, 6, 8)            139              1.16e-12   1.26e-12   0.92
    poisson6  (343, 6, 8)             62              2.63e-13   2.56e-13   1.02
    hex4      (375, 4, 8)             89              3.31e-12   1.64e-12   2.01
Both errors sit at the rounding floor of the dense solve itself (eps lambda_max / lambda_1 ~ 1e-12), so the ratio is a
ratio of two rounding errors; test_eigenpairs prints the figures of every run."""
import ctypes

import pytest
import torch

import modal_ref as MR
from conftest import rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
TOL = 1e-8


# ---------------------------------------------------------------- device operators of a modal_ref case
class Dev:
    def __init__(self, dev, cs, compress=True):
        from fem355 import system
        self.cs, self.dev = cs, dev
        el = cs.el.to(dev)
        self.g = system.build_graph(el, cs.N, compress=compress)
        self.A, self.Mg = system.SellMatrix(self.g, cs.dpn), system.SellMatrix(self.g, 1)
        if cs.dpn == 3:
            self.A.add_stiffness_and_mass(cs.Ke.to(dev), cs.Ms.to(dev), el, self.Mg)
        else:
            self.A.add_element_matrices(cs.Ke.to(dev), el)
            self.Mg.add_element_matrices(cs.Ms.to(dev), el)
        mask = torch.zeros((cs.N, cs.dpn), dtype=torch.uint8, device=dev)
        mask[cs.fixed.to(dev)] = 1
        self.w = self.A.jacobi(mask.view(-1))


_DEV = {}


@pytest.fixture(scope="module")
def devcase(gpu):
    def get(name, clamp=True, compress=True):
        key = (name, clamp, compress)
        if key not in _DEV:
            _DEV[key] = Dev(gpu, MR.case(name, clamp), compress)
        return _DEV[key]
    yield get
    _DEV.clear()


# ---------------------------------------------------------------- 1. the fused product
LS = (1, 2, 3, 4, 5, 8)


def _check_product(A, Mg, Ke, Ms, el, N, dpn, seed):
    """matvec_km_multi with both mass forms against matvec_multi of each matrix (bit for bit) and the oracle."""
    n = N * dpn
    X = torch.randn(n, max(LS), dtype=F64, generator=torch.Generator().manual_seed(seed))
    Me = torch.kron(Ms, torch.eye(dpn, dtype=F64).view(1, dpn, dpn))
    refK = torch.stack([R.nodal_forces(Ke, el, X[:, j].reshape(N, dpn)).reshape(-1) for j in range(max(LS))], 1)
    refM = torch.stack([R.nodal_forces(Me, el, X[:, j].reshape(N, dpn)).reshape(-1) for j in range(max(LS))], 1)
    Xd = X.to(A.device)
    d = torch.rand(n, dtype=F64, generator=torch.Generator().manual_seed(seed + 1)).to(A.device) + 0.5
    for L in LS:
        XL = Xd[:, :L].contiguous()
        Y, Z = A.matvec_km_multi(Mg, XL)
        Yd, Zd = A.matvec_km_multi(d, XL)
        Y1 = A.matvec_multi(XL)
        # the mass is M_s (x) I: component r of M X is the scalar matrix applied to component r of X
        Z1 = torch.stack([Mg.matvec_multi(XL.view(N, dpn, L)[:, r, :].contiguous()) for r in range(dpn)], 1).view(n, L)
        assert Y.shape == Z.shape == (n, L) and Y.dtype == F64
        eK, eM = max(rel(Y[:, j], refK[:, j]) for j in range(L)), max(rel(Z[:, j], refM[:, j]) for j in range(L))
        print(f"dpn={dpn} L={L}: K X vs oracle {eK:.2e}, M X vs oracle {eM:.2e}")
        assert torch.equal(Y, Y1) and torch.equal(Yd, Y1), L
        assert torch.equal(Z, Z1), L
        assert torch.equal(Zd, d[:, None] * XL), L
        assert eK < 1e-12 and eM < 1e-12, (L, eK, eM)


@pytest.mark.parametrize("op", ["elastic", "poisson"])
@pytest.mark.parametrize("n", [4, 10])
@pytest.mark.parametrize("compress", [True, False], ids=["delta16", "int32"])
def test_product_tets(gpu, op, n, compress):
    from fem355 import mesh, system
    c, t = mesh.kuhn_cube(n, jitter=0.15)
    c = c * MR.SCALE
    N, dpn = c.shape[0], 3 if op == "elastic" else 1
    if n == 4:
        assert N == 125       # a partial last slice
    else:
        assert (N + 63) // 64 == 21
    Ke = R.tet4_K(c, t, MR.E, MR.NU) if op == "elastic" else R.tet4_poisson_K(c, t)
    Ms = MR.tet_scalar_mass(c, t)
    g = system.build_graph(t.to(gpu), N, compress=compress)
    assert (g.dcols is not None) == compress
    A, Mg = system.SellMatrix(g, dpn), system.SellMatrix(g, 1)
    A.add_element_matrices(Ke.to(gpu), t.to(gpu))
    Mg.add_element_matrices(Ms.to(gpu), t.to(gpu))
    _check_product(A, Mg, Ke, Ms, t, N, dpn, 10 * n + dpn)


def test_product_hexes(gpu):
    """hex_box(4): the c3d8 stiffness and the scalar mass from the device element kernels, assembled in one pass."""
    from fem355 import element, mesh, system
    c, h = mesh.hex_box(4)
    c = c * MR.SCALE
    N = c.shape[0]
    cg, hg = c.to(gpu), h.to(gpu)
    Ke = element.compute_c3d8_K_matrix(cg, hg, MR.E, MR.NU, device=gpu, dtype=F64)
    Ms = element.compute_M_matrix(cg, hg, "c3d8", MR.RHO, device=gpu, dtype=F64, scalar=True)
    g = system.build_graph(hg, N)
    A, Mg = system.SellMatrix(g, 3), system.SellMatrix(g, 1)
    A.add_stiffness_and_mass(Ke, Ms, hg, Mg)
    _check_product(A, Mg, Ke.cpu(), Ms.cpu(), h, N, 3, 5)


# ---------------------------------------------------------------- 2. Gram, rotation, residual
TAIL = 64   # sentinel rows past row n


class Vecs:
    """Nine seeded multi-vectors [n, m] (X W P KX KW KP MX MW MP) living in buffers with a NaN tail past row n."""

    def __init__(self, dev, n, m, seed):
        g = torch.Generator().manual_seed(seed)
        self.n, self.m = n, m
        self.host = [torch.randn(n, m, dtype=F64, generator=g) for _ in range(9)]
        self.buf = [torch.full((n + TAIL, m), float("nan"), dtype=F64, device=dev) for _ in range(9)]
        for b, h in zip(self.buf, self.host):
            b[:n] = h.to(dev)
        self.ptrs = (ctypes.c_void_p * 9)(*[b.data_ptr() for b in self.buf])

    def tails_untouched(self):
        return all(bool(torch.isnan(b[self.n:]).all()) for b in self.buf)


def _sizes(gpu):
    from fem355 import mesh
    return [3 * mesh.kuhn_cube(n)[0].shape[0] for n in (4, 10)]   # 375 and 3993 dofs: no multiple of the row tile


@pytest.mark.parametrize("a", [2, 3], ids=["noP", "P"])
@pytest.mark.parametrize("m", [2, 4, 8])
def test_gram(gpu, m, a):
    from fem355 import _capi as C
    lib = C.lib()
    for n in _sizes(gpu):
        assert n % 32
        v = Vecs(gpu, n, m, 100 * m + a)
        work = torch.empty(int(lib.fem_modal_work_len()), dtype=F64, device=gpu)
        outs = []
        for _ in range(2):
            out = torch.full((C.MODAL_OUT_LEN,), float("nan"), dtype=F64, device=gpu)
            C.check(lib.fem_modal_gram(n, m, a, v.ptrs, C.ptr(work), C.ptr(out), C.stream(gpu)), "fem_modal_gram")
            outs.append(out.cpu())
        assert torch.equal(torch.nan_to_num(outs[0]), torch.nan_to_num(outs[1]))
        am = a * m
        S = torch.cat(v.host[0:a], 1)
        for name, off, lo in (("G_K", 0, 3), ("G_M", C.MODAL_OUT_GM, 6)):
            G = outs[0][off: off + am * am].view(am, am)
            T = torch.cat(v.host[lo: lo + a], 1)
            ref = S.T @ T
            ref = ref.triu() + ref.triu(1).T          # the upper triangle is computed and mirrored
            scale = S.norm(dim=0)[:, None] * T.norm(dim=0)[None, :]
            scale = scale.triu() + scale.triu(1).T
            err = float(((G - ref).abs() / scale).max())
            print(f"gram n={n} m={m} a={a} {name}: {err:.2e}")
            assert torch.equal(G, G.T)
            assert err <= 1e-13, (n, name, err)      # finite: the NaN rows past n were not read
        assert v.tails_untouched()


@pytest.mark.parametrize("a", [1, 2, 3], ids=["X", "noP", "P"])
@pytest.mark.parametrize("m", [2, 4, 8])
def test_rotate(gpu, m, a):
    from fem355 import _capi as C
    lib = C.lib()
    for n in _sizes(gpu):
        Cm = torch.randn(a * m, m, dtype=F64, generator=torch.Generator().manual_seed(7 * m + a))
        coef = Cm.reshape(-1).to(gpu)
        res = []
        for _ in range(2):
            v = Vecs(gpu, n, m, 200 * m + a)
            C.check(lib.fem_modal_rotate(n, m, a, v.ptrs, C.ptr(coef), C.stream(gpu)), "fem_modal_rotate")
            res.append([b[:n].cpu() for b in v.buf])
            assert v.tails_untouched()
        worst = 0.0
        for f in range(3):
            X, W, P = v.host[3 * f: 3 * f + 3]
            S = torch.cat([X, W, P][:a], 1)
            Pn = torch.cat([W, P][: a - 1], 1) @ Cm[m:] if a >= 2 else P
            Xn = S @ Cm
            bound = S.norm(dim=1)[:, None] * Cm.norm(dim=0)[None, :]
            worst = max(worst, float(((res[0][3 * f] - Xn).abs() / bound).max()))
            assert torch.equal(res[0][3 * f + 1], W)       # W is read only
            if a >= 2:
                worst = max(worst, float(((res[0][3 * f + 2] - Pn).abs() / bound).max()))
            else:
                assert torch.equal(res[0][3 * f + 2], P)   # a = 1 leaves P alone
        print(f"rotate n={n} m={m} a={a}: {worst:.2e}")
        assert worst <= 1e-13, (n, worst)
        assert all(torch.equal(x, y) for x, y in zip(*res))


@pytest.mark.parametrize("m", [2, 4, 8])
def test_residual(gpu, m):
    from fem355 import _capi as C
    lib = C.lib()
    for n in _sizes(gpu):
        g = torch.Generator().manual_seed(300 + m)
        theta = torch.rand(m, dtype=F64, generator=g) + 0.5
        w = torch.rand(n, dtype=F64, generator=g) + 0.5
        w[torch.randperm(n, generator=g)[: n // 7]] = 0.0         # fixed dofs
        work = torch.empty(int(lib.fem_modal_work_len()), dtype=F64, device=gpu)
        res, wd, thd = [], w.to(gpu), theta.to(gpu)
        for _ in range(2):
            v = Vecs(gpu, n, m, 400 + m)
            out = torch.zeros(C.MODAL_OUT_LEN, dtype=F64, device=gpu)
            C.check(lib.fem_modal_residual(n, m, C.ptr(v.buf[3]), C.ptr(v.buf[6]), C.ptr(wd), C.ptr(thd),
                                           C.ptr(v.buf[1]), C.ptr(work), C.ptr(out), C.stream(gpu)),
                    "fem_modal_residual")
            res.append((v.buf[1][:n].cpu(), out.cpu()))
            assert v.tails_untouched()
        KX, MX = v.host[3], v.host[6]
        Rr = KX - MX * theta
        Wd, out = res[0]
        mag = KX.abs() + (MX * theta).abs()
        eW = float(((Wd - w[:, None] * Rr).abs() / (w[:, None] * mag + 1e-300)).max())
        free = w != 0
        rn, mn = out[C.MODAL_OUT_NORMS: C.MODAL_OUT_NORMS + m], out[C.MODAL_OUT_NORMS + m: C.MODAL_OUT_NORMS + 2 * m]
        eR = float(((rn - Rr[free].norm(dim=0)).abs() / mag[free].norm(dim=0)).max())
        eM = float(((mn - MX[free].norm(dim=0)).abs() / MX[free].norm(dim=0)).max())
        print(f"residual n={n} m={m}: W {eW:.2e}, ||R|| {eR:.2e}, ||MX|| {eM:.2e}")
        assert bool((Wd[~free] == 0).all())
        assert max(eW, eR, eM) <= 1e-13, (n, eW, eR, eM)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------- 3. eigenpairs
def _solve(dc, **kw):
    """The case's solve on the device -> ModalResult (the lumped case through vectorized_modal_solver)."""
    from fem355 import solver
    cs = dc.cs
    if cs.mass == "lumped":
        lam, modes, res = solver.vectorized_modal_solver(cs.Ke, cs.Me, cs.el, cs.fixed, cs.N, num_eigs=cs.k,
                                                         max_iter=kw.pop("max_iter", 2000), device=dc.dev, dtype=F64,
                                                         tol=TOL, return_info=True)
        assert lam.shape == (cs.k,) and modes.shape == (cs.n, cs.k) and modes.dtype == F64
        assert torch.equal(lam.cpu(), res.lam) and torch.equal(modes, res.X)
        return res
    return dc.A.eig_lowest(dc.Mg, cs.k, dc.w, block=cs.m, tol=TOL, **kw)


@pytest.mark.parametrize("name", list(MR.CASES))
def test_eigenpairs(devcase, name):
    from fem355 import _capi as C
    dc = devcase(name)
    cs = dc.cs
    res = _solve(dc)
    lam_d, U = cs.eig
    ref = cs.lobpcg
    assert ref[3] == MR.CONVERGED
    ref_err = cs.eig_error(ref[0])
    err = cs.eig_error(res.lam)
    X = res.X.cpu()
    rec = cs.residuals(res.lam, X)
    gram = X.T @ cs.M @ X
    orth = float((gram - torch.eye(cs.k, dtype=F64)).abs().max())
    print(f"{name}: n={cs.n} k={cs.k} m={cs.m}: {res.iterations} iterations (reference LOBPCG {ref[2]}), "
          f"{res.restarts} restarts; eigenvalue error {err:.2e} vs reference LOBPCG {ref_err:.2e} "
          f"(ratio {err / ref_err:.2f}); residuals reported {float(res.residuals.max()):.2e} recomputed "
          f"{float(rec.max()):.2e}; |X^T M X - I| {orth:.2e}")
    assert res.status == C.PCG_CONVERGED
    assert res.lam.shape == (cs.k,) and res.X.shape == (cs.n, cs.k)
    assert bool((res.lam[1:] >= res.lam[:-1]).all())
    assert float(rec.max()) <= 2 * TOL, rec
    assert orth <= 1e-10, orth
    assert bool((X[~cs.free] == 0).all())
    # Davis-Kahan: the M-sine to the dense eigenvector against rho_j / gap_j
    f = cs.free
    Lm = torch.linalg.cholesky(cs.M[f][:, f])
    Rr = ((cs.K @ X) - (cs.M @ X) * res.lam)[f]
    rho = torch.linalg.solve_triangular(Lm, Rr, upper=False).norm(dim=0)      # ||r||_{M^-1}, x M-normalised
    for j in range(cs.k):
        others = torch.cat([lam_d[:j], lam_d[j + 1:]])
        gap = float((others - res.lam[j]).abs().min())
        x, u = X[:, j], U[:, j]
        d = x - u * float(u @ (cs.M @ x))
        sine = float(torch.sqrt(d @ (cs.M @ d)) / torch.sqrt(x @ (cs.M @ x)))
        print(f"  mode {j}: lambda {float(res.lam[j]):.6e} sine {sine:.2e} bound {float(rho[j]) / gap:.2e}")
        assert sine <= float(rho[j]) / gap + 1e-10, (j, sine, float(rho[j]) / gap)
    assert err <= 8 * ref_err, (err, ref_err)


# ---------------------------------------------------------------- 4. behaviour
def test_same_seed_same_bits(devcase):
    dc = devcase("elastic4")
    a, b = _solve(dc, history=True), _solve(dc, history=True)
    assert a.iterations == b.iterations and a.restarts == b.restarts
    assert torch.equal(a.lam, b.lam) and torch.equal(a.X, b.X) and torch.equal(a.residuals, b.residuals)
    assert a.history.shape == (a.iterations, dc.cs.k) and torch.equal(a.history, b.history)
    assert torch.equal(a.history[-1], a.residuals)
    c = _solve(dc, seed=1)
    assert not torch.equal(c.X, a.X) and dc.cs.eig_error(c.lam) < 1e-9


def test_converged_start_stops_at_once(devcase):
    from fem355 import _capi as C
    dc = devcase("elastic4")
    a = _solve(dc)
    b = _solve(dc, X0=a.X)
    print(f"restart from the converged modes: {b.iterations} iterations, residuals {b.residuals}")
    assert b.status == C.PCG_CONVERGED and b.iterations == 0
    assert rel(b.lam, a.lam) < 1e-12


def test_max_iter_is_reported(devcase, capsys):
    from fem355 import _capi as C
    from fem355 import solver
    dc = devcase("lumped5")
    cs = dc.cs
    capsys.readouterr()
    lam, modes, res = solver.vectorized_modal_solver(cs.Ke, cs.Me, cs.el, cs.fixed, cs.N, num_eigs=cs.k, max_iter=3,
                                                     device=dc.dev, return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert res.status == C.PCG_MAXITER and res.iterations == 3
    assert lines == [f"Modal solver: reached max_iter (3) with residual {float(res.residuals.max()):.3e}"]
    assert lam.dtype == torch.float32 and modes.shape == (cs.n, cs.k)     # the reference's default output dtype
    assert bool(torch.isfinite(lam).all()) and float(res.residuals.max()) > TOL


def test_free_free_structure_breaks_down(devcase):
    """No clamped dof: K is singular, the lowest Ritz values fall towards zero -> PCG_BREAKDOWN, no NaN in lam."""
    from fem355 import _capi as C
    dc = devcase("elastic4", clamp=False)
    res = dc.A.eig_lowest(dc.Mg, 4, dc.w, block=8, tol=TOL)
    ref = MR.lobpcg_ref(dc.cs.K, dc.cs.M, dc.cs.w, 4, 8)
    print(f"free-free: status {res.status} after {res.iterations} iterations (reference LOBPCG: {ref[3]} after "
          f"{ref[2]}), lam {res.lam}")
    assert ref[3] == MR.BREAKDOWN
    assert res.status == C.PCG_BREAKDOWN
    assert bool(torch.isfinite(res.lam).all()) and bool(torch.isfinite(res.X).all())


def test_modal_solver_frequencies(devcase, capsys):
    import math
    from fem355 import _capi as C
    from fem355 import solver
    cs = MR.case("elastic6")
    ref_err = cs.eig_error(cs.lobpcg[0])
    capsys.readouterr()
    # the full [Me, 12, 12] mass of compute_c3d4_M_matrix: the scalar factor is taken from it
    freq, lam, modes, res = solver.modal_solver(cs.Ke, cs.Me, cs.el, cs.fixed, cs.N, num_modes=cs.k, block=cs.m,
                                                tol=TOL, device="cuda:0", return_info=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    want = torch.sqrt(cs.eig[0][: cs.k]) / (2 * math.pi)
    err = float(((freq.cpu() - want).abs() / want).max())
    print(f"modal_solver: frequencies {freq.cpu().tolist()} Hz, error {err:.2e} (bound {8 * ref_err:.2e})")
    assert res.status == C.PCG_CONVERGED
    assert freq.shape == lam.shape == (cs.k,) and modes.shape == (cs.k, cs.N, 3) and freq.dtype == F64
    assert len(lines) == cs.k and all(ln.startswith(f"Mode {j + 1}: f = ") for j, ln in enumerate(lines))
    assert torch.equal(modes.permute(1, 2, 0).reshape(cs.n, cs.k), res.X)
    assert err <= 8 * ref_err, (err, ref_err)
    # the scalar factor gives the same bits
    f2, _, _ = solver.modal_solver(cs.Ke, cs.Ms, cs.el, cs.fixed, cs.N, num_modes=cs.k, block=cs.m, tol=TOL)
    assert torch.equal(f2, freq)


def test_bad_arguments_are_refused(devcase):
    from fem355 import _capi as C
    dc = devcase("elastic4")
    lib = C.lib()
    n, m = dc.cs.n, 4
    v = Vecs(dc.dev, n, m, 1)
    work = torch.empty(int(lib.fem_modal_work_len()), dtype=F64, device=dc.dev)
    out = torch.zeros(C.MODAL_OUT_LEN, dtype=F64, device=dc.dev)
    A = dc.A
    for bs, nv, form in ((2, 4, C.MASS_SELL), (3, 3, C.MASS_SELL), (3, 4, 2)):
        rc = lib.fem_spmm_km(A.g.n_nodes, bs, nv, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols), C.ptr(A.g.dcols),
                             C.ptr(A.plain_values()), C.ptr(dc.Mg.plain_values()), form, C.ptr(v.buf[0]),
                             C.ptr(v.buf[3]), C.ptr(v.buf[6]), C.stream(dc.dev))
        assert rc == C.FEM_EARG, (bs, nv, form, rc)
    assert lib.fem_modal_gram(n, 3, 3, v.ptrs, C.ptr(work), C.ptr(out), C.stream(dc.dev)) == C.FEM_EARG
    assert lib.fem_modal_gram(n, m, 4, v.ptrs, C.ptr(work), C.ptr(out), C.stream(dc.dev)) == C.FEM_EARG
    assert lib.fem_modal_rotate(n, m, 0, v.ptrs, C.ptr(out), C.stream(dc.dev)) == C.FEM_EARG
    assert lib.fem_modal_residual(0, m, C.ptr(v.buf[3]), C.ptr(v.buf[6]), C.ptr(dc.w), C.ptr(out), C.ptr(v.buf[1]),
                                  C.ptr(work), C.ptr(out), C.stream(dc.dev)) == C.FEM_EARG
    torch.cuda.synchronize()
    assert all(torch.equal(b[:n].cpu(), h) for b, h in zip(v.buf, v.host))   # nothing was launched
