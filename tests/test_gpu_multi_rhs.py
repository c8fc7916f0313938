"""Multi-load-case (P)CG on the device (csrc/pcg_multi.hip): SellMatrix.matvec_multi / pcg_multi and the public
multi-load solvers against the CPU oracle and against the single-right-hand-side path.

Mesh: mesh.kuhn_cube(n, jitter=0.15), E = 113.8e9, nu = 0.342, z = 0 face fixed, exact Jacobi with fixed rows zeroed.
Load columns on the z = 1 face: z (cube_elasticity_case), x shear, torsion, a point load, and z * 1e-3.
Tolerances: 1e-12 operator parity (the project's operator tolerance), 1e-10 iterate parity (at
rtol = 1e-12 the oracle's own iterate moves <= 3.5e-13 when stopped two iterations earlier or later), 1e-12 against the
single-vector three-kernel schedule (what the schedule-vs-schedule tests use), 1e-14 per column against matvec
(same summation order, FMA contraction only)."""
import ctypes

import pytest
import torch

from conftest import rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

E, NU = 113.8e9, 0.342
F64 = torch.float64
LS = (1, 2, 3, 4, 5, 8, 11)


def _loads(c):
    """{name: F [N, 3]} of the five load columns."""
    from fem355 import mesh
    N = c.shape[0]
    top = mesh.face_nodes(c, 2, 1.0)
    z = mesh.cube_elasticity_case(c)[0]
    x = torch.zeros((N, 3), dtype=F64)
    x[top, 0] = 1e6 / top.numel()
    tors = torch.zeros((N, 3), dtype=F64)
    tors[top, 0] = -(c[top, 1] - 0.5) * 1e5
    tors[top, 1] = (c[top, 0] - 0.5) * 1e5
    point = torch.zeros((N, 3), dtype=F64)
    point[N - 1, 1] = 1e3
    return {"z": z, "x": x, "tors": tors, "point": point, "zs": z * 1e-3}


class Case:
    """One mesh with its oracle element matrices, Jacobi, loads and device operator; oracle solves are memoised."""

    def __init__(self, dev, n, kind):
        from fem355 import mesh, system
        self.dev, self.kind = dev, kind
        self.dpn = 3 if kind == "elastic" else 1
        self.c, self.t = mesh.kuhn_cube(n, jitter=0.15)
        self.N = self.c.shape[0]
        self.n = self.N * self.dpn
        self.K = R.tet4_K(self.c, self.t, E, NU) if kind == "elastic" else R.tet4_poisson_K(self.c, self.t)
        self.fixed = mesh.face_nodes(self.c, 2, 0.0)
        self.dinv = R.diag_preconditioner(self.K, self.t, self.N, dpn=self.dpn)
        self.dinv[self.fixed] = 0.0
        self.free = torch.ones((self.N, self.dpn), dtype=F64)
        self.free[self.fixed] = 0.0
        if kind == "elastic":
            self.loads = _loads(self.c)
        else:   # scalar sources: the bench's unit source, a graded one, two seeded random ones
            g = torch.Generator().manual_seed(11)
            f = mesh.cube_poisson_case(self.c)[0]
            self.loads = {"one": f, "graded": f * self.c[:, :1],
                          "r0": torch.randn(self.N, 1, dtype=F64, generator=g),
                          "r1": torch.randn(self.N, 1, dtype=F64, generator=g)}
        self.A = system.assemble_tet4_system(self.c.to(dev), self.t.to(dev), kind, E if kind == "elastic" else 1.0,
                                             NU if kind == "elastic" else 0.0)
        self._memo = {}

    def B(self, names):
        """[n, L] device multi-vector of the named loads (a tensor instead of a name is taken as it is)."""
        cols = [(self.loads[k] if isinstance(k, str) else k).reshape(-1) for k in names]
        return torch.stack(cols, dim=1).to(self.dev)

    def w(self, pcg):
        return (self.dinv if pcg else self.free).reshape(-1).to(self.dev)

    def r0norm(self, name, pcg):
        """sqrt(r0.z0) (PCG) resp. sqrt(r0.r0) (CG, fixed rows zeroed) from x0 = 0."""
        F = self.loads[name]
        return float(torch.sqrt(torch.sum(F * self.dinv * F))) if pcg else float(torch.sqrt(torch.sum((F * self.free) ** 2)))

    def oracle(self, name, pcg, tol, max_iter=1000):
        """(u [n], iterations, status, history) of the oracle's solve of one load column."""
        key = (name, pcg, tol, max_iter)
        if key not in self._memo:
            hist = []
            F = self.loads[name]
            if pcg:
                u, it, st = R.pcg(self.K, self.t, F, self.dinv, tol=tol, max_iter=max_iter, history=hist)
            else:
                u, it, st = R.stable_cg(self.K, self.t, F, self.fixed, tol=tol, max_iter=max_iter, history=hist)
            self._memo[key] = (u.reshape(-1), it, st, torch.tensor(hist, dtype=F64))
        return self._memo[key]


_CASES = {}


@pytest.fixture(scope="module")
def case(gpu):
    def get(n, kind):
        if (n, kind) not in _CASES:
            _CASES[(n, kind)] = Case(gpu, n, kind)
        return _CASES[(n, kind)]
    yield get
    _CASES.clear()


def _check_operator(A, K, t, N, dpn, seed):
    """matvec_multi against the oracle's EBE product per column, and against matvec, for every L of LS."""
    n = N * dpn
    X = torch.randn(n, max(LS), dtype=F64, generator=torch.Generator().manual_seed(seed))
    ref = torch.stack([R.nodal_forces(K, t, X[:, j].reshape(N, dpn)).reshape(-1) for j in range(max(LS))], dim=1)
    Xd = X.to(A.device)
    single = torch.stack([A.matvec(Xd[:, j].contiguous()) for j in range(max(LS))], dim=1)
    # bs = 3 takes 4 columns per pass by default: the 8-column kernels are checked through max_cols = 8 as well
    for L, wide in [(L, None) for L in LS] + ([(L, 8) for L in LS if L > 4] if dpn == 3 else []):
        Y = A.matvec_multi(Xd[:, :L], max_cols=wide)
        assert Y.shape == (n, L) and Y.dtype == F64
        for j in range(L):
            e = rel(Y[:, j], ref[:, j])
            print(f"L={L} max_cols={wide} col {j}: vs oracle {e:.2e}, vs matvec {rel(Y[:, j], single[:, j]):.2e}")
            assert e < 1e-12, (L, wide, j, e)
            assert rel(Y[:, j], single[:, j]) < 1e-14, (L, wide, j)


# ---------------------------------------------------------------- 1. operator vs oracle
@pytest.mark.parametrize("kind,n", [("elastic", 4), ("elastic", 12), ("poisson", 4), ("poisson", 12)])
def test_matvec_multi_tets(case, kind, n):
    cs = case(n, kind)
    if n == 4:
        assert cs.N == 125   # two slices, the second with 61 rows
    _check_operator(cs.A, cs.K, cs.t, cs.N, cs.dpn, 100 + n)


def test_matvec_multi_hexes(gpu):
    """bs = 3 hexes: wide rows (up to 27 blocks)."""
    from fem355 import mesh, solver
    c, h = mesh.hex_box(5)
    K = R.iso_K(c, h, "c3d8", E, NU)
    A = solver.assemble(K, h, c.shape[0], gpu)
    _check_operator(A, K, h, c.shape[0], 3, 7)


# ---------------------------------------------------------------- 2. int32 columns
def test_matvec_multi_int32_columns(gpu):
    from fem355 import mesh, system
    c, t = mesh.kuhn_cube(32)
    N = c.shape[0]
    assert N == 35937
    p = torch.randperm(N, generator=torch.Generator().manual_seed(5))   # old node i becomes node p[i]
    c2 = torch.empty_like(c)
    c2[p] = c
    t2 = p[t]
    A = system.assemble_tet4_system(c2.to(gpu), t2.to(gpu), "poisson", 1.0, 0.0)
    assert A.g.dcols is None
    K = R.tet4_poisson_K(c2, t2)
    X = torch.randn(N, 4, dtype=F64, generator=torch.Generator().manual_seed(6))
    Y = A.matvec_multi(X.to(gpu))
    for j in range(4):
        e = rel(Y[:, j], R.nodal_forces(K, t2, X[:, j:j + 1]).reshape(-1))
        print(f"int32 columns, col {j}: {e:.2e}")
        assert e < 1e-12, (j, e)


# ---------------------------------------------------------------- 3. fixed iterations
@pytest.mark.parametrize("pcg", [True, False], ids=["pcg", "cg"])
@pytest.mark.parametrize("kind,n", [("poisson", 4), ("poisson", 12), ("elastic", 4), ("elastic", 12)])
def test_fixed_iterations(case, kind, n, pcg):
    from fem355 import _capi as C
    cs = case(n, kind)
    names = ["z", "x", "tors", "point"] if kind == "elastic" else ["one", "graded", "r0", "r1"]
    mode = C.MODE_PCG if pcg else C.MODE_CG_STABLE
    B = cs.B(names)
    res = cs.A.pcg_multi(B, w=cs.w(pcg), mode=mode, tol=0.0, max_iter=25, history=True)
    assert res.status == [C.PCG_MAXITER] * 4 and res.iterations == [25] * 4
    assert res.history.shape == (25, 4)
    for j, name in enumerate(names):
        u, it, st, hist = cs.oracle(name, pcg, 0.0, 25)
        assert it == 25 and st == "max_iter"
        single = cs.A.pcg(B[:, j].contiguous(), w=cs.w(pcg), mode=mode, tol=0.0, max_iter=25, schedule=0)
        eo, es, eh = rel(res.x[:, j], u), rel(res.x[:, j], single.x), rel(res.history[:20, j], hist[:20])
        print(f"{kind} n={n} {'pcg' if pcg else 'cg'} {name}: oracle {eo:.2e} single {es:.2e} history {eh:.2e}")
        assert eo < 1e-10, (name, eo)
        assert es < 1e-12, (name, es)
        assert eh < 1e-10, (name, eh)


# ---------------------------------------------------------------- 4. to tolerance
FIVE = ["z", "x", "tors", "point", "zs"]


@pytest.mark.parametrize("pcg", [True, False], ids=["pcg", "cg"])
@pytest.mark.parametrize("n", [4, 6])
def test_to_tolerance(case, n, pcg):
    from fem355 import _capi as C
    cs = case(n, "elastic")
    tols = [1e-12 * cs.r0norm(k, pcg) for k in FIVE]
    for wide in (None, 8):   # the default passes of 4 + 1 columns, and all five in one 8-column pass
        res = cs.A.pcg_multi(cs.B(FIVE), w=cs.w(pcg), mode=C.MODE_PCG if pcg else C.MODE_CG_STABLE, tol=tols,
                             max_iter=1000, max_cols=wide)
        assert res.status == [C.PCG_CONVERGED] * 5, res.status
        for j, name in enumerate(FIVE):
            u, it, st, _ = cs.oracle(name, pcg, tols[j])
            e = rel(res.x[:, j], u)
            print(f"n={n} {'pcg' if pcg else 'cg'} max_cols={wide} {name}: {res.iterations[j]} iterations "
                  f"(oracle {it}), rel {e:.2e}")
            assert st == "converged"
            assert abs(res.iterations[j] - it) <= 2, (name, res.iterations[j], it)
            assert e < 1e-10, (name, e)


# ---------------------------------------------------------------- 5. columns stop at different times, stay frozen
def test_columns_stop_apart_and_stay_frozen(case):
    from fem355 import _capi as C
    cs = case(4, "elastic")
    B, w = cs.B(FIVE), cs.w(True)
    # all five columns in ONE 8-column pass, so the column that stops first shares its launches with running ones
    res = cs.A.pcg_multi(B, w=w, tol=1e-6, max_iter=1000, max_cols=8)
    its = [cs.oracle(k, True, 1e-6)[1] for k in FIVE]
    print("iterations", res.iterations, "oracle", its)
    assert res.status == [C.PCG_CONVERGED] * 5
    assert all(abs(a - b) <= 2 for a, b in zip(res.iterations, its)), (res.iterations, its)
    assert len(set(its)) > 1 and max(its) - min(its) > 10   # the case does make them stop apart
    first = min(range(5), key=lambda j: res.iterations[j])
    short = cs.A.pcg_multi(B, w=w, tol=1e-6, max_iter=res.iterations[first], max_cols=8)
    assert short.iterations[first] == res.iterations[first]
    assert torch.equal(short.x[:, first], res.x[:, first])   # later iterations did not touch the frozen column


# ---------------------------------------------------------------- 6. a bad column does not poison the others
def test_bad_column_is_contained(case):
    from fem355 import _capi as C
    cs = case(4, "elastic")
    w = cs.w(False)
    zero = torch.zeros((cs.N, 3), dtype=F64)
    tols = [1e-10 * cs.r0norm("z", False), 1e-10 * cs.r0norm("tors", False), 1e-10 * cs.r0norm("x", False)]
    bad = cs.A.pcg_multi(cs.B(["z", zero, "x"]), w=w, mode=C.MODE_CG_STABLE, tol=tols, max_iter=1000)
    good = cs.A.pcg_multi(cs.B(["z", "tors", "x"]), w=w, mode=C.MODE_CG_STABLE, tol=tols, max_iter=1000)
    _, it, st = R.stable_cg(cs.K, cs.t, zero, cs.fixed, tol=tols[1])
    assert (it, st) == (1, "breakdown_pAp")
    assert bad.status[1] == C.PCG_BREAKDOWN and bad.iterations[1] == 1
    assert torch.equal(bad.x[:, 1], torch.zeros(cs.n, dtype=F64, device=bad.x.device))
    assert good.status == [C.PCG_CONVERGED] * 3
    for j in (0, 2):
        assert bad.status[j] == C.PCG_CONVERGED and bad.iterations[j] == good.iterations[j]
        assert torch.equal(bad.x[:, j], good.x[:, j])
    assert bool(torch.isfinite(bad.x).all())


# ---------------------------------------------------------------- 7. reproducibility and independence
def test_reproducible_and_independent(case):
    cs = case(4, "elastic")
    w = cs.w(True)
    B = cs.B(["z", "x", "tors", "point"])
    a = cs.A.pcg_multi(B, w=w, tol=1e-6, history=True)
    b = cs.A.pcg_multi(B, w=w, tol=1e-6, history=True)
    assert torch.equal(a.x, b.x) and a.iterations == b.iterations and a.rz == b.rz and a.pq == b.pq
    assert torch.equal(torch.nan_to_num(a.history), torch.nan_to_num(b.history))
    rnd = torch.randn(cs.N, 3, dtype=F64, generator=torch.Generator().manual_seed(3))
    other = cs.A.pcg_multi(cs.B(["z", 5.0 * cs.loads["point"], rnd, "x"]), w=w, tol=1e-6)
    assert other.iterations[0] == a.iterations[0] and other.rz[0] == a.rz[0]
    assert torch.equal(other.x[:, 0], a.x[:, 0])


# ---------------------------------------------------------------- 8. public API
def _lines(capsys):
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]


def _message(fn, *args):
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*args)
    return buf.getvalue().rstrip("\n")


def test_public_pcg_solver(case, capsys):
    from fem355 import solver
    cs = case(4, "elastic")
    names = ["z", "x", "tors"]
    F = torch.stack([cs.loads[k] for k in names])
    tols = [1e-12 * cs.r0norm(k, True) for k in names]
    capsys.readouterr()
    u, res = solver.multi_load_pcg_solver(cs.K, cs.t, F, cs.dinv, tol=tols, device=cs.dev, dtype=F64,
                                          return_info=True)
    lines = _lines(capsys)
    assert u.shape == (3, cs.N, 3) and u.dtype == F64
    assert lines == [f"Load case {j}: " + _message(solver._pcg_messages, res.column(j)) for j in range(3)]
    assert lines[0] == f"Load case 0: Converged after {res.iterations[0]} iterations."
    for j in range(3):
        us, rs = solver.preconditioned_conjugate_gradient_solver(cs.K, cs.t, F[j], cs.dinv, tol=tols[j],
                                                                 device=cs.dev, dtype=F64, return_info=True)
        assert rel(u[j], us) < 1e-10 and abs(rs.iterations - res.iterations[j]) <= 2
    u32 = solver.multi_load_pcg_solver(cs.K, cs.t, F, cs.dinv, tol=tols, device=cs.dev)
    assert u32.shape == (3, cs.N, 3) and u32.dtype == torch.float32   # the single solver's default output dtype
    assert rel(u32, u) < 1e-6


def test_public_cg_solver(case, capsys):
    from fem355 import solver
    cs = case(4, "elastic")
    names = ["z", "x", "tors"]
    F = torch.stack([cs.loads[k] for k in names])
    tols = [1e-12 * cs.r0norm(k, False) for k in names]
    capsys.readouterr()
    u, res = solver.multi_load_cg_solver(cs.K, cs.t, F, cs.fixed, tol=tols, device=cs.dev, return_info=True)
    lines = _lines(capsys)
    assert u.shape == (3, cs.N, 3) and u.dtype == F64
    assert lines == [f"Load case {j}: " + _message(solver._cg_messages, res.column(j), "stable") for j in range(3)]
    assert lines[1] == (f"Load case 1: Converged after {res.iterations[1]} iterations. "
                        f"Residual norm: {res.rz[1]:.3e}")
    for j in range(3):
        us, rs = solver.stable_conjugate_gradient_solver(cs.K, cs.t, F[j], cs.fixed, tol=tols[j], device=cs.dev,
                                                         return_info=True)
        assert rel(u[j], us) < 1e-10 and abs(rs.iterations - res.iterations[j]) <= 2


def test_public_solve_tet4_multi(case):
    from fem355 import solver, system
    cs = case(4, "elastic")
    names = ["z", "x", "tors"]
    f = torch.stack([cs.loads[k] for k in names])
    u, res, A = solver.solve_tet4_multi(cs.c, cs.t, f, cs.fixed, kind="elastic", E=E, nu=NU, rtol=1e-12,
                                        device=cs.dev)
    assert u.shape == (3, cs.N, 3) and u.dtype == F64
    assert isinstance(res, system.MultiPcgResult) and isinstance(A, system.SellMatrix)
    for j in range(3):
        us, rs, _ = solver.solve_tet4(cs.c, cs.t, f[j], cs.fixed, kind="elastic", E=E, nu=NU, rtol=1e-12,
                                      device=cs.dev)
        assert rel(u[j], us) < 1e-10 and abs(rs.iterations - res.iterations[j]) <= 2
        assert rel(u[j], cs.oracle(names[j], True, 1e-12 * cs.r0norm(names[j], True))[0].reshape(cs.N, 3)) < 1e-10


# ---------------------------------------------------------------- 9. errors
def test_bad_arguments_are_refused(case):
    from fem355 import _capi as C
    cs = case(4, "elastic")
    A, lib = cs.A, C.lib()
    w = cs.w(True)
    with pytest.raises(C.FemError):
        A.pcg_multi(cs.B(["z", "x"]), w=w, mode=C.MODE_CG_CONSTRAINED)
    Bp = torch.ones((cs.n, 8), dtype=F64, device=cs.dev)
    Xp = torch.zeros((cs.n, 8), dtype=F64, device=cs.dev)
    tol = (ctypes.c_double * 16)(*([1e-8] * 16))

    def create(bs, nv, nactive, mode):
        h = ctypes.c_void_p()
        rc = lib.fem_mpcg_create(A.g.n_nodes, bs, nv, nactive, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols),
                                 C.ptr(A.g.dcols), C.ptr(A.plain_values()), C.ptr(Bp), C.ptr(Xp), C.ptr(w), mode, tol,
                                 1e-30, None, 0, C.stream(A.device), ctypes.byref(h))
        if rc == C.FEM_OK:
            lib.fem_mpcg_destroy(h)
        return rc

    assert create(3, 8, 8, C.MODE_PCG) == C.FEM_OK
    for bs, nv, nactive, mode in ((3, 8, 8, C.MODE_CG_CONSTRAINED), (3, 0, 0, C.MODE_PCG), (3, 9, 9, C.MODE_PCG),
                                  (2, 8, 8, C.MODE_PCG), (3, 8, 0, C.MODE_PCG), (3, 4, 5, C.MODE_PCG)):
        rc = create(bs, nv, nactive, mode)
        assert rc == C.FEM_EARG, (bs, nv, nactive, mode, rc)
        with pytest.raises(C.FemError):
            C.check(rc, "fem_mpcg_create")
    for bs, nv in ((3, 0), (3, 9), (2, 8)):
        rc = lib.fem_spmm(A.g.n_nodes, bs, nv, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols), C.ptr(A.g.dcols),
                          C.ptr(A.plain_values()), C.ptr(Bp), C.ptr(Xp), C.stream(A.device))
        assert rc == C.FEM_EARG, (bs, nv, rc)
    torch.cuda.synchronize()
    assert not bool(Xp.any())   # nothing was launched
