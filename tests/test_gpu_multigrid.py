"""GPU tier: the geometric multigrid PCG (csrc/multigrid.hip, system.Multigrid, the solver routes) against the
restatement of tests/multigrid_ref.py. The device matrices of every level are assembled from the oracle's element
matrices (Multigrid's `assemble` hook), so the restatement and the device sum the same numbers and differ by summation
order only; the restatement runs on the device hierarchy's own meshes and parents.

Tolerances:
  prolongation       bit-exact: 0.5 (a + b) is one rounding however it is written.
  restriction        2^-52 sum |terms| per entry; the restatement sums 0.5 r_f over each child list in list order, one
                     term per occurrence, as the kernel does, so the results are in fact equal bit for bit (asserted
                     too; the difference from the reversed-order restatement is printed). Bit-identical on a second
                     call. <P x, y> = <x, P^T y> to sum |x_c| bound_c plus one rounding per product (the sums
                     themselves are formed exactly, math.fsum).
  apply, history     100 x the spread between the restatement under ascending and reversed node numbering, floor 1e-12
                     (relative to the largest entry / per entry): the two-level tests' criterion. Spreads measured on
                     this file's cases, apply / history: 6e-16 .. 2.8e-14 / 1.2e-14 .. 3.2e-13 (the beam the largest);
                     the device's own differences on an MI355X: at most 1.0e-13 / 1.1e-13.
  solves (rtol 1e-12) iteration count within +-2 of the restatement's, u within 1e-9 of the sparse direct solve."""
import math

import pytest
import torch

import multigrid_ref as MG
from twolevel_ref import kuhn_box

pytestmark = pytest.mark.gpu
F64 = torch.float64
SPREAD_FACTOR, SPREAD_FLOOR = 100.0, 1e-12

_CASES = {}


def _mods():
    import fem355  # noqa: F401
    from fem355 import mesh, solver, system, topology
    return mesh, solver, system, topology


def _coarse(name):
    """name -> (coarse coords, tets, levels)"""
    mesh, _, _, _ = _mods()
    if name == "beam":
        return (*kuhn_box(2, 2, 6, (1.0, 1.0, 3.0), 0.15), 1)
    n, levels = {"2-4": (2, 1), "2-4-8": (2, 2), "4-8-16": (4, 2)}[name]
    return (*mesh.kuhn_cube(n, 0.15), levels)


class Case:
    """One hierarchy, kind and column format: the device hierarchy and Multigrid, the restatement both ways -- formed
    once and shared by the tests of the shape."""

    def __init__(self, name, kind, compress, gpu):
        mesh, _, system, topology = _mods()
        self.name, self.kind, self.gpu = name, kind, gpu
        self.bs = bs = 1 if kind == "poisson" else 3
        c, t, levels = _coarse(name)
        self.h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=levels)
        self.host = [(lv.coords.cpu(), lv.elements.cpu(), None if lv.parents is None else lv.parents.cpu().long())
                     for lv in self.h.levels]
        fc = self.host[-1][0]
        self.N = fc.shape[0]
        fixed = mesh.face_nodes(fc, 2, 0.0)
        self.mask = torch.zeros(self.N, dtype=torch.bool)
        self.mask[fixed] = True
        if kind == "elastic":
            top = mesh.face_nodes(fc, 2, float(fc[:, 2].max()))
            F = torch.zeros((self.N, 3), dtype=F64)
            F[top, 2] = -1e6 / top.numel()
        else:
            F = torch.ones((self.N, 1), dtype=F64)
            F[fixed] = 0.0
        self.b = F.reshape(-1)
        self.Ke = [MG.element_matrices(x, y, kind, MG.E_MOD, MG.NU) for x, y, _ in self.host]

        def assemble(l, coords, elements):
            g = system.build_graph(elements, coords.shape[0], compress=compress)
            assert (g.dcols is not None) == compress
            return system.SellMatrix(g, bs).add_element_matrices(self.Ke[l].to(gpu), elements)

        self.assemble = assemble
        self.mg = self.multigrid()
        self.ref = MG.MultigridRef(self.host, kind, fixed=self.mask, matrices=self.Ke)
        self.desc = MG.MultigridRef(self.host, kind, fixed=self.mask, matrices=self.Ke, descending=True)
        self.r = torch.randn(bs * self.N, dtype=F64, generator=torch.Generator().manual_seed(11))

    def multigrid(self, **kw):
        _, _, system, _ = _mods()
        return system.Multigrid(self.h, self.kind, MG.E_MOD, MG.NU, self.mask.to(self.gpu), assemble=self.assemble,
                                **kw)


SHAPES = [("2-4", "elastic", True), ("2-4", "poisson", False), ("beam", "elastic", False), ("2-4-8", "elastic", False),
          ("2-4-8", "poisson", True), ("4-8-16", "elastic", True), ("4-8-16", "poisson", False)]


@pytest.fixture(params=SHAPES, ids=[f"{n}-{k}-{'d16' if c else 'i32'}" for n, k, c in SHAPES])
def case(request, gpu):
    key = request.param
    if key not in _CASES:
        _CASES[key] = Case(*key, gpu)
    return _CASES[key]


def test_levels_and_lmax_vs_restatement(case):
    mg, ref = case.mg, case.ref
    info = mg.levels_info()
    assert [i["nodes"] for i in info] == ref.N
    assert set(mg.times) == {"assemble", "eig", "coarse"}
    for l in range(1, len(ref.N)):
        assert torch.equal(mg.masks[l].cpu(), ref.masks[l])
        assert abs(info[l]["lmax"] - ref.lmax[l]) <= 1e-10 * ref.lmax[l], (l, info[l]["lmax"], ref.lmax[l])
        assert info[l]["free_dofs"] == int(ref.free[l].sum())


def test_prolongation_is_bit_exact(case):
    mg, ref = case.mg, case.ref
    for l in range(1, len(ref.N)):
        g = torch.Generator().manual_seed(100 + l)
        xc = torch.randn(case.bs * ref.N[l - 1], dtype=F64, generator=g)
        xf = torch.randn(case.bs * ref.N[l], dtype=F64, generator=g)
        assert torch.equal(mg.prolong(l, xc.to(case.gpu)).cpu(), ref.prolong(l, xc))
        assert torch.equal(mg.prolong(l, xc.to(case.gpu), xf.to(case.gpu)).cpu(), ref.prolong(l, xc, xf))


def test_restriction_vs_restatement_and_adjointness(case):
    mg, ref = case.mg, case.ref
    for l in range(1, len(ref.N)):
        g = torch.Generator().manual_seed(200 + l)
        y = torch.randn(case.bs * ref.N[l], dtype=F64, generator=g)
        x = torch.randn(case.bs * ref.N[l - 1], dtype=F64, generator=g)
        rc = mg.restrict(l, y.to(case.gpu))
        err, bound = (rc.cpu() - ref.restrict(l, y)).abs(), ref.restrict_bound(l, y)
        derr = (rc.cpu() - case.desc.restrict(l, y)).abs()
        print(f"{case.name} level {l}: restrict max err / (2^-52 sum|terms|) {float((err / bound.clamp(min=1e-300)).max()):.3e}"
              f", against the reversed order {float((derr / bound.clamp(min=1e-300)).max()):.3e}")
        assert bool((err <= bound).all())
        assert torch.equal(rc.cpu(), ref.restrict(l, y))   # the same sum in the same order
        assert torch.equal(mg.restrict(l, y.to(case.gpu)), rc)
        Px = mg.prolong(l, x.to(case.gpu)).cpu()
        lhs = math.fsum((Px * y).tolist())
        rhs = math.fsum((x * rc.cpu()).tolist())
        allowed = float((x.abs() * bound).sum()) + MG.EPS * float((Px * y).abs().sum() + (x * rc.cpu()).abs().sum())
        print(f"{case.name} level {l}: <Px, y> - <x, P^T y> = {lhs - rhs:.3e}, allowed {allowed:.3e}")
        assert abs(lhs - rhs) <= allowed


def _spread(a, b, per_entry=False):
    d = (a - b).abs()
    return float((d / a.abs()).max()) if per_entry else float(d.max() / a.abs().max())


def test_apply_and_history_vs_restatement(case):
    mg, ref, desc = case.mg, case.ref, case.desc
    za = ref.apply(case.r)
    spread = _spread(za, desc.apply(case.r))
    tol = max(SPREAD_FACTOR * spread, SPREAD_FLOOR)
    z = mg.apply(case.r.to(case.gpu))
    err = _spread(za, z.cpu())
    print(f"{case.name} {case.kind}: apply spread {spread:.3e} tol {tol:.3e} err {err:.3e}")
    assert err <= tol
    assert torch.equal(mg.apply(case.r.to(case.gpu)), z)
    assert bool((z.cpu().view(-1, case.bs)[case.mask] == 0).all())
    _, _, ha, _ = ref.pcg(case.b, tol=0.0, max_iter=20)
    _, _, hd, _ = desc.pcg(case.b, tol=0.0, max_iter=20)
    spread = _spread(ha, hd, per_entry=True)
    tol = max(SPREAD_FACTOR * spread, SPREAD_FLOOR)
    res = mg.pcg(case.b.to(case.gpu), tol=0.0, max_iter=20, history=True)
    assert res.iterations == 20 and res.history.numel() == 20
    err = _spread(ha, res.history.cpu(), per_entry=True)
    print(f"{case.name} {case.kind}: history spread {spread:.3e} tol {tol:.3e} err {err:.3e}")
    assert err <= tol
    res2 = mg.pcg(case.b.to(case.gpu), tol=0.0, max_iter=20, history=True, chunk=7)
    assert torch.equal(res2.history, res.history) and torch.equal(res2.x, res.x)


def test_solve_vs_direct(case):
    from fem355 import _capi as C
    mg, ref = case.mg, case.ref
    bd = case.b.to(case.gpu)
    tol = 1e-12 * float(torch.sqrt(torch.dot(bd, mg.apply(bd))))
    res = mg.pcg(bd, tol=tol, max_iter=500)
    _, it_ref, _, status = ref.pcg(case.b, rtol=1e-12, max_iter=500)
    u, ud = res.x.cpu(), ref.direct(case.b)
    uerr = float((u - ud).abs().max() / ud.abs().max())
    print(f"{case.name} {case.kind}: iterations {res.iterations} vs {it_ref}, u err {uerr:.3e}")
    assert res.status == C.PCG_CONVERGED and status == "converged"
    assert abs(res.iterations - it_ref) <= 2
    assert uerr <= 1e-9
    assert bool((u.view(-1, case.bs)[case.mask] == 0).all())


def test_negated_matrix_breaks_down_at_iteration_one(gpu):
    """The fine matrix's values negated after the setup: p.Ap < 0 (or r0.z0 < 0) stops the first iteration with
    PCG_BREAKDOWN and x is the start vector, bit for bit."""
    from fem355 import _capi as C
    key = ("2-4", "elastic", True)
    if key not in _CASES:
        _CASES[key] = Case(*key, gpu)
    case = _CASES[key]
    mg = case.multigrid()
    mg.fine.vals.neg_()
    x0 = torch.randn(case.b.numel(), dtype=F64, generator=torch.Generator().manual_seed(3)).to(gpu)
    x0.view(-1, 3)[case.mask.to(gpu)] = 0.0
    for start in (None, x0):
        res = mg.pcg(case.b.to(gpu), start, tol=1e-8, max_iter=50, history=True)
        assert res.status == C.PCG_BREAKDOWN and res.iterations == 1
        assert torch.equal(res.x, torch.zeros_like(x0) if start is None else x0)
    mg.close()


def test_zero_right_hand_side_converges_at_once(gpu):
    """b = 0 from x = 0: r0.z0 = 0, nothing to iterate on -- PCG_CONVERGED with 0 iterations and x untouched, as the
    restatement says (not a breakdown on p.Ap = 0)."""
    from fem355 import _capi as C
    key = ("2-4", "poisson", False)
    if key not in _CASES:
        _CASES[key] = Case(*key, gpu)
    case = _CASES[key]
    zero = torch.zeros_like(case.b)
    res = case.mg.pcg(zero.to(gpu), tol=1e-8, max_iter=50, history=True)
    x, it, hist, status = case.ref.pcg(zero, tol=1e-8, max_iter=50)
    assert res.status == C.PCG_CONVERGED and status == "converged"
    assert res.iterations == it == 0 and res.history.numel() == 0
    assert float(res.x.abs().max()) == 0.0 and res.rz == 0.0
    after = case.mg.pcg(case.b.to(gpu), tol=0.0, max_iter=3, history=True)   # the context is fine afterwards
    assert after.iterations == 3 and bool(torch.isfinite(after.history).all())


def test_solve_tet4_routes(gpu):
    """The default kwarg is today's path bit for bit; "multigrid" reaches the same solution in far fewer iterations;
    the clamp of the coarse mesh reaches the fine one through carry()."""
    mesh, solver, system, topology = _mods()
    c, t = mesh.kuhn_cube(4, 0.15)
    h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=1)
    fc, fe = h.fine
    F, fixed = mesh.cube_elasticity_case(fc)
    assert torch.equal(h.carry(mesh.face_nodes(c, 2, 0.0)), fixed)
    kw = dict(kind="elastic", E=MG.E_MOD, nu=MG.NU, rtol=1e-10, device=gpu)
    u0, r0, _ = solver.solve_tet4(fc, fe, F, fixed, **kw)
    u1, r1, _ = solver.solve_tet4(fc, fe, F, fixed, preconditioner="jacobi", hierarchy=None, **kw)
    assert torch.equal(u0, u1) and r0.iterations == r1.iterations
    u2, r2, A2 = solver.solve_tet4(fc, fe, F, fixed, preconditioner="multigrid", hierarchy=h, **kw)
    assert isinstance(r2.multigrid, system.Multigrid) and A2 is r2.multigrid.fine
    assert 4 * r2.iterations < r0.iterations
    assert float((u2 - u0).abs().max() / u0.abs().max()) < 1e-7
    u3, r3 = solver.multigrid_pcg_solver(h, F, fixed, E=MG.E_MOD, nu=MG.NU, rtol=1e-10, return_info=True)
    assert torch.equal(u3, u2) and r3.iterations == r2.iterations
    f1, fx1 = mesh.cube_poisson_case(fc)
    u4, r4, _ = solver.solve_tet4(fc, fe, f1, fx1, kind="poisson", preconditioner="multigrid", hierarchy=h, rtol=1e-10,
                                  device=gpu, mg_degree=3)
    u5, r5, _ = solver.solve_tet4(fc, fe, f1, fx1, kind="poisson", rtol=1e-10, device=gpu)
    assert r4.multigrid.degree == 3 and 4 * r4.iterations < r5.iterations
    assert float((u4 - u5).abs().max() / u5.abs().max()) < 1e-7


def test_out_of_scope_combinations_raise(gpu):
    mesh, solver, system, topology = _mods()
    c, t = mesh.kuhn_cube(2, 0.15)
    h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=1)
    fc, fe = h.fine
    F, fixed = mesh.cube_elasticity_case(fc)
    kw = dict(kind="elastic", E=MG.E_MOD, nu=MG.NU, device=gpu, preconditioner="multigrid")
    with pytest.raises(ValueError, match="matrix-free"):
        solver.solve_tet4(fc, fe, F, fixed, hierarchy=h, operator="matfree", **kw)
    with pytest.raises(ValueError, match="modulus_scale"):
        solver.solve_tet4(fc, fe, F, fixed, hierarchy=h,
                          modulus_scale=torch.ones(fe.shape[0], dtype=F64, device=gpu), **kw)
    with pytest.raises(ValueError, match="reorder"):
        solver.solve_tet4(fc, fe, F, fixed, hierarchy=h, reorder="rcm", **kw)
    with pytest.raises(ValueError, match="hierarchy"):
        solver.solve_tet4(fc, fe, F, fixed, **kw)
    with pytest.raises(ValueError, match="hierarchy"):
        solver.solve_tet4(fc, fe, F, fixed, kind="elastic", device=gpu, hierarchy=h)
    with pytest.raises(ValueError, match="kind"):
        solver.solve_tet4(fc, fe, F, fixed, hierarchy=h, **{**kw, "kind": "shell"})
    with pytest.raises(ValueError, match="hierarchy.fine"):   # the coarse mesh is not the hierarchy's finest
        Fc, fxc = mesh.cube_elasticity_case(c)
        solver.solve_tet4(c, t, Fc, fxc, hierarchy=h, **kw)
    with pytest.raises(ValueError, match="hierarchy.fine"):   # same shapes, another mesh
        solver.solve_tet4(fc + 1e-3, fe, F, fixed, hierarchy=h, **kw)
    # the C entry points refuse other block sizes themselves (FEM_EARG)
    from fem355 import _capi as C
    z = torch.zeros(8, dtype=F64, device=gpu)
    zi = torch.zeros(8, dtype=torch.int32, device=gpu)
    rc = C.lib().fem_mg_restrict(2, 2, 2, C.ptr(zi), C.ptr(zi), C.ptr(z), C.ptr(z), C.ptr(z),
                                 C.stream(torch.device(gpu)))
    assert rc == C.FEM_EARG


def test_coarse_cap_is_checked_before_assembly(gpu, monkeypatch):
    """11^3 nodes, one face clamped: 3630 free dofs on level 0 > 3072. The error names the cap and the way out, and
    comes before any level is assembled."""
    mesh, _, system, topology = _mods()
    c, t = mesh.kuhn_cube(10)
    h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=1, reorder=None)
    mask = torch.zeros(h.levels[-1].n_nodes, dtype=torch.bool, device=gpu)
    mask[mesh.face_nodes(h.fine[0], 2, 0.0)] = True

    def no_assembly(*a, **k):
        raise AssertionError("a level was assembled before the cap was checked")

    monkeypatch.setattr(system, "assemble_tet4_system", no_assembly)
    with pytest.raises(ValueError, match="3072.*start from a coarser mesh or add a level"):
        system.Multigrid(h, "elastic", MG.E_MOD, MG.NU, mask)
