"""GPU tier: the two-level PCG (csrc/pcg_coarse.hip, SellMatrix.rigid_coarse_space / pcg_two_level, the solver routes)
against the dense restatement of tests/twolevel_ref.py. The device matrices are assembled from the oracle's element
matrices, so the restatement and the device sum the same numbers and differ by summation order only.

Tolerances:
  restrict, E        terms 2^-52 sum |terms| per entry, computed by the restatement (element contributions to A_ij
                     counted as terms); E - E^T to the same bound; both bit-identical on a second run.
  apply, history     100 x the spread between the restatement evaluated with the aggregates' node lists ascending and
                     descending, floor 1e-12 (relative to the largest entry / per entry). Spreads measured (with the
                     device's Jacobi weights, this file's cases), apply / history: beam k = 6 1.7e-13 / 1.8e-12, with the
                     2-node aggregate 3.5e-13 / 2.8e-12; 6-cube k = 1 1.5e-15 / 1.5e-15, k = 5 4.7e-15 / 5.7e-15, k = 8
                     7.3e-15 / 5.7e-15, explicit ids 4.5e-16 / 1.4e-14; 12-cube k = 27 1.0e-14 / 2.8e-15 -- so the floor
                     decides nearly everywhere but on the beam. The device's own differences on an MI355X: beam 5.8e-14
                     / 1.4e-12, the cubes at most 7.0e-15 / 8.6e-15.
  solves (rtol 1e-12) iteration count within +-2 of the restatement's, u within 1e-9 of the dense direct solve, and the
                     masked true residual within what the tolerance reached allows: the recurrence's r has
                     ||r||_2 <= sqrt(r.z) / sqrt(min free w) < tol / sqrt(min free w) because M^-1 - diag(w) is positive
                     semidefinite, and the true residual differs from it by at most 2^-52 iterations || |A||x| + |b| ||_2
                     (the rounding of the x and r updates, first order)."""
import pytest
import torch

import twolevel_ref as TL
from conftest import load_golden
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
SPREAD_FACTOR, SPREAD_FLOOR = 100.0, 1e-12

_CASES = {}


def _mods():
    import fem355  # noqa: F401
    from fem355 import mesh, solver, system
    return mesh, solver, system


def _cube(n):
    mesh, _, _ = _mods()
    c, t = mesh.kuhn_cube(n, 0.15)
    F, fixed = mesh.cube_elasticity_case(c)
    return c, t, F, fixed


def _geometry(name):
    """name -> (coords, tets, F, fixed, n_aggregates, explicit ids or None)"""
    if name.startswith("beam"):
        c, t, F, fixed = TL.beam_case()
        return c, t, F, fixed, 6
    n, k = {"cube6_k1": (6, 1), "cube6_k5": (6, 5), "cube6_k8": (6, 8), "cube12_k27": (12, 27),
            "cube6_ids": (6, 2)}[name]
    return (*_cube(n), k)


class Case:
    """One shape: the oracle's element matrices, the device matrix and coarse space, the restatement both ways --
    formed once and shared by the tests of the shape."""

    def __init__(self, name, gpu, compress):
        _, _, system = _mods()
        self.name = name
        c, t, F, fixed, k = _geometry(name)
        self.coords, self.F, self.N = c, F, c.shape[0]
        Ke = R.tet4_K(c, t, TL.E_MOD, TL.NU)
        A, Aabs, Cnt = TL.dense_matrix([(Ke, t)], self.N)
        el = t.to(gpu)
        g = system.build_graph(el, self.N, compress=compress)
        assert (g.dcols is not None) == compress
        self.A = system.SellMatrix(g, 3).add_element_matrices(Ke.to(gpu), el)
        mask = torch.zeros((self.N, 3), dtype=torch.uint8, device=gpu)
        mask[fixed.to(gpu)] = 1
        self.w = self.A.jacobi(mask.view(-1))
        w = self.w.cpu()
        self.ids = None
        if name == "beam_two_node":      # the RCB aggregates plus a 2-node one: explicit ids
            self.ids = TL.rcb_aggregates(c, w, k)
            last = torch.nonzero(self.ids == k - 1).view(-1)
            self.ids[last[-2:]] = k
        elif name == "cube6_ids":        # labels 5 and 15, each aggregate strided through the node numbering
            kz = torch.arange(self.N) % 7
            self.ids = 10 * (kz // 4) + 5
        agg = self.ids if self.ids is not None else TL.rcb_aggregates(c, w, k)
        self.k = k
        self.cs = self.space()
        self.ref = TL.TwoLevelRef(A, c, w, agg, Aabs=Aabs, Cnt=Cnt)
        self.desc = TL.TwoLevelRef(A, c, w, agg, descending=True)
        self.r = torch.randn(3 * self.N, dtype=F64, generator=torch.Generator().manual_seed(11))

    def space(self):
        if self.ids is not None:
            return self.A.rigid_coarse_space(self.coords, self.w, aggregates=self.ids)
        return self.A.rigid_coarse_space(self.coords, self.w, n_aggregates=self.k)


SHAPES = [("beam", True), ("beam", False), ("beam_two_node", False), ("cube6_k1", True), ("cube6_k5", False),
          ("cube6_k8", True), ("cube12_k27", True), ("cube6_ids", False)]


@pytest.fixture(params=SHAPES, ids=[f"{n}-{'d16' if c else 'i32'}" for n, c in SHAPES])
def case(request, gpu):
    key = request.param
    if key not in _CASES:
        _CASES[key] = Case(key[0], gpu, key[1])
    return _CASES[key]


def test_aggregates_and_dropped_directions(case):
    cs, ref = case.cs, case.ref
    assert cs.n_aggregates == ref.k and cs.m == 6 * ref.k
    assert torch.equal(cs.agg.cpu().long(), ref.agg)
    assert cs.dropped == ref.dropped == (1 if case.name == "beam_two_node" else 0)
    assert torch.equal(cs.rel.cpu(), ref.rel), float((cs.rel.cpu() - ref.rel).abs().max())
    ptr, nodes = cs.agg_ptr.cpu().long(), cs.agg_nodes.cpu().long()
    for a in range(ref.k):
        assert torch.equal(nodes[ptr[a]:ptr[a + 1]], torch.nonzero(ref.agg == a).view(-1))
    assert set(cs.times) == {"aggregation", "E", "inverse"}


def test_restrict_and_galerkin_vs_restatement(case):
    cs, ref = case.cs, case.ref
    c = cs.restrict(case.r.to(cs.device))
    err, bound = (c.cpu() - ref.restrict(case.r)).abs(), ref.restrict_bound(case.r)
    print(f"{case.name}: restrict max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= bound).all())
    E, bound = cs.E.cpu(), ref.E_bound()
    err = (E - ref.E).abs()
    print(f"{case.name}: E max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3e}, "
          f"asymmetry/bound {float(((E - E.T).abs() / bound.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= bound).all())
    assert bool(((E - E.T).abs() <= bound).all())
    again = case.space()
    assert torch.equal(again.E, cs.E) and torch.equal(again.Einv, cs.Einv)
    assert torch.equal(again.restrict(case.r.to(cs.device)), c)


def _spread(a, b, per_entry=False):
    d = (a - b).abs()
    return float((d / a.abs()).max()) if per_entry else float(d.max() / a.abs().max())


def test_apply_and_history_vs_restatement(case):
    cs, ref, desc = case.cs, case.ref, case.desc
    za = ref.apply(case.r)
    spread = _spread(za, desc.apply(case.r))
    tol = max(SPREAD_FACTOR * spread, SPREAD_FLOOR)
    z = cs.apply(case.r.to(cs.device), case.w)
    err = _spread(za, z.cpu())
    print(f"{case.name}: apply spread {spread:.3e} tol {tol:.3e} err {err:.3e}")
    assert err <= tol
    assert torch.equal(cs.apply(case.r.to(cs.device)), z)
    b = case.F.reshape(-1)
    _, _, ha, _ = ref.pcg(b, tol=0.0, max_iter=20)
    _, _, hd, _ = desc.pcg(b, tol=0.0, max_iter=20)
    spread = _spread(ha, hd, per_entry=True)
    tol = max(SPREAD_FACTOR * spread, SPREAD_FLOOR)
    res = case.A.pcg_two_level(b.to(cs.device), coarse=cs, tol=0.0, max_iter=20, history=True)
    assert res.iterations == 20 and res.history.numel() == 20
    err = _spread(ha, res.history.cpu(), per_entry=True)
    print(f"{case.name}: history spread {spread:.3e} tol {tol:.3e} err {err:.3e}")
    assert err <= tol
    res2 = case.A.pcg_two_level(b.to(cs.device), coarse=cs, tol=0.0, max_iter=20, history=True, chunk=7)
    assert torch.equal(res2.history, res.history) and torch.equal(res2.x, res.x)


def test_solve_vs_direct(case):
    _, _, system = _mods()
    from fem355 import _capi as C
    cs, ref = case.cs, case.ref
    b = case.F.reshape(-1)
    bd = b.to(cs.device)
    tol = 1e-12 * float(torch.sqrt(torch.dot(bd, cs.apply(bd))))
    res = case.A.pcg_two_level(bd, coarse=cs, tol=tol, max_iter=3000)
    _, it_ref, _, status = ref.pcg(b, rtol=1e-12, max_iter=3000)
    u, ud = res.x.cpu(), ref.direct(b)
    uerr = float((u - ud).abs().max() / ud.abs().max())
    w = case.w.cpu()
    free = w != 0
    true_res = ref.masked_residual(b, u)
    allowed = tol / float(w[free].min()) ** 0.5 + TL.EPS * res.iterations * float(
        ((ref.A[ref.idp][:, ref.idp].abs() @ u.abs() + b.abs()) * free).norm())
    print(f"{case.name}: iterations {res.iterations} vs {it_ref}, u err {uerr:.3e}, true residual {true_res:.3e} "
          f"allowed {allowed:.3e} (||b|| {float(b.norm()):.3e})")
    assert res.status == C.PCG_CONVERGED and status == "converged"
    assert abs(res.iterations - it_ref) <= 2
    assert uerr <= 1e-9
    assert true_res <= allowed


def test_two_level_halves_the_iterations_on_the_beam(gpu):
    """On the device, against SellMatrix.pcg with the same w: each solved to 1e-10 of its own sqrt(r0.z0), which
    brings both true residuals below 1e-8 ||b|| (measured: 84 against 395 iterations, 5.3e-9 and 1.5e-10)."""
    from fem355 import _capi as C
    key = ("beam", True)
    if key not in _CASES:
        _CASES[key] = Case("beam", gpu, True)
    case = _CASES[key]
    b = case.F.reshape(-1)
    bd = b.to(gpu)
    two = case.A.pcg_two_level(bd, coarse=case.cs, tol=1e-10 * float(torch.sqrt(torch.dot(bd, case.cs.apply(bd)))),
                               max_iter=5000)
    jac = case.A.pcg(bd, None, w=case.w, mode=C.MODE_PCG, tol=1e-10 * float(torch.sqrt(torch.dot(bd, case.w * bd))),
                     max_iter=5000)
    r2 = case.ref.masked_residual(b, two.x.cpu()) / float(b.norm())
    r1 = case.ref.masked_residual(b, jac.x.cpu()) / float(b.norm())
    print(f"beam: Jacobi {jac.iterations} iterations (true residual {r1:.2e}), two-level {two.iterations} ({r2:.2e})")
    assert two.status == jac.status == C.PCG_CONVERGED
    assert r1 < 1e-8 and r2 < 1e-8
    assert 2 * two.iterations <= jac.iterations


def test_mixed_families_through_the_solver_route(gpu, capsys):
    """The mixed_static golden box (c3d4 + c3d8 + c3d6) through two_level_pcg_solver, against the restatement."""
    _, solver, _ = _mods()
    g = load_golden("mixed_static")
    c, fixed = g["coords"].to(F64), g["fixed"].long()
    N = c.shape[0]
    fams = [(R.tet4_K(c, g["c3d4"].long(), TL.E_MOD, TL.NU), g["c3d4"].long()),
            (R.iso_K(c, g["c3d8"].long(), "c3d8", TL.E_MOD, TL.NU), g["c3d8"].long()),
            (R.iso_K(c, g["c3d6"].long(), "c3d6", TL.E_MOD, TL.NU), g["c3d6"].long())]
    F = g["force"].to(F64)[:, :3].contiguous()
    u, res = solver.two_level_pcg_solver([k for k, _ in fams], [el for _, el in fams], c, F, fixed, rtol=1e-12,
                                         max_iter=3000, n_aggregates=4, device=gpu, return_info=True)
    out = capsys.readouterr().out
    assert f"Converged after {res.iterations} iterations." in out
    A, _, _ = TL.dense_matrix(fams, N)
    w = res.coarse.w.cpu()
    ref = TL.TwoLevelRef(A, c, w, TL.rcb_aggregates(c, w, 4))
    assert torch.equal(res.coarse.agg.cpu().long(), ref.agg)
    _, it_ref, _, status = ref.pcg(F, rtol=1e-12, max_iter=3000)
    ud = ref.direct(F)
    uerr = float((u.cpu().reshape(-1) - ud).abs().max() / ud.abs().max())
    print(f"mixed: iterations {res.iterations} vs {it_ref}, u err {uerr:.3e}")
    assert status == "converged" and abs(res.iterations - it_ref) <= 2 and uerr <= 1e-9
    assert float(u.cpu()[fixed].abs().max()) == 0.0


def test_out_of_scope_combinations_raise(gpu):
    mesh, solver, system = _mods()
    c, t = mesh.kuhn_cube(3, 0.1)
    f, fixed = mesh.cube_poisson_case(c)
    with pytest.raises(ValueError):
        solver.solve_tet4(c, t, f, fixed, kind="poisson", preconditioner="two-level", device=gpu)
    F, fixed = mesh.cube_elasticity_case(c)
    with pytest.raises(ValueError):
        solver.solve_tet4(c, t, F, fixed, kind="elastic", E=TL.E_MOD, nu=TL.NU, operator="matfree",
                          preconditioner="two-level", device=gpu)
    with pytest.raises(ValueError):
        solver.solve_tet4(c, t, F, fixed, kind="elastic", E=TL.E_MOD, nu=TL.NU, preconditioner="ilu", device=gpu)
    A1 = system.assemble_tet4_system(c.to(gpu), t.to(gpu), "poisson", 1.0, 0.0)   # bs = 1
    w1 = torch.ones(A1.n, dtype=F64, device=gpu)
    with pytest.raises(ValueError):
        A1.rigid_coarse_space(c.to(gpu), w1)
    with pytest.raises(ValueError):
        A1.pcg_two_level(w1, coarse=None)
    # the C entry points refuse bs = 1 themselves (FEM_EARG)
    from fem355 import _capi as C
    z = torch.zeros(8, dtype=F64, device=gpu)
    zi = torch.zeros(8, dtype=torch.int32, device=gpu)
    rc = C.lib().fem_coarse_restrict(2, 1, 1, C.ptr(zi), C.ptr(zi), C.ptr(z), C.ptr(z), C.ptr(z), C.ptr(z),
                                     C.stream(torch.device(gpu)))
    assert rc == C.FEM_EARG


def test_indefinite_matrix_is_refused_or_breaks_down(gpu):
    """-K instead of K: the coarse matrix is negative definite, so the setup's Cholesky fails with a ValueError that
    names an aggregate; with a space built on K and the values negated afterwards, the first p.Ap is negative and the
    solve stops with PCG_BREAKDOWN at iteration 1 without touching x."""
    mesh, _, system = _mods()
    from fem355 import _capi as C
    c, t = mesh.kuhn_cube(3, 0.1)
    F, fixed = mesh.cube_elasticity_case(c)
    Ke = R.tet4_K(c, t, TL.E_MOD, TL.NU).to(gpu)
    el = t.to(gpu)
    A = system.SellMatrix(system.build_graph(el, c.shape[0]), 3).add_element_matrices(Ke, el)
    mask = torch.zeros((c.shape[0], 3), dtype=torch.uint8, device=gpu)
    mask[fixed.to(gpu)] = 1
    w = A.jacobi(mask.view(-1))
    cs = A.rigid_coarse_space(c, w, n_aggregates=2)
    A.vals.neg_()
    with pytest.raises(ValueError, match="aggregate"):
        A.rigid_coarse_space(c, w, n_aggregates=2)
    res = A.pcg_two_level(F.reshape(-1).to(gpu), coarse=cs, tol=1e-8, max_iter=50)
    assert res.status == C.PCG_BREAKDOWN and res.iterations == 1 and res.pq < 0.0
    assert float(res.x.abs().max()) == 0.0


@pytest.mark.parametrize("reorder", [None, "rcm"])
def test_solve_tet4_routes(gpu, reorder):
    """The default kwarg is today's path bit for bit; "two-level" reaches the same solution in fewer iterations."""
    mesh, solver, _ = _mods()
    c, t = mesh.kuhn_cube(6, 0.15)
    F, fixed = mesh.cube_elasticity_case(c)
    kw = dict(kind="elastic", E=TL.E_MOD, nu=TL.NU, rtol=1e-10, device=gpu, reorder=reorder)
    u0, r0, _ = solver.solve_tet4(c, t, F, fixed, **kw)
    u1, r1, _ = solver.solve_tet4(c, t, F, fixed, preconditioner="jacobi", n_aggregates=None, **kw)
    assert torch.equal(u0, u1) and r0.iterations == r1.iterations
    u2, r2, _ = solver.solve_tet4(c, t, F, fixed, preconditioner="two-level", n_aggregates=8, **kw)
    assert r2.coarse.n_aggregates == 8
    assert r2.iterations < r0.iterations
    assert float((u2 - u0).abs().max() / u0.abs().max()) < 1e-7
