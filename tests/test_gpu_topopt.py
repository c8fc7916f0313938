"""Topology optimisation on the device (the scaled c3d4 assembly of csrc/assemble.hip, csrc/topopt.hip, system.TopOpt,
solver.topology_optimization_solver, solve_tet4(modulus_scale=...)) against the CPU restatement tests/topopt_ref.py.

Meshes: mesh.kuhn_cube(3, jitter=0.15) (64 nodes, 162 tets: two full blocks of 64 elements and a partial one),
kuhn_cube(2, jitter=0.15), the single tet of test_gpu_nonlinear.mesh_of, and the apex mesh (topopt_ref.apex_mesh: kuhn3
plus a node joined to the 18 triangles of z = 1, whose row has 17 columns, so bs = 1 takes the 32-column accumulator
configuration). E = 1, nu = 0.3. Arrays of raw launches carry NaN tails past N and M (PAD rows): the tails must come
back NaN and no NaN may come out.

Tolerances:
  scaled assembly  scale = 1: bitwise the unscaled add_tet4; scale = 0.25: bitwise 0.25 x it; seeded scale in
                   [1e-3, 1]: per row max deviation <= 1e-12 x the row's largest reference magnitude (the operator
                   tolerance) against the restatement's dense sum_e s_e K_e and against add_element_matrices of the
                   scaled element matrices; s1 then s2 without reset against the restatement of s1 + s2; two runs
                   bitwise. Fresh matrix (solver layout) and plain-values-first, bs = 1 and 3, all four meshes.
  solve_tet4       modulus_scale, rtol 1e-13: rel(u, direct restatement) < 1e-10 (test_gpu_parity's bound).
  unit energy      ce, dct per element <= 1e-12 x the element's reference magnitude; compliance vs u^T (A u) with A the
                   scaled assembly: 1e-12 relative.
  filter           forward / adjoint vs the restatement 1e-13 relative, passes 0, 1, 3; passes = 0 bitwise; constants
                   1e-15; volume 1e-14; adjoint identity 1e-13; two runs bitwise.
  OC update        rho_new vs the restatement 1e-12 absolute; bounds and pins exact; reached volume <= f sum V
                   (1 + 1e-12) and within 1e-10 relative of the restatement's; two runs bitwise.
  optimisation     kuhn3 cantilever, 12 iterations at linear_rtol 1e-10: every solve converges, volume fraction 0.4
                   within 1e-10, compliance non-increasing (1e-12 relative allowance), last <= 0.6 x first; max
                   |rho_dev - rho_direct| and the relative deviation of the compliance history each <= 8 x the PCG
                   restatement's own deviation from the direct one (floor 1e-11).

Measured on the MI355X (the tests print every figure before asserting), worst case over the parametrised cases:
    scaled assembly  vs restatement 5.4e-16, vs add_element_matrices 5.4e-16, s1 + s2 6.6e-16 (bound 1e-12)
    solve_tet4       elastic 86 PCG iterations, rel 1.6e-14; poisson 35 iterations, rel 4.6e-15 (bound 1e-10)
    unit energy      ce 8.6e-16, dct 9.4e-16, compliance vs u.(A u) 1.9e-16 (bounds 1e-12)
    filter           forward 3.8e-16, adjoint 4.8e-16, fused scale 1.1e-15 (1e-13); constant 1.7e-16 (1e-15); volume
                     2.4e-16 (1e-14); <F x, y> - <x, F^T y> 1.3e-16 (1e-13)
    OC update        max |rho_new - restatement| 4.4e-16 (bound 1e-12; below 1e-13, nothing to explain); the reached
                     volume fraction 0.500000000000000 in all six cases
    optimisation     PCG iterations 72-82 per design iteration, compliance 112.4561 -> 61.1585 (ratio 0.5438);
                     max |rho - rho_direct| device 5.83e-11, PCG restatement 5.43e-11, ratio 1.07 (bound 8);
                     compliance history device 1.32e-11, PCG restatement 1.20e-11, ratio 1.10 (bound 8).
The warm start does not lower the iteration counts of this small case (72 in the first iteration, 74 in the third):
the stop rule is relative to the load, and a move limit of 0.2 changes the operator as much as the solution."""
import functools

import pytest
import torch

import topopt_ref as TR
from conftest import rel
from test_gpu_nonlinear import mesh_of as nl_mesh_of, nan_padded

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
PAD = 3
MESHES = ("kuhn3", "kuhn2", "tet1", "apex")
PENAL, S_MIN, RHO_MIN, MOVE = 3.0, 1e-3, 1e-3, 0.2


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(coords, tets, model) of one mesh, formed once and shared (never modified)."""
    if name == "apex":
        c, t = TR.apex_mesh()
    else:
        c, t, _, _, _ = nl_mesh_of(name, "unit")
    return c, t, TR.Model(c, t, 1.0, 0.3)


def seeded(n, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(n, dtype=F64, generator=g)


def padded_mesh(name, dev):
    """Device coords / connectivity as views of arrays with tails past N and M (NaN coordinates, zero node ids)."""
    c, t, m = case_of(name)
    cd = nan_padded(c, dev)
    td = torch.cat([t, torch.zeros((PAD, 4), dtype=torch.long)]).to(dev)
    return cd, td, m


def tail_is_nan(x, n):
    return bool(torch.isnan(x[n:]).all()) and not bool(torch.isnan(x[:n]).any())


# ============================================================================ scaled assembly
@functools.lru_cache(maxsize=None)
def graph_of(name, dev):
    from fem355 import system
    c, t, m = case_of(name)
    return system.build_graph(t.to(dev), m.N)


def assemble(name, bs, mode, dev, scales, E=1.0, nu=0.3):
    """A SellMatrix of mesh `name` with add_tet4 called once per entry of `scales` (None: unscaled). mode "fresh": the
    class chooses the layout (the solver layout); "plain": the plain values were requested first."""
    from fem355 import system
    cd, td, m = padded_mesh(name, dev)
    A = system.SellMatrix(graph_of(name, dev), bs)
    if mode == "plain":
        A.vals
    for s in scales:
        sd = None if s is None else nan_padded(s, dev)[: m.M]
        A.add_tet4(cd[: m.N], td[: m.M], E, nu if bs == 3 else 0.0, scale=sd)
    torch.cuda.synchronize()
    assert tail_is_nan(cd, m.N)
    if mode == "fresh":
        assert A.solver_layout
    return A


def dense_of(A):
    rp, ci, v = A.csr()
    rp, ci, v = rp.cpu().long(), ci.cpu().long(), v.cpu()
    nb, bs = A.n_rows, A.bs
    rows = torch.repeat_interleave(torch.arange(nb), rp[1:] - rp[:-1])
    D = torch.zeros(nb, bs, nb, bs, dtype=F64)
    D[rows, :, ci[: rows.numel()], :] = v[: rows.numel()]
    return D.reshape(nb * bs, nb * bs)


def row_dev(D, K):
    """max over rows of max |D - K| / the row's largest |K|."""
    return float(((D - K).abs().max(1).values / K.abs().max(1).values).max())


@pytest.mark.parametrize("mode", ["fresh", "plain"])
@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_scaled_assembly(gpu, name, bs, mode):
    from fem355 import system
    c, t, m = case_of(name)
    kind = "elastic" if bs == 3 else "poisson"
    if bs == 1:
        assert (graph_of(name, gpu).max_width > 16) == (name == "apex")
    base = assemble(name, bs, mode, gpu, [None]).plain_values().clone()
    one = assemble(name, bs, mode, gpu, [torch.ones(m.M, dtype=F64)]).plain_values()
    assert torch.equal(one, base)
    quarter = assemble(name, bs, mode, gpu, [torch.full((m.M,), 0.25, dtype=F64)]).plain_values()
    assert torch.equal(quarter, 0.25 * base)
    s1, s2 = seeded(m.M, 1e-3, 1.0, 11), seeded(m.M, 1e-3, 1.0, 12)
    A1 = assemble(name, bs, mode, gpu, [s1])
    d_ref = row_dev(dense_of(A1), m.dense(s1, kind))
    again = assemble(name, bs, mode, gpu, [s1])
    assert torch.equal(A1.plain_values(), again.plain_values())
    # the same operator from stored, scaled element matrices
    Ke = m.element_matrices(kind) * s1.view(-1, 1, 1)
    B = system.SellMatrix(graph_of(name, gpu), bs).add_element_matrices(Ke.to(gpu), t.to(gpu))
    d_ke = row_dev(dense_of(A1), dense_of(B))
    A12 = assemble(name, bs, mode, gpu, [s1, s2])
    d_sum = row_dev(dense_of(A12), m.dense(s1 + s2, kind))
    print(f"scaled assembly {name} bs={bs} {mode}: vs restatement {d_ref:.2e}, vs add_element_matrices {d_ke:.2e}, "
          f"s1 + s2 {d_sum:.2e} (bound 1e-12)")
    assert d_ref <= 1e-12 and d_ke <= 1e-12 and d_sum <= 1e-12


@pytest.mark.parametrize("bs", [1, 3])
def test_scaled_assembly_reports_a_degenerate_element(gpu, bs):
    from fem355 import system
    c, t, m = case_of("kuhn2")
    c = c.clone()
    c[t[5, 3]] = c[t[5, 0]]
    A = system.SellMatrix(graph_of("kuhn2", gpu), bs)
    A.add_tet4(c.to(gpu), t.to(gpu), 1.0, 0.3 if bs == 3 else 0.0, scale=torch.ones(m.M, dtype=F64, device=gpu))
    with pytest.raises(ValueError, match="Singular matrix"):
        A.check_singular()


def test_scale_validation(gpu):
    from fem355 import solver, system
    c, t, m = case_of("kuhn2")
    cd, td = c.to(gpu), t.to(gpu)
    A = system.SellMatrix(graph_of("kuhn2", gpu), 3)
    good = torch.ones(m.M, dtype=F64, device=gpu)
    for bad in (good.cpu(), good.float(), good[:-1], torch.ones(m.M + 1, dtype=F64, device=gpu), [1.0] * m.M):
        with pytest.raises(ValueError):
            A.add_tet4(cd, td, 1.0, 0.3, scale=bad)
        with pytest.raises(ValueError):
            system.assemble_tet4_system(cd, td, "elastic", 1.0, 0.3, scale=bad)
    F, mask = TR.cantilever(c)
    fixed = torch.nonzero(mask[:, 0]).view(-1)
    with pytest.raises(ValueError):
        solver.solve_tet4(c, t, F, fixed, kind="elastic", E=1.0, nu=0.3, device=gpu, modulus_scale=good.cpu())
    with pytest.raises(ValueError, match="matrix-free"):
        solver.solve_tet4(c, t, F, fixed, kind="elastic", E=1.0, nu=0.3, device=gpu, modulus_scale=good,
                          operator="matfree")


@pytest.mark.parametrize("kind", ["elastic", "poisson"])
def test_solve_tet4_with_a_modulus_scale(gpu, kind):
    from fem355 import solver
    c, t, m = case_of("kuhn3")
    s = seeded(m.M, 1e-3, 1.0, 13)
    F, mask = TR.cantilever(c)
    fixed = torch.nonzero(mask[:, 0]).view(-1)
    dpn = 3 if kind == "elastic" else 1
    f = F if dpn == 3 else F[:, 2:3].clone()
    u, res, _ = solver.solve_tet4(c, t, f, fixed, kind=kind, E=1.0, nu=0.3 if dpn == 3 else 0.0, rtol=1e-13,
                                  device=gpu, modulus_scale=s.to(gpu))
    K = m.dense(s, kind)
    free = ~(mask.reshape(-1) if dpn == 3 else mask[:, 0])
    ref = torch.zeros(dpn * m.N, dtype=F64)
    ref[free] = torch.linalg.solve(K[free][:, free], f.reshape(-1)[free])
    d = rel(u.reshape(-1), ref)
    print(f"solve_tet4 modulus_scale {kind}: {res.iterations} PCG iterations, rel deviation {d:.2e} (bound 1e-10)")
    assert res.status == 1 and d < 1e-10


# ============================================================================ raw launches
def raw_volumes(name, dev, c=None):
    from fem355 import _capi as C
    lib = C.lib()
    cd, td, m = padded_mesh(name, dev)
    if c is not None:
        cd = nan_padded(c, dev)
    g = graph_of(name, dev)
    V = torch.full((m.M + PAD,), NAN, dtype=F64, device=dev)
    Vn = torch.full((m.N + PAD,), NAN, dtype=F64, device=dev)
    bad = torch.full((1,), m.M, dtype=torch.int64, device=dev)
    C.check(lib.fem_tet4_volumes(C.ptr(cd), C.ptr(td), m.M, C.ptr(g.inc_ptr), C.ptr(g.inc), m.N, C.ptr(V), C.ptr(Vn),
                                 C.ptr(bad), C.stream(torch.device(dev))), "fem_tet4_volumes")
    torch.cuda.synchronize()
    assert tail_is_nan(V, m.M) and tail_is_nan(Vn, m.N)
    return cd, td, g, V, Vn, int(bad.item())


@pytest.mark.parametrize("name", MESHES)
def test_volumes(gpu, name):
    _, _, m = case_of(name)
    _, _, _, V, Vn, bad = raw_volumes(name, gpu)
    assert bad == m.M
    assert rel(V[: m.M], m.V) <= 1e-14 and rel(Vn[: m.N], m.Vn) <= 1e-14


def raw_energy(name, dev, u, rho_t, c=None, want_dct=True):
    from fem355 import _capi as C
    lib = C.lib()
    cd, td, m = padded_mesh(name, dev)
    if c is not None:
        cd = nan_padded(c, dev)
    ud = nan_padded(u.view(m.N, 3), dev)
    rd = nan_padded(rho_t, dev)
    full = lambda n: torch.full((n,), NAN, dtype=F64, device=dev)
    ce, dct, comp = full(m.M + PAD), full(m.M + PAD), full(1 + PAD)
    work = full(int(lib.fem_topopt_work_len(m.M)) + PAD)
    bad = torch.full((1,), m.M, dtype=torch.int64, device=dev)
    C.check(lib.fem_tet4_unit_energy(C.ptr(cd), C.ptr(td), m.M, C.ptr(ud), 0.3, C.ptr(rd), PENAL, S_MIN, 1.0,
                                     C.ptr(ce), C.ptr(dct) if want_dct else None, C.ptr(work), C.ptr(comp), C.ptr(bad),
                                     C.stream(torch.device(dev))), "fem_tet4_unit_energy")
    torch.cuda.synchronize()
    assert tail_is_nan(ce, m.M) and tail_is_nan(comp, 1) and bool(torch.isnan(work[-PAD:]).all())
    assert tail_is_nan(dct, m.M) if want_dct else bool(torch.isnan(dct).all())
    return ce[: m.M].cpu(), dct[: m.M].cpu(), float(comp[0]), int(bad.item())


@pytest.mark.parametrize("name", MESHES)
def test_unit_energy(gpu, name):
    c, t, m = case_of(name)
    u = seeded(3 * m.N, -1e-2, 1e-2, 21)
    rho_t = seeded(m.M, RHO_MIN, 1.0, 22)
    ce, dct, comp, bad = raw_energy(name, gpu, u, rho_t)
    ce_ref = m.unit_energy(u)
    dct_ref = -PENAL * (1.0 - S_MIN) * rho_t ** (PENAL - 1.0) * ce_ref
    d_ce = float(((ce - ce_ref).abs() / ce_ref.abs()).max())
    d_dct = float(((dct - dct_ref).abs() / dct_ref.abs()).max())
    # the compliance against u^T (A u) with A from the scaled assembly
    s = TR.simp(rho_t, PENAL, S_MIN)
    A = assemble(name, 3, "fresh", gpu, [s])
    ud = u.to(gpu)
    quad = float(torch.dot(ud, A.matvec(ud)))
    d_c = abs(comp - quad) / abs(quad)
    ce2, _, comp2, _ = raw_energy(name, gpu, u, rho_t, want_dct=False)
    print(f"unit energy {name}: ce {d_ce:.2e}, dct {d_dct:.2e}, compliance vs u.Au {d_c:.2e} (bounds 1e-12)")
    assert bad == m.M and d_ce <= 1e-12 and d_dct <= 1e-12 and d_c <= 1e-12
    assert torch.equal(ce, ce2) and comp == comp2


def test_unit_energy_degenerate_element(gpu):
    c, t, m = case_of("kuhn3")
    c = c.clone()
    c[t[70, 3]] = c[t[70, 0]]
    flat = TR.HR.R.tet_volumes(c, t) < 1e-12 / 6.0
    first = int(torch.nonzero(flat).view(-1)[0])
    u = seeded(3 * m.N, -1e-2, 1e-2, 23)
    ce, dct, comp, bad = raw_energy("kuhn3", gpu, u, seeded(m.M, RHO_MIN, 1.0, 24), c=c)
    assert bad == first and bool(flat[70])
    assert bool((ce[flat] == 0).all()) and bool((dct[flat] == 0).all())
    assert not bool(torch.isnan(ce).any()) and comp == comp
    _, _, _, _, _, vbad = raw_volumes("kuhn3", gpu, c=c)
    assert vbad == first


def raw_filter(name, dev, x, passes, adjoint, want_scale=False):
    from fem355 import _capi as C
    lib = C.lib()
    _, _, m = case_of(name)
    cd, td, g, V, Vn, _ = raw_volumes(name, dev)
    xd = nan_padded(x, dev)
    full = lambda n: torch.full((n,), NAN, dtype=F64, device=dev)
    nt, et, out, sc = full(m.N + PAD), full(m.M + PAD), full(m.M + PAD), full(m.M + PAD)
    C.check(lib.fem_density_filter(C.ptr(td), m.M, C.ptr(g.inc_ptr), C.ptr(g.inc), m.N, C.ptr(V), C.ptr(Vn), C.ptr(xd),
                                   passes, 1 if adjoint else 0, PENAL, S_MIN, C.ptr(nt), C.ptr(et), C.ptr(out),
                                   C.ptr(sc) if want_scale else None, C.stream(torch.device(dev))),
            "fem_density_filter")
    torch.cuda.synchronize()
    assert tail_is_nan(out, m.M) and bool(torch.isnan(nt[m.N:]).all()) and bool(torch.isnan(et[m.M:]).all())
    assert tail_is_nan(xd, m.M)
    if want_scale:
        assert tail_is_nan(sc, m.M)
    return out[: m.M].cpu(), sc[: m.M].cpu()


@pytest.mark.parametrize("passes", [0, 1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_filter(gpu, name, passes):
    _, _, m = case_of(name)
    x, y = seeded(m.M, RHO_MIN, 1.0, 31), seeded(m.M, -1.0, 1.0, 32)
    fx, sc = raw_filter(name, gpu, x, passes, False, want_scale=True)
    fty, _ = raw_filter(name, gpu, y, passes, True)
    d_f, d_a = rel(fx, m.filter(x, passes)), rel(fty, m.filter_adjoint(y, passes))
    d_s = rel(sc, TR.simp(m.filter(x, passes), PENAL, S_MIN))
    const, _ = raw_filter(name, gpu, torch.full((m.M,), 0.37, dtype=F64), passes, False)
    d_c = float((const - 0.37).abs().max())
    v0, v1 = float(m.V @ x), float(m.V @ fx)
    a, b = float(fx @ y), float(x @ fty)
    d_id = abs(a - b) / max(abs(a), float(x.norm() * y.norm()))
    print(f"filter {name} passes={passes}: forward {d_f:.2e}, adjoint {d_a:.2e}, scale {d_s:.2e} (1e-13); constant "
          f"{d_c:.2e} (1e-15); volume {abs(v0 - v1) / v0:.2e} (1e-14); <Fx,y> - <x,F'y> {d_id:.2e} (1e-13)")
    assert d_f <= 1e-13 and d_a <= 1e-13 and d_s <= 1e-13 and d_c <= 1e-15
    assert abs(v0 - v1) <= 1e-14 * v0 and d_id <= 1e-13
    if passes == 0:
        assert torch.equal(fx, x) and torch.equal(fty, y)
    again, sc2 = raw_filter(name, gpu, x, passes, False, want_scale=True)
    assert torch.equal(again, fx) and torch.equal(sc2, sc) and torch.equal(raw_filter(name, gpu, y, passes, True)[0], fty)


def oc_inputs(m, seed):
    rho = seeded(m.M, RHO_MIN, 1.0, seed)
    dc = seeded(m.M, -2.0, 0.5, seed + 1)
    dc[::7] = 0.0
    return rho, dc


def raw_oc(name, dev, rho, dc, passive, f):
    from fem355 import _capi as C
    lib = C.lib()
    _, _, m = case_of(name)
    _, _, _, V, _, _ = raw_volumes(name, dev)
    rd, dd = nan_padded(rho, dev), nan_padded(dc, dev)
    pd = None if passive is None else torch.cat([passive, torch.full((PAD,), 1, dtype=torch.int8)]).to(dev)
    full = lambda n: torch.full((n,), NAN, dtype=F64, device=dev)
    new, out, work = full(m.M + PAD), full(2 + PAD), full(int(lib.fem_topopt_work_len(m.M)) + PAD)
    C.check(lib.fem_oc_update(C.ptr(rd), C.ptr(dd), C.ptr(V), C.ptr(pd), m.M, f, MOVE, RHO_MIN, TR.N_BISECT,
                              C.ptr(work), C.ptr(new), C.ptr(out), C.stream(torch.device(dev))), "fem_oc_update")
    torch.cuda.synchronize()
    assert tail_is_nan(new, m.M) and tail_is_nan(out, 2) and bool(torch.isnan(work[-PAD:]).all())
    assert tail_is_nan(rd, m.M) and tail_is_nan(dd, m.M)
    return new[: m.M].cpu(), float(out[0]), float(out[1])


@pytest.mark.parametrize("with_passive", [False, True])
@pytest.mark.parametrize("name", ["kuhn3", "kuhn2", "apex"])
def test_oc_update(gpu, name, with_passive):
    _, _, m = case_of(name)
    passive = None
    if with_passive:
        passive = torch.zeros(m.M, dtype=torch.int8)
        passive[:6], passive[6:12] = 1, -1
    rho, dc = oc_inputs(m, 41)
    f = 0.5
    new, ch, vf = raw_oc(name, gpu, rho, dc, passive, f)
    ref, ch_ref, vf_ref, _ = TR.oc_update(rho, dc, m.V, f, MOVE, RHO_MIN, passive)
    d = float((new - ref).abs().max())
    lo, hi = TR.oc_bounds(rho, MOVE, RHO_MIN)
    free = torch.ones(m.M, dtype=torch.bool) if passive is None else passive == 0
    print(f"OC {name} passive={with_passive}: max |rho_new - ref| {d:.2e} (bound 1e-12), volume fraction {vf:.15f} "
          f"vs {vf_ref:.15f}, change {ch:.6f}")
    assert d <= 1e-12
    assert bool((new[free] >= lo[free]).all()) and bool((new[free] <= hi[free]).all())
    if passive is not None:
        assert bool((new[passive > 0] == 1.0).all()) and bool((new[passive < 0] == RHO_MIN).all())
    assert vf <= f * (1 + 1e-12)
    assert abs(vf - vf_ref) <= 1e-10 * vf_ref and abs(ch - ch_ref) <= 1e-12
    again = raw_oc(name, gpu, rho, dc, passive, f)
    assert torch.equal(again[0], new) and again[1:] == (ch, vf)


def test_oc_update_without_a_descent_direction(gpu):
    _, _, m = case_of("kuhn3")
    rho = seeded(m.M, RHO_MIN, 1.0, 43)
    dc = seeded(m.M, 0.0, 1.0, 44)
    dc[::5] = 0.0
    new, ch, vf = raw_oc("kuhn3", gpu, rho, dc, None, 0.5)
    assert torch.equal(new, rho) and ch == 0.0
    assert abs(vf - float(m.V @ rho) / float(m.V.sum())) <= 1e-14


# ============================================================================ the optimisation run
RUN = dict(E=1.0, nu=0.3, volume_fraction=0.4, penal=PENAL, s_min=S_MIN, rho_min=RHO_MIN, filter_passes=1, move=MOVE,
           max_iter=12, change_tol=0.0, linear_rtol=1e-10)


@functools.lru_cache(maxsize=None)
def reference_runs():
    """The restatement's direct and PCG runs of the optimisation case, formed once."""
    c, t, m = case_of("kuhn3")
    F, mask = TR.cantilever(c)
    rho0 = torch.full((m.M,), 0.4, dtype=F64)
    direct = TR.Design(m, F, mask, 0.4).run(rho0, 12)
    pcg = TR.Design(m, F, mask, 0.4, linear="pcg", linear_rtol=1e-10).run(rho0, 12)
    return F, mask, direct, pcg


def test_optimisation_run(gpu):
    from fem355 import solver
    c, t, m = case_of("kuhn3")
    F, mask, direct, pcg = reference_runs()
    res = solver.topology_optimization_solver(c, t, F, mask, device=gpu, **RUN)
    comp = res.compliance
    print(f"optimisation run: status {res.status}, PCG iterations {res.pcg_iterations}, compliance {comp[0]:.4f} -> "
          f"{comp[-1]:.4f} (ratio {comp[-1] / comp[0]:.4f})")
    assert res.status == "MAX_ITER" and not res.converged and len(comp) == 12 and len(res.pcg_iterations) == 12
    assert all(abs(v - 0.4) <= 1e-10 for v in res.volume_fraction)
    assert all(c1 <= c0 * (1 + 1e-12) for c0, c1 in zip(comp, comp[1:]))
    assert comp[-1] <= 0.6 * comp[0]
    assert max(abs(a - b) / abs(a) for a, b in zip(comp, res.load_work)) <= 1e-8
    hist = lambda h: max(abs(a - b) / abs(b) for a, b in zip(h["compliance"], direct["compliance"]))
    dev_rho = float((res.density.cpu() - direct["density"]).abs().max())
    pcg_rho = float((pcg["density"] - direct["density"]).abs().max())
    dev_c, pcg_c = hist({"compliance": comp}), hist(pcg)
    print(f"  max |rho - rho_direct|: device {dev_rho:.2e}, PCG restatement {pcg_rho:.2e}, ratio "
          f"{dev_rho / max(pcg_rho, 1e-300):.2f} (bound 8, floor 1e-11)")
    print(f"  compliance history rel: device {dev_c:.2e}, PCG restatement {pcg_c:.2e}, ratio "
          f"{dev_c / max(pcg_c, 1e-300):.2f} (bound 8, floor 1e-11)")
    assert dev_rho <= max(8 * pcg_rho, 1e-11) and dev_c <= max(8 * pcg_c, 1e-11)
    assert float(res.filtered_density.min()) > 0 and tuple(res.u.shape) == (m.N, 3)
    assert tuple(res.modulus_scale.shape) == (m.M,)


def steps(gpu, n, passive=None):
    from fem355 import system
    c, t, m = case_of("kuhn3")
    F, mask = TR.cantilever(c)
    to = system.TopOpt(c.to(gpu), t.to(gpu), F, mask.to(torch.uint8).view(-1), 1.0, 0.3, 0.4, PENAL, S_MIN, RHO_MIN, 1,
                       MOVE, passive=passive)
    rho = torch.full((m.M,), 0.4, dtype=F64, device=gpu)
    recs = []
    try:
        for _ in range(n):
            r = to.step(rho, 1e-10)
            rho = r["rho_new"].clone()
            recs.append((rho.cpu(), r["compliance"], r["change"], r["volume_fraction"], r["pcg_iterations"],
                         r["u"].cpu().clone()))
    finally:
        to.close()
    return recs


def test_step_twice_is_bitwise_identical(gpu):
    a, b = steps(gpu, 12), steps(gpu, 12)
    res_c = [r[1] for r in a]
    assert res_c[-1] <= 0.6 * res_c[0]   # the optimisation case itself
    for ra, rb in zip(a, b):
        assert torch.equal(ra[0], rb[0]) and torch.equal(ra[5], rb[5]) and ra[1:5] == rb[1:5]


def test_passive_solid_elements_stay_solid(gpu):
    c, t, m = case_of("kuhn3")
    F, _ = TR.cantilever(c)
    loaded = torch.nonzero(F[:, 2] != 0).view(-1)
    passive = torch.zeros(m.M, dtype=torch.int8)
    passive[torch.isin(t, loaded).any(1)] = 1
    assert 0 < int(passive.sum()) < m.M
    recs = steps(gpu, 4, passive=passive)
    assert all(bool((r[0][passive > 0] == 1.0).all()) for r in recs)
    assert all(abs(r[3] - 0.4) <= 1e-10 for r in recs)


def test_modules_export_the_user_kernels(gpu):
    from fem355 import element
    c, t, m = case_of("kuhn3")
    u = seeded(3 * m.N, -1e-2, 1e-2, 51).view(m.N, 3)
    ce = element.compute_c3d4_unit_energy(c, t, u, 0.3, device=gpu)
    assert float(((ce.cpu() - m.unit_energy(u)).abs() / m.unit_energy(u)).max()) <= 1e-12
    x = seeded(m.M, 0.0, 1.0, 52)
    for adj in (False, True):
        got = element.density_filter(c, t, x, passes=2, adjoint=adj, device=gpu).cpu()
        assert rel(got, (m.filter_adjoint if adj else m.filter)(x, 2)) <= 1e-13


# ============================================================================ failure paths
@pytest.mark.parametrize("kw", [dict(volume_fraction=0.0), dict(volume_fraction=1.5), dict(penal=0.5), dict(s_min=0.0),
                                dict(s_min=1.0), dict(rho_min=0.0), dict(rho_min=1.0), dict(move=0.0),
                                dict(filter_passes=-1), dict(rho0="short"), dict(passive="short"), dict(F="fixed only"),
                                dict(elements="c3d8")])
def test_value_errors(gpu, kw):
    from fem355 import solver
    c, t, m = case_of("kuhn2")
    F, mask = TR.cantilever(c)
    args = dict(RUN, max_iter=1)
    el = t
    for k, v in kw.items():
        if k == "rho0":
            args[k] = torch.full((m.M - 1,), 0.4, dtype=F64)
        elif k == "passive":
            args[k] = torch.zeros(m.M + 1, dtype=torch.int8)
        elif k == "F":
            F = torch.zeros_like(F)
            F[mask[:, 0], 2] = 1.0
        elif k == "elements":
            el = torch.cat([t, t], dim=1)
        else:
            args[k] = v
    with pytest.raises(ValueError):
        solver.topology_optimization_solver(c, el, F, mask, device=gpu, **args)


def test_degenerate_element_raises(gpu):
    from fem355 import solver
    c, t, m = case_of("kuhn2")
    F, mask = TR.cantilever(c)
    c = c.clone()
    c[t[5, 3]] = c[t[5, 0]]
    with pytest.raises(ValueError, match="Singular matrix encountered while computing B matrix."):
        solver.topology_optimization_solver(c, t, F, mask, device=gpu, **RUN)


def test_linear_solve_failure_keeps_the_start_density(gpu):
    from fem355 import solver
    c, t, m = case_of("kuhn3")
    F, mask = TR.cantilever(c)
    res = solver.topology_optimization_solver(c, t, F, mask, device=gpu, **dict(RUN, linear_max_iter=1))
    assert res.status == "LINEAR_SOLVE_FAILED" and not res.converged and res.message
    assert torch.equal(res.density.cpu(), torch.full((m.M,), 0.4, dtype=F64))
    assert res.compliance == [] and res.pcg_iterations == [1]
