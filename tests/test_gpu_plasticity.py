"""Elastoplastic c3d4 statics on the device (csrc/plasticity.hip, element.compute_c3d4_plastic_update,
system.PlasticStatics, solver.elastoplastic_static_solver) against the CPU restatement of tests/plasticity_ref.py.

Meshes: mesh.kuhn_cube(3, jitter=0.15) (64 nodes, 162 tets: two full blocks of 64 elements and a partial one),
kuhn_cube(2, jitter=0.15), the single tet of test_gpu_nonlinear.mesh_of, and no element at all. Materials: E = 1,
nu = 0.3, sigma_y = 0.01, H = 0.1 on the unit cube; modal_ref.E / NU with sigma_y = 1e-3 E, H = 0.1 E on coordinates
scaled by modal_ref.SCALE. Fields (plasticity_ref.field): zero, random small (all elastic), random large (all plastic),
the graded stretch u = (a x^2, 0, 0) (half the elements yield), each from the virgin state and from the hardened state
the reference reaches on a graded stretch in z. Every case has |f_tr| >= 1e-6 sigma_y in every element of the reference
(asserted), so no element sits on the branch cut of the tangent.

Tolerances:
  element outputs  per element, max deviation <= 1e-12 x that element's max reference magnitude (the operator tolerance)
                   for Kt, fe, we, sigma, ep_out, alpha_out; where an element's reference is exactly zero: 1e-12 x
                   mu V max|g| (forces), mu V (energy), mu (stress), sigma_y / mu (strains). `plastic` exactly.
                   Packed == full upper blocks, full == its transpose, the Kt == NULL launch == the tangent launch in
                   every other output, aliased state buffers == separate ones, two runs: all bitwise. NaN tails past M
                   and N in every array stay NaN and no NaN comes out.
  elastic limit    sigma_y = 1e30: Kt vs compute_c3d4_K_matrix rel <= 1e-12, state out == state in, plastic all zero.
  state isolation  evaluate() at trial points leaves the committed buffers bit-identical; after commit() state() is the
                   last trial state bitwise; a refilled tangent matrix == a fresh one bitwise.
  uniaxial         kuhn_cube(2), rollers on x = 0 / y = 0 / z = 0, traction t on x = 1, load path 0.5, 1.0, 0.0 with
                   t_max = 2 sigma_y, tol 1e-10: max|u - u_exact| <= 2 tol ||F_free|| / lambda_min(K_T) (lambda_min of
                   the reference's final dense tangent); stress and alpha within the same bound times the strain per
                   displacement (sum_a |g_a|_1, and the moduli for the stress).
  solver cases     kuhn_cube(3), z = 0 fixed, top-face pull / shear sized so that 77 % / 64 % of the elements yield at
                   full load, load path 0.5, 1.0, 0.3, tol 1e-10: converged; Newton iterations per step <= the direct
                   restatement's + 2; max|u_dev - u_direct| <= 8 x the PCG restatement's own deviation from the direct
                   one; alpha within the same 8 x rule scaled by the strain per displacement 1/h, floor
                   1e-12 sigma_y / mu; the unloading step elastic (plastic_fraction 0, state bitwise unchanged); the
                   answer more than 1e-2 away from the linear-elastic one.

Measured on the MI355X (test_solver_cases prints: Newton iterations per step device / direct restatement, PCG iterations
per Newton iteration, share of yielding elements per step, deviation of the device / of the PCG restatement from the
direct restatement and their ratio (bound 8), the same for alpha, distance from the linear-elastic answer):
    pull   [5, 6, 2] / [5, 6, 1]   53-80 PCG iterations   plastic 0.025, 0.765, 0   7.49e-15  7.51e-15  1.00
           alpha 1.92e-14 / 1.91e-14 (bound 1.8e-13)   vs linear 6.99
    shear  [2, 6, 2] / [1, 6, 1]   47-71                  plastic 0, 0.636, 0       2.11e-15  2.15e-15  0.98
           alpha 4.24e-15 / 4.41e-15                   vs linear 1.22
The second iteration of an elastic step comes from the inexact inner solves (linear_rtol 1e-6 against tol 1e-10), as in
the PCG restatement. Before the first iteration of a step took the elastic tangent, the device needed 9 iterations with
step lengths down to 1/8 for the shear case's unloading step (the restatement 2): see DESIGN 8s.
Uniaxial case: max|u - u_exact| 2.1e-15 / 8.6e-15 / 7.7e-15 after the three load factors (bound 2.49e-11).
Element outputs against the restatement, worst case over the 48 (mesh, scale, start, field) cases, in units of the
bound's scale: Kt 1.2e-15, fe 4.5e-15, we 1.2e-15, sigma 4.3e-15, ep 2.3e-15, alpha 2.6e-15 (bound 1e-12)."""
import functools

import pytest
import torch

import plasticity_ref as PR
from conftest import rel
from test_gpu_nonlinear import mesh_of as nl_mesh_of, nan_padded, per_element_dev, per_element_mag, unpack

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
PAD = 3
MESHES = ("kuhn3", "kuhn2", "tet1")
SCALES = ("unit", "bench")
STARTS = ("virgin", "hardened")
OUTS = ("fe", "we", "sigma", "ep", "alpha", "plastic")


@functools.lru_cache(maxsize=None)
def case_of(name, scale):
    """(coords, tets, n, model) of one mesh and material."""
    c, t, n, _, _ = nl_mesh_of(name, scale)
    return c, t, n, PR.Model(c, t, *PR.material(scale))


@functools.lru_cache(maxsize=None)
def reference(name, scale, start, fld):
    """The restatement's outputs for one case, formed once and shared (never modified)."""
    c, t, n, m = case_of(name, scale)
    state = None if start == "virgin" else PR.hardened_state(m, n)
    u = PR.field(fld, c, n, PR.yield_strain(m.E, m.nu, m.sigma_y))
    return dict(u=u, state=state, **m.element(u, state))


def launch(dev, c, t, u, mat, state, packed, tangent=True, alias=False):
    """One raw fem_tet4_j2 launch on arrays with NaN tails past N and M -> the outputs' first M rows (+ bad)."""
    from fem355 import _capi as C
    lib = C.lib()
    N, M = c.shape[0], t.shape[0]
    E, nu, sy, H = mat
    cd, ud = nan_padded(c, dev), nan_padded(u, dev)
    td = torch.cat([t, torch.zeros((PAD, 4), dtype=torch.long)]).to(dev)
    S = int(lib.fem_ke_sym_stride(4))
    full = lambda *s: torch.full(s, NAN, dtype=F64, device=dev)
    ep_in = al_in = None
    if state is not None:
        ep_in, al_in = nan_padded(state[0], dev), nan_padded(state[1], dev)
    out = dict(Kt=full(M + PAD, S) if packed else full(M + PAD, 12, 12), fe=full(M + PAD, 4, 3), we=full(M + PAD),
               sigma=full(M + PAD, 6), ep=ep_in if alias else full(M + PAD, 6), alpha=al_in if alias else full(M + PAD))
    assert not alias or state is not None
    plastic = torch.full((M + PAD,), 255, dtype=torch.uint8, device=dev)
    bad = torch.full((1,), M, dtype=torch.int64, device=dev)
    C.check(lib.fem_tet4_j2(C.ptr(cd), C.ptr(td), M, C.ptr(ud), float(E), float(nu), float(sy), float(H),
                            C.ptr(ep_in), C.ptr(al_in), 1 if packed else 0, C.ptr(out["Kt"]) if tangent else None,
                            C.ptr(out["fe"]), C.ptr(out["we"]), C.ptr(out["sigma"]), C.ptr(out["ep"]),
                            C.ptr(out["alpha"]), C.ptr(plastic), C.ptr(bad), C.stream(torch.device(dev))),
            "fem_tet4_j2")
    torch.cuda.synchronize()
    res = {}
    for k, v in out.items():
        v = v.cpu()
        assert bool(torch.isnan(v[M:]).all()), f"{k}: the tail past M was written"
        if k != "Kt" or tangent:
            assert not bool(torch.isnan(v[:M]).any()), f"{k}: NaN in the output"
        res[k] = v[:M]
    plastic = plastic.cpu()
    assert bool((plastic[M:] == 255).all()) and bool((plastic[:M] <= 1).all())
    res["plastic"] = plastic[:M] != 0
    assert bool(torch.isnan(cd[N:]).all()) and bool(torch.isnan(ud[N:]).all())
    if state is not None and not alias:
        assert torch.equal(ep_in[:M].cpu(), state[0]) and torch.equal(al_in[:M].cpu(), state[1])
    res["bad"] = int(bad.cpu())
    return res


def scaled_dev(got, ref, floor):
    """max over elements of |got - ref| / (the element's max |ref|, or `floor` [M] where that is exactly zero)."""
    mag = per_element_mag(ref)
    return float((per_element_dev(got, ref) / torch.where(mag == 0, floor, mag)).max())


# ---------------------------------------------------------------- element kernel
@pytest.mark.parametrize("fld", PR.FIELDS)
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", MESHES)
def test_element_outputs(gpu, name, scale, start, fld):
    c, t, n, m = case_of(name, scale)
    o = reference(name, scale, start, fld)
    u, state, M = o["u"], o["state"], t.shape[0]
    mat = (m.E, m.nu, m.sigma_y, m.H)
    # no element of the reference sits on the branch cut
    assert float(o["f_tr"].abs().min()) >= 1e-6 * m.sigma_y
    full = launch(gpu, c, t, u, mat, state, packed=False)
    pk = launch(gpu, c, t, u, mat, state, packed=True)
    nt = launch(gpu, c, t, u, mat, state, packed=False, tangent=False)
    again = launch(gpu, c, t, u, mat, state, packed=False)
    assert full["bad"] == M
    # bitwise properties
    for (a, b), blk in unpack(pk["Kt"]).items():
        assert torch.equal(blk, full["Kt"][:, 3 * a: 3 * a + 3, 3 * b: 3 * b + 3]), (a, b)
    assert torch.equal(full["Kt"], full["Kt"].transpose(1, 2))
    for k in OUTS:
        assert torch.equal(nt[k], full[k]) and torch.equal(pk[k], full[k]), k
        assert torch.equal(again[k], full[k]), k
    assert torch.equal(again["Kt"], full["Kt"])
    if state is not None:
        al = launch(gpu, c, t, u, mat, state, packed=False, alias=True)
        for k in OUTS + ("Kt",):
            assert torch.equal(al[k], full[k]), k
    # against the restatement, per element
    assert torch.equal(full["plastic"], o["plastic"])
    gmax = m.g.abs().reshape(M, -1).amax(1)
    strain = torch.full((M,), m.sigma_y / m.mu, dtype=F64)
    floors = {"Kt": torch.ones(M, dtype=F64), "fe": m.mu * m.V * gmax, "we": m.mu * m.V, "sigma": torch.full((M,), m.mu, dtype=F64),
              "ep": strain, "alpha": strain}
    worst = {k: scaled_dev(full[k], o[k], floors[k]) for k in floors}
    print(f"{name} {scale} {start} {fld}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-12, (k, v)
    if fld == "zero" and state is None:
        assert float(full["fe"].abs().max()) == 0.0 and float(full["we"].abs().max()) == 0.0
    if not bool(o["plastic"].any()) and state is not None:     # an elastic update hands the state through
        assert torch.equal(full["ep"], state[0]) and torch.equal(full["alpha"], state[1])


@pytest.mark.parametrize("scale", SCALES)
def test_elastic_limit_is_the_linear_stiffness(gpu, scale):
    from fem355 import element, system
    c, t, n, m = case_of("kuhn3", scale)
    o = reference("kuhn3", scale, "hardened", "large")
    st = system.PlasticState(*o["state"])
    r = element.compute_c3d4_plastic_update(c, t, o["u"], m.E, m.nu, 1e30, m.H, state=st, device=gpu, dtype=F64)
    K0 = element.compute_c3d4_K_matrix(c, t, m.E, m.nu, device=gpu, dtype=F64)
    assert rel(r.K, K0) <= 1e-12
    assert torch.equal(r.state.plastic_strain.cpu(), o["state"][0])
    assert torch.equal(r.state.equivalent_plastic_strain.cpu(), o["state"][1])
    assert r.plastic.dtype == torch.bool and not bool(r.plastic.any())


def test_public_update(gpu):
    """The element.py layer on one case: shapes, dtype conversion, the tangent=False form, the singular element."""
    from fem355 import element, system
    c, t, n, m = case_of("kuhn3", "unit")
    o = reference("kuhn3", "unit", "hardened", "graded")
    st = system.PlasticState(*o["state"])
    args = (c, t, o["u"], m.E, m.nu, m.sigma_y, m.H)
    r = element.compute_c3d4_plastic_update(*args, state=st, device=gpu, dtype=F64)
    for got, k in ((r.K, "Kt"), (r.forces, "fe"), (r.energy, "we"), (r.stress, "sigma"),
                   (r.state.plastic_strain, "ep"), (r.state.equivalent_plastic_strain, "alpha")):
        assert got.is_cuda and rel(got, o[k]) <= 1e-12, k
    assert torch.equal(r.plastic.cpu(), o["plastic"])
    r2 = element.compute_c3d4_plastic_update(*args, state=st, tangent=False, device=gpu, dtype=F64)
    assert r2.K is None and torch.equal(r2.forces, r.forces) and torch.equal(r2.energy, r.energy)
    assert torch.equal(st.plastic_strain, o["state"][0])          # the caller's state is not modified
    assert element.compute_c3d4_plastic_update(*args, device=gpu).K.dtype == torch.float32
    v = element.compute_c3d4_plastic_update(*args, device=gpu, dtype=F64)
    w = element.compute_c3d4_plastic_update(*args, state=system.PlasticState.virgin(t.shape[0], gpu), device=gpu,
                                            dtype=F64)
    assert torch.equal(v.K, w.K) and torch.equal(v.state.plastic_strain, w.state.plastic_strain)
    flat = c.clone()
    flat[t[70]] = flat[t[70, 0]].clone()
    with pytest.raises(ValueError, match="Singular matrix"):
        element.compute_c3d4_plastic_update(flat, t, o["u"], m.E, m.nu, m.sigma_y, m.H, device=gpu)


def test_degenerate_element_and_no_elements(gpu):
    from fem355 import _capi as C, element
    lib = C.lib()
    c, t, n, m = case_of("kuhn3", "unit")
    o = reference("kuhn3", "unit", "hardened", "large")
    mat = (m.E, m.nu, m.sigma_y, m.H)
    flat = c.clone()
    for e in (70, 130):
        flat[t[e, 1:]] = flat[t[e, 0]].clone()       # collapses these tets (and degrades their neighbours)
    p = flat[t]
    det = ((p[:, 1] - p[:, 0]) * torch.linalg.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0])).sum(1)
    dead = det.abs() < 1e-12
    full = launch(gpu, flat, t, o["u"], mat, o["state"], packed=False)     # asserts: no NaN anywhere
    assert full["bad"] == int(torch.nonzero(dead)[0]) and bool(dead[70]) and bool(dead[130])
    for k in ("Kt", "fe", "we", "sigma"):
        assert float(full[k][dead].abs().max()) == 0.0, k
    assert not bool(full["plastic"][dead].any())
    assert torch.equal(full["ep"][dead], o["state"][0][dead]) and torch.equal(full["alpha"][dead], o["state"][1][dead])
    # M == 0: FEM_OK without a launch, null pointers are never touched; the argument errors come first
    nul = (None, None, 0) + (None,) * 9       # ep_in, alpha_in, packed, the outputs, bad_idx, stream
    assert lib.fem_tet4_j2(None, None, 0, None, 1.0, 0.3, 0.01, 0.1, *nul) == 0
    for E_, nu_, sy_, H_ in ((1.0, 0.3, 0.0, 0.1), (1.0, 0.3, -1.0, 0.1), (1.0, 0.3, 0.01, -0.1), (1.0, 0.5, 0.01, 0.1),
                             (1.0, -1.0, 0.01, 0.1), (1.0, 0.3, NAN, 0.1)):
        assert lib.fem_tet4_j2(None, None, 0, None, E_, nu_, sy_, H_, *nul) == C.FEM_EARG
        assert b"fem_tet4_j2" in lib.fem_last_error()
    one = torch.zeros(6, dtype=F64, device=gpu)
    assert lib.fem_tet4_j2(None, None, 0, None, 1.0, 0.3, 0.01, 0.1, C.ptr(one), *nul[1:]) == C.FEM_EARG
    assert lib.fem_tet4_j2(None, None, 0, None, 1.0, 0.3, 0.01, 0.0, *nul) == 0       # H = 0 is accepted
    t0 = torch.zeros((0, 4), dtype=torch.long)
    r = element.compute_c3d4_plastic_update(c, t0, torch.zeros_like(c), 1.0, 0.3, 0.01, 0.1, device=gpu, dtype=F64)
    assert r.K.shape == (0, 12, 12) and r.forces.shape == (0, 4, 3) and r.state.plastic_strain.shape == (0, 6)
    assert r.plastic.shape == (0,)


# ---------------------------------------------------------------- state isolation
@pytest.mark.parametrize("layout", ("layoutA", "plain"))
def test_state_isolation_and_refill(gpu, layout, monkeypatch):
    from fem355 import system
    if layout == "plain":
        monkeypatch.setenv("FEM355_SL", "0")
    c, t, n, m = case_of("kuhn3", "unit")
    o1, o2 = reference("kuhn3", "unit", "hardened", "graded"), reference("kuhn3", "unit", "hardened", "large")
    N, M = c.shape[0], t.shape[0]
    mask = torch.zeros(3 * N, dtype=torch.uint8, device=gpu)
    start = system.PlasticState(*(x.to(gpu) for x in o1["state"]))

    def make():
        return system.PlasticStatics(c.to(gpu), t.to(gpu), m.E, m.nu, m.sigma_y, m.H, mask, state=start)

    ns = make()
    committed = [b.clone() for b in ns._st[ns._c]]
    fext = torch.randn(3 * N, dtype=F64, generator=torch.Generator().manual_seed(13)).to(gpu)
    d = torch.randn(3 * N, dtype=F64, generator=torch.Generator().manual_seed(11)).to(gpu)
    for k, (o, tan) in enumerate(((o2, False), (o1, True), (o2, True), (o1, False))):
        r, en, rn, inv = ns.evaluate(o["u"].to(gpu), 0.5, fext, tangent=tan)
        assert inv is None
        assert torch.equal(ns._st[ns._c][0], committed[0]) and torch.equal(ns._st[ns._c][1], committed[1])
        assert torch.equal(ns.state().plastic_strain.cpu(), o1["state"][0])
        assert abs(en - float(o["we"].sum())) <= 1e-12 * float(o["we"].abs().sum())
        assert rel(r.cpu().view(N, 3), 0.5 * fext.cpu().view(N, 3) - m.f_int(None, fe=o["fe"])) <= 1e-12
        assert abs(ns.plastic_fraction() - float(o["plastic"].to(F64).mean())) <= 1e-15
    with pytest.raises(ValueError):
        ns.tangent()                   # the last evaluate formed no tangent
    # the tangent of an earlier evaluate, kept for tangent(), against the restatement's dense one
    ns.evaluate(o2["u"].to(gpu), 0.5, fext, tangent=True)
    y = ns.tangent().matvec(d).cpu()
    assert ns.A.solver_layout == (layout == "layoutA")
    assert rel(y, m.dense_tangent(o2["u"], o2["state"]) @ d.cpu()) <= 1e-12
    y1 = ns.tangent(o1["u"].to(gpu)).matvec(d).cpu()     # refilled in place
    fresh = make()
    assert torch.equal(y1, fresh.tangent(o1["u"].to(gpu)).matvec(d).cpu())
    assert torch.equal(ns.jacobi().cpu(), fresh.jacobi().cpu())
    # the elastic tangent of a step's first iteration: no state is touched, the trial state stays committable
    ye = ns.elastic_tangent().matvec(d).cpu()
    assert rel(ye, m.dense_tangent(torch.zeros_like(c)) @ d.cpu()) <= 1e-12
    assert torch.equal(ns._st[ns._c][0], committed[0]) and torch.equal(ns._st[ns._c][1], committed[1])
    # commit: the last trial state (that of o2) becomes the committed one, by a swap
    trial = ns.trial_state()
    ptrs = [b.data_ptr() for b in ns._st[1 - ns._c]]
    ns.commit()
    assert [b.data_ptr() for b in ns._st[ns._c]] == ptrs
    st = ns.state()
    assert torch.equal(st.plastic_strain, trial.plastic_strain)
    assert torch.equal(st.equivalent_plastic_strain, trial.equivalent_plastic_strain)
    assert rel(st.plastic_strain.cpu(), o2["ep"]) <= 1e-12 and rel(st.equivalent_plastic_strain.cpu(), o2["alpha"]) <= 1e-12
    with pytest.raises(ValueError):
        ns.commit()                    # nothing evaluated since
    assert rel(ns.stress(o1["u"].to(gpu)).cpu(), m.element(o1["u"], (o2["ep"], o2["alpha"]), tangent=False)["sigma"]) \
        <= 1e-12
    ns.close()
    fresh.close()


# ---------------------------------------------------------------- solver
def test_uniaxial_analytic_case(gpu, capsys):
    from fem355 import solver
    c, t, n, _ = case_of("kuhn2", "unit")
    m, F, mask, exact, pl = PR.uniaxial_case(c, t)
    tol, path = 1e-10, (0.5, 1.0, 0.0)
    _, st_ref, info = PR.newton(m, F, mask, path, tol=tol)
    assert info["converged"]
    free = ~mask.reshape(-1)
    lam_min = float(torch.linalg.eigvalsh(m.dense_tangent(info["u_steps"][2], st_ref)[free][:, free])[0])
    bound = 2.0 * tol * float(F.reshape(-1)[free].norm()) / lam_min
    gsum = float(m.g.abs().sum((1, 2)).max())         # |d eps_ij| <= gsum max|du| in every element
    t_max = 2.0 * m.sigma_y
    lines = []
    for k in range(3):       # the public function has no per-step output: one solve per prefix of the path
        u, res = solver.elastoplastic_static_solver(c, t, F, mask, m.E, m.nu, m.sigma_y, m.H, load_path=path[: k + 1],
                                                    tol=tol, device=gpu, return_info=True)
        assert res.converged and res.status == "OK" and res.failed_step is None
        dev_u = float((u.cpu() - exact[k]).abs().max())
        lines.append(f"lambda {path[k]}: max|u - u_exact| {dev_u:.2e} (bound {bound:.2e})")
        assert dev_u <= bound
        sig, al = res.stress.cpu(), res.state.equivalent_plastic_strain.cpu()
        want = torch.zeros(6, dtype=F64)
        want[0] = path[k] * t_max
        # |d sigma| <= (3 kappa + 2 mu) 3 |d eps|, |d alpha| <= sqrt(6) |d eps| (the return map does not expand)
        assert float((sig - want).abs().max()) <= (3.0 * m.kappa + 2.0 * m.mu) * 3.0 * gsum * bound
        if k >= 1:
            assert float((al - pl).abs().max()) <= 6.0 ** 0.5 * 3.0 * gsum * bound
            assert res.plastic_fraction[1:] == [1.0, 0.0][:k]     # lambda 0.5 has f_tr = 0 up to rounding: any share
    text = capsys.readouterr().out
    assert text.count("Load step 3/3") == 1
    with capsys.disabled():
        print("\n    uniaxial: " + "; ".join(lines))


@functools.lru_cache(maxsize=None)
def restatements(case):
    c, t, n, m = case_of("kuhn3", "unit")
    F, fixed = PR.solver_case(c, case)
    mask = torch.zeros(c.shape[0], 3, dtype=torch.bool)
    mask[fixed] = True
    ud, sd, idir = PR.newton(m, F, mask, PR.LOAD_PATH, tol=1e-10)
    up, sp, ipcg = PR.newton(m, F, mask, PR.LOAD_PATH, tol=1e-10, linear="pcg", linear_rtol=1e-6)
    assert idir["converged"] and ipcg["converged"]
    return F, fixed, ud, sd, idir, up, sp


@pytest.mark.parametrize("case", sorted(PR.SOLVER_CASES))
def test_solver_cases(gpu, case, capsys):
    from fem355 import solver
    c, t, n, m = case_of("kuhn3", "unit")
    F, fixed, ud, sd, idir, up, sp = restatements(case)
    kw = dict(tol=1e-10, device=gpu, return_info=True)
    u, info = solver.elastoplastic_static_solver(c, t, F, fixed, m.E, m.nu, m.sigma_y, m.H, load_path=PR.LOAD_PATH,
                                                 **kw)
    # the state before the unloading step: the same solve stopped after the second factor
    _, mid = solver.elastoplastic_static_solver(c, t, F, fixed, m.E, m.nu, m.sigma_y, m.H,
                                                load_path=PR.LOAD_PATH[:2], **kw)
    text = capsys.readouterr().out
    u = u.cpu()
    ulin = solver.solve_tet4(c, t, PR.LOAD_PATH[-1] * F, fixed, kind="elastic", E=m.E, nu=m.nu, rtol=1e-12,
                             device=gpu)[0].cpu()
    al = info.state.equivalent_plastic_strain.cpu()
    dev_d, pcg_d = float((u - ud).abs().max()), float((up - ud).abs().max())
    dev_a, pcg_a = float((al - sd[1]).abs().max()), float((sp[1] - sd[1]).abs().max())
    nonlin = float((u - ulin).abs().max() / ulin.abs().max())
    with capsys.disabled():
        print(f"\n    {case:5s} newton {info.newton_iterations} / {idir['iterations']}  pcg {info.pcg_iterations}  "
              f"plastic {[round(f, 3) for f in info.plastic_fraction]}  dev {dev_d:.2e}  pcg-restatement {pcg_d:.2e}  "
              f"ratio {dev_d / max(pcg_d, 1e-300):.2f}  alpha dev {dev_a:.2e} / {pcg_a:.2e}  "
              f"vs linear {nonlin:.3f}")
    assert info.converged and info.status == "OK" and info.failed_step is None
    assert text.count("Load step 3/3") == 1 and text.count("Converged after") == 5
    assert len(info.newton_iterations) == 3
    for k_dev, k_dir in zip(info.newton_iterations, idir["iterations"]):
        assert k_dev <= k_dir + 2
    assert dev_d <= 8 * pcg_d
    h = 1.0 / n
    assert dev_a <= max(8 * pcg_d / h, 1e-12 * m.sigma_y / m.mu)
    assert all(abs(a - b) <= 1.5 / t.shape[0] for a, b in zip(info.plastic_fraction, idir["plastic_fraction"]))
    assert 0.3 <= info.plastic_fraction[1] <= 0.9
    # the partial unloading is elastic and leaves the state as it was, bit for bit
    assert info.plastic_fraction[2] == 0.0
    assert torch.equal(info.state.plastic_strain, mid.state.plastic_strain)
    assert torch.equal(info.state.equivalent_plastic_strain, mid.state.equivalent_plastic_strain)
    assert rel(info.stress.cpu(), m.element(ud, sd, tangent=False)["sigma"]) <= 1e-8
    assert nonlin > 1e-2


def test_failure_paths_and_the_single_tet(gpu, capsys):
    from fem355 import solver, system
    c, t, n, m = case_of("kuhn3", "unit")
    F, fixed = PR.solver_case(c, "pull")
    hard = PR.hardened_state(m, n)
    st = system.PlasticState(*hard)
    u, info = solver.elastoplastic_static_solver(c, t, F, fixed, m.E, m.nu, m.sigma_y, m.H, load_path=[0.5, 1.0],
                                                 state=st, max_iter=1, device=gpu, return_info=True)
    assert not info.converged and info.status == system.NL_MAX_ITER and info.failed_step == 1
    assert "Load step 1" in info.message and info.plastic_fraction == []
    assert not bool(torch.isnan(u).any()) and not bool(torch.isnan(info.stress).any())
    assert torch.equal(info.state.plastic_strain.cpu(), hard[0])           # nothing converged: the state given
    assert torch.equal(info.state.equivalent_plastic_strain.cpu(), hard[1])
    # fails in the second step: the committed state is the first step's. A small first factor from the hardened state
    # is a linear problem (two iterations at tol 1e-4); two iterations cannot bring the full load, at which three
    # quarters of the elements yield, to 1e-4 ||F||.
    kw = dict(tol=1e-10, device=gpu, return_info=True)
    u2, two = solver.elastoplastic_static_solver(c, t, F, fixed, m.E, m.nu, m.sigma_y, m.H, load_path=[1e-3, 1.0],
                                                 state=st, max_iter=2, tol=1e-4, device=gpu, return_info=True)
    assert not two.converged and two.status == system.NL_MAX_ITER and two.failed_step == 2
    assert two.newton_iterations[0] <= 2 and two.plastic_fraction == [0.0] and not bool(torch.isnan(u2).any())
    assert torch.equal(two.state.plastic_strain.cpu(), hard[0])            # the elastic first step kept the state
    assert torch.equal(two.state.equivalent_plastic_strain.cpu(), hard[1])
    # the single tet: three nodes held, the fourth pulled past yield and released
    c1, t1, _, m1 = case_of("tet1", "unit")
    F1 = torch.zeros_like(c1)
    F1[3] = torch.tensor([0.0, 0.0, 0.004], dtype=F64)
    mask = torch.zeros(4, 3, dtype=torch.bool)
    mask[:3] = True
    ur, sr, ir = PR.newton(m1, F1, mask, (1.0, 0.0), tol=1e-10)
    u1, i1 = solver.elastoplastic_static_solver(c1, t1, F1, mask.to(torch.uint8), m1.E, m1.nu, m1.sigma_y, m1.H,
                                                load_path=[1.0, 0.0], **kw)
    capsys.readouterr()
    assert ir["converged"] and i1.converged and i1.plastic_fraction == [1.0, 0.0]
    assert rel(u1.cpu(), ur) <= 1e-8 and rel(i1.state.equivalent_plastic_strain.cpu(), sr[1]) <= 1e-8
    assert float(u1.cpu().abs().max()) > 0.0                                # a permanent set remains
    # default load path: k / load_steps
    _, i2 = solver.elastoplastic_static_solver(c1, t1, F1, [0, 1, 2], m1.E, m1.nu, m1.sigma_y, m1.H, load_steps=2,
                                               **kw)
    text = capsys.readouterr().out
    assert i2.converged and "Load step 2/2" in text and len(i2.newton_iterations) == 2
    with pytest.raises(ValueError):
        solver.elastoplastic_static_solver(c1, t1, F1, [0, 1, 2], m1.E, m1.nu, 0.0, m1.H, device=gpu)
