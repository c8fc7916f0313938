"""Transient dynamics on the device (csrc/transient.hip, system.NewmarkIntegrator, solver.transient_solver) against torch
compositions of the existing operators and the dense CPU restatement of tests/newmark_ref.py.

Kernel meshes: mesh.kuhn_cube(4, jitter=0.15) (125 nodes, a partial last slice), mesh.kuhn_cube(10, jitter=0.15) (1331
nodes, 21 slices), mesh.hex_box(4), scaled by modal_ref.SCALE. Axes: bs 1 and 3, 16-bit deltas and int32 columns, for
bs = 3 layout A and the plain planes (FEM355_SL=0), the SELL mass and a diagonal mass.

Tolerances:
  scaled_add_mass  element-wise 4 * 2^-53 (|cK k| + |cM m|): three roundings with either FMA contraction; Jacobi weights
                   4 eps of the reciprocal of the combined diagonal; matvec rel < 1e-12 (the operator tolerance).
  fem_newmark_rhs  rel < 1e-12 against amp F + M yM + A yK from the existing matvecs; two runs bit-equal; a NaN tail
                   past row n in every vector is neither read nor written.
  fem_newmark_update  every formula within 8 * 2^-53 of the sum of the magnitudes of its terms, evaluated in torch on
                   the kernel's own inputs to that formula; fixed rows exactly zero.
  energy           1e-13 ||x|| ||K x|| and 1e-13 ||y|| ||M y|| (the modal tall-skinny bound); two runs bit-equal.
  trajectories     transient_solver at rtol 1e-8, 64 steps on one context, the recorded u of every node against the
                   direct-solve restatement: max deviation <= 8 x the PCG restatement's own deviation on the same case
                   and scenario (8: the margin the modal and hard-geometry tests use for a ratio of two like errors);
                   conservative scenarios: energy drift <= 8 x the PCG restatement's drift + 64 sqrt(n) 2^-53; loaded or
                   damped scenarios (no conserved energy, E_0 may be 0): the energy history against the direct
                   restatement's, relative to its maximum, under the same bound built from the PCG restatement's.

Measured on the MI355X (test_trajectory prints every run; deviation of the device / of the PCG restatement from the direct
restatement, their ratio (bound 8), the energy figure and its bound; PCG iterations per step equal the restatement's
except hex4, 39..58 against 39..59):
    elastic4  mode       9.67e-09  1.02e-08  0.95   5.88e-12 (5.88e-11)     65..110 iterations
    elastic4  damped     2.67e-09  3.14e-09  0.85   8.90e-11 (7.56e-10)     93..112
    elastic4  step_load  3.59e-08  3.57e-08  1.01   2.18e-08 (1.75e-07)     92..106
    elastic4  sine_load  2.57e-08  2.50e-08  1.03   1.58e-08 (1.29e-07)     82..103
    elastic4  predictor  4.17e-09  4.37e-09  0.96   7.70e-13 (1.77e-11)     73..96
    poisson6  mode       3.35e-08  3.35e-08  1.00   3.23e-14 (3.33e-13)     22..42
    poisson6  damped     7.25e-09  7.25e-09  1.00   1.12e-09 (8.98e-09)     31..42
    poisson6  step_load  1.34e-07  1.34e-07  1.00   2.40e-08 (1.92e-07)     37..39
    poisson6  sine_load  6.04e-08  6.04e-08  1.00   1.81e-08 (1.45e-07)     31..38
    poisson6  predictor  1.88e-08  1.88e-08  1.00   3.46e-14 (4.47e-13)     26..35
    hex4      mode       1.87e-09  1.86e-09  1.00   3.52e-13 (4.90e-12)     39..58
    hex4      damped     2.68e-09  2.53e-09  1.06   8.62e-11 (6.93e-10)     74..89
    hex4      step_load  5.37e-08  5.49e-08  0.98   4.13e-08 (3.29e-07)     84..91
    hex4      sine_load  1.79e-08  2.00e-08  0.90   1.04e-08 (9.50e-08)     70..86
    hex4      predictor  1.67e-09  1.74e-09  0.96   7.23e-13 (4.77e-12)     42..52
    lumped5   mode       1.28e-08  1.28e-08  1.00   7.24e-12 (5.75e-11)     81..136
    lumped5   damped     3.44e-09  3.38e-09  1.02   4.84e-11 (3.92e-10)     120..141
    lumped5   step_load  2.86e-08  2.81e-08  1.02   2.49e-08 (1.97e-07)     119..132
    lumped5   sine_load  1.24e-08  1.18e-08  1.05   1.05e-08 (8.11e-08)     111..129
    lumped5   predictor  1.36e-08  1.31e-08  1.04   2.75e-12 (1.53e-11)     94..119
The update kernel's formulas: at most 3.84 x 2^-53 of their terms (bound 8)."""
import ctypes
import math

import pytest
import torch

import modal_ref as MR
import newmark_ref as NR
from conftest import rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -53
MESHES = ("kuhn4", "kuhn10", "hex4")
VARIANTS = ("bs1-delta16", "bs1-int32", "bs3-layoutA", "bs3-plain16", "bs3-int32")
CK, CM = 1.37, 2.9e9


# ---------------------------------------------------------------- device matrices of the kernel meshes
class Setup:
    def __init__(self, dev, mesh_name, variant, monkeypatch):
        from fem355 import mesh, system
        if mesh_name == "hex4":
            c, el = mesh.hex_box(4)
        else:
            c, el = mesh.kuhn_cube(4 if mesh_name == "kuhn4" else 10, jitter=0.15)
        c = c * MR.SCALE
        self.N, self.dpn = c.shape[0], 1 if variant.startswith("bs1") else 3
        self.n = self.N * self.dpn
        self.el = el
        if mesh_name == "hex4":
            self.Ms = MR.hex_scalar_mass(c, el)
            # bs = 1 on hexes: any symmetric element matrix on the pattern exercises the kernels
            self.Ke = R.iso_K(c, el, "c3d8", MR.E, MR.NU) if self.dpn == 3 else 3.0e13 * self.Ms
        else:
            self.Ms = MR.tet_scalar_mass(c, el)
            self.Ke = R.tet4_K(c, el, MR.E, MR.NU) if self.dpn == 3 else R.tet4_poisson_K(c, el) * 1e9
        self.Me = torch.kron(self.Ms, torch.eye(self.dpn, dtype=F64).view(1, self.dpn, self.dpn))
        if variant == "bs3-plain16":
            monkeypatch.setenv("FEM355_SL", "0")
        compress = not variant.endswith("int32")
        self.g = system.build_graph(el.to(dev), self.N, compress=compress)
        assert (self.g.dcols is not None) == compress
        self.A, self.Mg = system.SellMatrix(self.g, self.dpn), system.SellMatrix(self.g, 1)
        if self.dpn == 3:
            self.A.add_stiffness_and_mass(self.Ke.to(dev), self.Ms.to(dev), el.to(dev), self.Mg)
        else:
            self.A.add_element_matrices(self.Ke.to(dev), el.to(dev))
            self.Mg.add_element_matrices(self.Ms.to(dev), el.to(dev))
        assert self.A.solver_layout == (variant == "bs3-layoutA")
        gen = torch.Generator().manual_seed(len(mesh_name) * 31 + len(variant))
        self.d = (torch.rand(self.n, dtype=F64, generator=gen) + 0.5).to(dev) * float(self.Ms.abs().max())
        fixed = mesh.face_nodes(c, 2, 0.0)
        mask = torch.zeros((self.N, self.dpn), dtype=torch.uint8, device=dev)
        mask[fixed.to(dev)] = 1
        self.mask = mask.view(-1)
        self.gen = gen

    def masses(self):
        return (("sell", self.Mg), ("diag", self.d))

    def mass_times(self, mass, x):
        """M x from the existing operators."""
        if torch.is_tensor(mass):
            return mass * x
        X = x.view(self.N, self.dpn)
        return torch.stack([mass.matvec(X[:, r].contiguous()) for r in range(self.dpn)], 1).reshape(-1)

    def randn(self, *shape):
        return torch.randn(*shape, dtype=F64, generator=self.gen).to(self.A.device)


_SETUPS = {}


@pytest.fixture
def kcase(gpu, monkeypatch):
    def get(mesh_name, variant):
        key = (mesh_name, variant)
        if key not in _SETUPS:
            _SETUPS[key] = Setup(gpu, mesh_name, variant, monkeypatch)
        return _SETUPS[key]
    return get


def _padded(vals, n):
    """(buffer with a NaN tail of 64 values per row of `vals`, its leading view holding vals)."""
    vals = vals.contiguous()
    buf = torch.full((n + 64,) + tuple(vals.shape[1:]), float("nan"), dtype=F64, device=vals.device)
    buf[:n] = vals
    return buf, buf[:n]


# ---------------------------------------------------------------- 1. K_eff = cK K + cM M
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_name", MESHES)
def test_scaled_add_mass(kcase, mesh_name, variant):
    s = kcase(mesh_name, variant)
    A, g, bs = s.A, s.g, s.dpn
    Kc = A.csr()[2].clone()
    Mc = s.Mg.csr()[2].clone()
    eye = torch.eye(bs, dtype=F64, device=A.device)
    for name, mass in s.masses():
        B = A.scaled_add_mass(mass, CK, CM)
        assert B.solver_layout == A.solver_layout and B.g is g and B.bs == bs
        if name == "sell":
            Mfull = Mc.view(-1, 1, 1) * eye
        else:
            Mfull = torch.zeros_like(Kc)
            Mfull[g.diagpos.long()] = torch.diag_embed(mass.view(s.N, bs))
        want = CK * Kc + CM * Mfull
        got = B.csr()[2]
        bound = 4.0 * EPS * ((CK * Kc).abs() + (CM * Mfull).abs())
        worst = float(((got - want).abs() - bound).max())
        assert worst <= 0.0, (name, worst)
        # the stored array: every padding value exactly 0
        ent = g.sell_entries
        real = torch.zeros(ent, dtype=torch.bool, device=A.device)
        real[g.csr2sell[: g.nnz]] = True
        pad = ~real.view(-1, 64)
        if B.solver_layout:
            ch = B._svals[: ent * 9].view(-1, 576)
            assert not bool(ch[:, :512].view(-1, 4, 64, 2)[pad[:, None, :, None].expand(-1, 4, -1, 2)].any())
            assert not bool(ch[:, 512:][pad].any())
        else:
            ch = B._vals[: ent * bs * bs].view(-1, bs * bs, 64)
            assert not bool(ch[pad[:, None, :].expand(-1, bs * bs, -1)].any())
        # Jacobi weights and the product
        diag = want[g.diagpos.long()].diagonal(dim1=1, dim2=2).reshape(-1)
        w = B.jacobi(s.mask)
        free = s.mask == 0
        assert not bool(w[~free].any())
        assert float(((w - 1.0 / diag).abs() * diag)[free].max()) <= 4.0 * 2.0 ** -52
        x = s.randn(s.n)
        e = rel(B.matvec(x), CK * A.matvec(x) + CM * s.mass_times(mass, x))
        print(f"{mesh_name} {variant} {name}: matvec {e:.2e}")
        assert e < 1e-12, (name, e)
        # pcg reads the result as it is
        rhs = B.matvec(x * free)
        res = B.pcg(rhs, w=w, tol=1e-10 * float(torch.sqrt(torch.dot(rhs, w * rhs))), max_iter=2000)
        assert res.status == 1 and rel(res.x, x * free) < 1e-6


def test_scaled_add_mass_of_a_bs1_solver_layout_matrix(gpu):
    """Only add_tet4 makes a bs = 1 matrix in the solver layout: it goes through plain_values() and yields a plain
    K_eff with the same values."""
    from fem355 import mesh, system
    c, t = mesh.kuhn_cube(4, jitter=0.15)
    A = system.assemble_tet4_system(c.to(gpu), t.to(gpu), "poisson", E=2.0)
    assert A.solver_layout and A.bs == 1
    d = torch.rand(A.n, dtype=F64, generator=torch.Generator().manual_seed(3)).to(gpu) + 0.5
    B = A.scaled_add_mass(d, CK, 0.25)
    assert not B.solver_layout and A.solver_layout
    Kc = A.csr()[2].clone()
    Mfull = torch.zeros_like(Kc)
    Mfull[A.g.diagpos.long()] = d.view(-1, 1, 1)
    bound = 4.0 * EPS * ((CK * Kc).abs() + (0.25 * Mfull).abs())
    assert float(((B.csr()[2] - (CK * Kc + 0.25 * Mfull)).abs() - bound).max()) <= 0.0
    x = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(4)).to(gpu)
    assert rel(B.matvec(x), CK * A.matvec(x) + 0.25 * d * x) < 1e-12


# ---------------------------------------------------------------- 2. the right-hand side
def _rhs(s, mass, kv, la, amp, F, Y, b):
    from fem355 import _capi as C
    A = s.A
    form, mass = A._mass_form("test", mass)
    mv = A._mass_values(form, mass)
    cols, dcols = A._multi_cols()
    C.check(C.lib().fem_newmark_rhs(s.N, s.dpn, la, C.ptr(s.g.slice_ptr), cols, dcols, C.ptr(kv), C.ptr(mv), form,
                                    float(amp), C.ptr(F), C.ptr(Y), C.ptr(b), C.stream(A.device)), "fem_newmark_rhs")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_name", MESHES)
def test_newmark_rhs(kcase, mesh_name, variant):
    s = kcase(mesh_name, variant)
    A, n = s.A, s.n
    kv, la = A._held_values()
    assert la == (1 if variant == "bs3-layoutA" else 0)
    amp = 0.7
    Ybuf, Y = _padded(s.randn(n, 2), n)
    Fbuf, F = _padded(s.randn(n) * float(s.Ke.abs().max()), n)
    Kyk = A.matvec(Y[:, 0].contiguous())
    for name, mass in s.masses():
        Mym = s.mass_times(mass, Y[:, 1].contiguous()) * 1e9   # the mass term at the size of the stiffness term
        Ys = Y.clone()
        Ys[:, 1] *= 1e9
        Ysbuf, Ysv = _padded(Ys, n)
        for damped in (True, False):
            want = amp * F + Mym + (Kyk if damped else 0.0)
            outs = []
            for _ in range(2):
                bbuf = torch.full((n + 64,), float("nan"), dtype=F64, device=A.device)
                _rhs(s, mass, kv if damped else None, la if damped else 0, amp, F, Ysv, bbuf[:n])
                assert bool(torch.isnan(bbuf[n:]).all()) and bool(torch.isfinite(bbuf[:n]).all())
                outs.append(bbuf[:n].clone())
            e = rel(outs[0], want)
            print(f"{mesh_name} {variant} {name} damped={damped}: {e:.2e}")
            assert e < 1e-12, (name, damped, e)
            assert torch.equal(outs[0], outs[1])
        assert bool(torch.isnan(Ysbuf[n:]).all())
    # no load: F = NULL
    b = torch.empty(n, dtype=F64, device=A.device)
    _rhs(s, s.d, kv, la, 0.0, None, Y, b)
    assert rel(b, s.d * Y[:, 1] + Kyk) < 1e-12
    assert bool(torch.isnan(Ybuf[n:]).all()) and bool(torch.isnan(Fbuf[n:]).all())


# ---------------------------------------------------------------- 3. the vector update
@pytest.mark.parametrize("predictor", [False, True], ids=["warm", "predictor"])
@pytest.mark.parametrize("n", [375, 3993, 1024])
def test_newmark_update(gpu, n, predictor):
    from fem355 import _capi as C, system
    c = system.newmark_constants(1e-3, 0.3025, 0.6, (2.0, 1e-4))
    k = c["coef"]
    gen = torch.Generator().manual_seed(n)
    vec = lambda scale: _padded((torch.randn(n, dtype=F64, generator=gen) * scale).to(gpu), n)
    (xb, x), (ub, u), (vb, v), (ab, a) = vec(1.0), vec(1.0), vec(1e3), vec(1e6)
    w = torch.rand(n, dtype=F64, generator=gen)
    w[torch.rand(n, generator=gen) < 0.2] = 0.0
    w[-1] = 0.5
    wb, w = _padded(w.to(gpu), n)
    Yb = torch.full((n + 64, 2), float("nan"), dtype=F64, device=gpu)
    un, uo, vo, ao = x.clone(), u.clone(), v.clone(), a.clone()
    C.check(C.lib().fem_newmark_update(n, (ctypes.c_double * 12)(*k), 1 if predictor else 0, C.ptr(x), C.ptr(u),
                                       C.ptr(v), C.ptr(a), C.ptr(w), C.ptr(Yb), C.stream(torch.device(gpu))),
            "fem_newmark_update")
    Y = Yb[:n]
    for buf in (xb, ub, vb, ab, wb, Yb):
        assert bool(torch.isnan(buf[n:]).all())
    free = w != 0
    for t in (x, u, v, a, Y[:, 0], Y[:, 1]):
        assert not bool(t[~free].any())
        assert bool(torch.isfinite(t).all())

    def check(what, got, terms):
        want = sum(terms)
        mag = sum(t.abs() for t in terms)
        worst = float(((got - want).abs() / mag)[free].max() / EPS)
        print(f"n={n} {what}: {worst:.2f} x 2^-53 of the terms")
        assert worst <= 8.0, (what, worst)

    # every formula on the kernel's own inputs to it (a_new feeds v_new; both feed Y and the predictor)
    check("a", a, [k[0] * un, -k[0] * uo, -k[1] * vo, -k[2] * ao])
    check("v", v, [vo, k[3] * ao, k[4] * a])
    assert torch.equal(u[free], un[free])
    check("yM", Y[:, 1], [k[5] * u, k[6] * v, k[7] * a])
    check("yK", Y[:, 0], [k[8] * u, k[9] * v, k[10] * a])
    if predictor:
        check("x", x, [u, k[11] * v])
    else:
        assert torch.equal(x, u)


# ---------------------------------------------------------------- 4. the energy
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_name", MESHES)
def test_energy(kcase, mesh_name, variant):
    s = kcase(mesh_name, variant)
    x, y = s.randn(s.n), s.randn(s.n)
    xc, yc = x.cpu(), y.cpu()
    Kx = R.nodal_forces(s.Ke, s.el, xc.view(s.N, s.dpn)).reshape(-1)
    for name, mass in s.masses():
        My = mass.cpu() * yc if name == "diag" else R.nodal_forces(s.Me, s.el, yc.view(s.N, s.dpn)).reshape(-1)
        q = s.A.quadforms(mass, x, y)
        q2 = s.A.quadforms(mass, x, y)
        assert torch.equal(q, q2)
        q = q.cpu()
        eK = abs(float(q[0]) - float(torch.dot(xc, Kx))) / float(xc.norm() * Kx.norm())
        eM = abs(float(q[1]) - float(torch.dot(yc, My))) / float(yc.norm() * My.norm())
        print(f"{mesh_name} {variant} {name}: x^T K x {eK:.2e}, y^T M y {eM:.2e}")
        assert eK <= 1e-13 and eM <= 1e-13, (name, eK, eM)
        assert s.A.energy(mass, x, y) == 0.5 * float(s.A.quadforms(mass, x, y).sum())


# ---------------------------------------------------------------- 5. trajectories
SCENARIOS = ("mode", "damped", "step_load", "sine_load", "predictor")
CONSERVATIVE = ("mode", "predictor")


def _solve(gpu, name, scen, amplitude="tensor", **kw):
    from fem355 import solver
    cs = MR.case(name)
    sc = NR.scenario(cs, scen)
    dt = sc["dt"]
    shape = (cs.N, cs.dpn)
    args = dict(dt=dt, steps=NR.STEPS, rtol=1e-8, record=torch.arange(cs.N), energy_every=1, device=gpu,
                return_info=True, beta=sc.get("beta", 0.25), gamma=sc.get("gamma", 0.5),
                damping=(sc.get("alpha", 0.0), sc.get("beta_r", 0.0)), predictor=sc.get("predictor", False),
                lumped=cs.mass == "lumped")
    if "u0" in sc:
        args["u0"] = sc["u0"].view(shape)
    F = torch.zeros(shape, dtype=F64)
    if scen in ("step_load", "sine_load"):
        F = NR.load_vector(cs).view(shape)
    if scen == "sine_load":
        om = NR.mode(cs)[0]
        fn = lambda t: math.sin(0.7 * om * t)
        args["amplitude"] = (fn if amplitude == "callable"
                             else torch.tensor([fn(k * dt) for k in range(NR.STEPS + 1)], dtype=F64))
    args.update(kw)
    F = args.pop("F", F)
    M = cs.Me if cs.mass == "lumped" else cs.Ms
    return solver.transient_solver(cs.Ke, M, cs.el, F, cs.fixed, cs.N, **args)


@pytest.mark.parametrize("scen", SCENARIOS)
@pytest.mark.parametrize("name", NR.CASES)
def test_trajectory(gpu, name, scen):
    """64 solves on one context against the dense restatements (module docstring for the bounds)."""
    from fem355 import _capi as C
    cs = MR.case(name)
    d, p = NR.reference(name, scen, "direct"), NR.reference(name, scen, "pcg")
    u, v, a, res = _solve(gpu, name, scen)
    assert res.steps_done == NR.STEPS and res.converged and len(res.iterations) == NR.STEPS
    assert res.rec_u.shape == (NR.STEPS + 1, cs.N, cs.dpn)
    U = res.rec_u.reshape(NR.STEPS + 1, -1).cpu()
    assert torch.equal(U[-1], u.reshape(-1).cpu())
    assert not bool(U[:, ~cs.free].any())
    umax = float(d.u.abs().max())
    dev_g, dev_p = float((U - d.u).abs().max()) / umax, float((p.u - d.u).abs().max()) / umax
    floor = NR.STEPS * math.sqrt(cs.n) * EPS
    E = res.energies
    if scen in CONSERVATIVE:
        en_g, en_p = float((E - E[0]).abs().max() / E[0]), p.drift()
    else:
        emax = float(d.energy.max())
        en_g, en_p = float((E - d.energy).abs().max()) / emax, float((p.energy - d.energy).abs().max()) / emax
    print(f"{name} {scen}: iterations {min(res.iterations)}..{max(res.iterations)} (reference {min(p.iters)}.."
          f"{max(p.iters)}), deviation {dev_g:.2e} (PCG restatement {dev_p:.2e}, ratio {dev_g / dev_p:.2f}), "
          f"energy {en_g:.2e} (PCG restatement {en_p:.2e}, bound {8 * en_p + floor:.2e})")
    assert dev_p < 1e-5    # the comparison is not vacuous
    assert dev_g <= 8.0 * dev_p, (dev_g, dev_p)
    assert en_g <= 8.0 * en_p + floor, (en_g, en_p)
    assert all(s == C.PCG_CONVERGED for s in res.status)


def test_amplitude_tensor_and_callable_agree(gpu):
    a = _solve(gpu, "elastic4", "sine_load", "tensor")
    b = _solve(gpu, "elastic4", "sine_load", "callable")
    assert rel(a[3].rec_u, b[3].rec_u) <= 1e-12 and rel(a[0], b[0]) <= 1e-12
    # the full history [steps + 1, N, dpn] is the same load
    cs = MR.case("elastic4")
    om, dt = NR.mode(cs)[0], NR.step_size(cs)
    amps = torch.tensor([math.sin(0.7 * om * k * dt) for k in range(NR.STEPS + 1)], dtype=F64)
    hist = amps.view(-1, 1, 1) * NR.load_vector(cs).view(1, cs.N, cs.dpn)
    # (amp F rounds in torch here and inside the kernel there, so the PCG iterates differ at the solver tolerance:
    # the trajectory bound against the direct restatement applies, not bit equality)
    c = _solve(gpu, "elastic4", "step_load", F=hist)
    d, p = NR.reference("elastic4", "sine_load", "direct"), NR.reference("elastic4", "sine_load", "pcg")
    U = c[3].rec_u.reshape(NR.STEPS + 1, -1).cpu()
    assert float((U - d.u).abs().max()) <= 8.0 * float((p.u - d.u).abs().max())


# ---------------------------------------------------------------- 6. book-keeping
@pytest.mark.parametrize("name", ["elastic4", "poisson6"])
def test_one_context_one_effective_matrix(gpu, name, monkeypatch):
    from fem355 import _capi as C, system
    lib = C.lib()
    calls = {"fem_pcg_create": 0, "fem_sell_axpby_mass": 0, "fem_pcg_solve": 0, "sched": []}

    def wrap(fn_name):
        fn = getattr(lib, fn_name)

        def f(*args):
            calls[fn_name] += 1
            return fn(*args)
        monkeypatch.setattr(lib, fn_name, f)

    for fn_name in ("fem_pcg_create", "fem_sell_axpby_mass", "fem_pcg_solve"):
        wrap(fn_name)
    set_schedule = lib.fem_pcg_set_schedule
    monkeypatch.setattr(lib, "fem_pcg_set_schedule", lambda h, s: calls["sched"].append(s) or set_schedule(h, s))
    u1 = _solve(gpu, name, "mode", steps=16)
    assert calls["fem_pcg_create"] == 1 and calls["fem_sell_axpby_mass"] == 1 and calls["fem_pcg_solve"] == 16
    bs = MR.case(name).dpn
    assert calls["sched"] == [system.DEFAULT_SCHEDULE[bs]]
    assert system.DEFAULT_SCHEDULE[1] == system.SCHED_PERSIST and system.DEFAULT_SCHEDULE[3] == system.SCHED_AUTO
    u2 = _solve(gpu, name, "mode", steps=16)
    for x, y in zip(u1[:3], u2[:3]):
        assert torch.equal(x, y)
    assert torch.equal(u1[3].rec_a, u2[3].rec_a) and torch.equal(u1[3].energies, u2[3].energies)
    assert u1[3].iterations == u2[3].iterations


def test_non_convergence_stops_the_run(gpu, capsys):
    from fem355 import _capi as C
    cs = MR.case("elastic4")
    phi = NR.mode(cs)[1]
    u, v, a, res = _solve(gpu, "elastic4", "mode", max_iter=3)
    out = capsys.readouterr().out
    assert f"Transient solver: step 1 stopped with status 2 after {res.iterations[0]} iterations" in out
    assert res.steps_done == 0 and res.status == [C.PCG_MAXITER] and res.iterations == [3]
    assert res.rec_u.shape[0] == 1 and res.times.numel() == 1
    assert rel(u.reshape(-1), phi) <= 1e-15 and not bool(v.any())
    a0 = NR.reference("elastic4", "mode", "direct").a[0]
    assert rel(a.reshape(-1), a0) < 1e-9
