"""GPU tier of the third generation of element kernels on hard geometry: the explicit dynamics' internal force, strain
energy, lumped mass and stable step (csrc/explicit.hip: k_xd_force, k_xd_mass, k_xd_dt), the shell kernels
(csrc/shell.hip: k_shell_ke in its three modes, k_shell_geom, k_shell_stress, k_shell_apply) and the topology
optimisation's volumes, unit strain energy and scaled assembly (csrc/topopt.hip: k_tet4_vol, k_tet4_unit_energy; the
scaled c3d4 assembly of csrc/assemble.hip), judged by exact rational arithmetic (tests/exact_ref3.py). Their own tests
run well-shaped, positively oriented meshes of order one near the origin against fp64 restatements or recorded values.

c3d4 meshes and comparison are those of tests/test_gpu_hard_geometry.py: the seven half-flipped cases of
exact_ref.TET4_CASES (81 of 162 elements in local order [1, 0, 2, 3]), exact_ref.check asserting error <= 8 x
max(calibration error, 2.2e-16), nodal vectors per dof against the exact magnitude sum, per-node and per-element
positive values per entry, energies and the compliance as relative errors of one number. Calibration: the
restatements' formulas (hyperelastic_ref, explicit_ref, topopt_ref) on the fp64 edge-difference gradients and
|det| / 6. The nonlinear materials take exact_ref2.hyper_u (a finite-strain unit-mesh field pushed through the
case's linear map), the linear one exact_ref.tet4_u.

Shell patch (exact_ref3.shell_case): 9 x 8 quads of spacing 0.1 on z = 0.05 sin sin, nodes moved in-plane by 0.15 of
the spacing, so every quad is warped; 72 s4 elements (a full 64-element block and a ragged one) or 144 s3 (three
blocks, the last ragged); every second element's node list starts one place further round, so that its frame origin
and axes differ from its neighbours'. Cases: plain, shifts of 1e4 and 1e6, scales 1e-3 and 1e3, a squash to 1e4 : 1
slivers (y and the height z by 1e-4: y alone would leave the rise of the surface along the short edges and no sliver)
and the squash followed by exact_ref._orthogonal(). Material: the membrane / bending triples of
tests/golden/shell_cells.npz. Calibration: tests/shell_ref.py as it is. Element matrices are compared on 8 elements per
family (elements 0, 63, 64, the last, both start orders); frames, local coordinates, J, gradients, NMQ and the
operator on the whole patch. The operator takes shell_ref's local K and frames as its fp64 inputs, on both sides.

Fixed assertions (no tolerance): lumped mass and topopt volumes of the half-flipped mesh equal the unflipped mesh's
bit for bit; ExplicitDynamics.start reports ("OK", -1) on every flipped case and material (a negative reference det is
no inverted element); local and global shell K are symmetric bit for bit and the rows and columns of w and thz exact
zeros; every dt_e > 0 and finite, dt == min dt_e, and dt <= 2 / omega_max of the dense lumped-mass pencil where that
eigenproblem is well conditioned (flipped, shift1e4, scale1e-3, scale1e3); under a translation by the power of two
2^20 (1, -1, 1) of a mesh rounded to multiples of 2^-20 the internal forces, lumped mass, volumes, shell K and frames
are the unshifted run's bits; the |det| < 1e-12 threshold is accepted at 4e-12 and reported at 2.5e-13 the way each
path documents (explicit: ExplicitDynamics raises ValueError when it builds its element-chunk layout, so k_xd_force's
zero-force branch cannot be reached from a degenerate reference element; topopt: the element's index in the `bad`
word, zero ce / dct, and system.TopOpt raises ValueError).

Measured on the MI355X, as "error / ratio": the kernel's error against exact, and its ratio to max(calibration
error, 2.2e-16) (the tests assert ratio <= 8; the largest is 3.30, the neo-Hooke nodal force on the rotated sliver; the
calibration side is CPU arithmetic and moves in the last digit between hosts). The c3d4 kernels stay at 1e-15 at any
shift and scale and share the rotated sliver's 1e-12 with the edge form. The shell kernels do not see a shift at all
(edge differences) and lose on the 1e4 : 1 slivers exactly what shell_ref loses, 4e-12 for s3 and 6e-13 for s4 in the
frame already: the projection b - (a.b / a.a) a removes all but 1e-4 of b. That loss is the calibration's as well and
is recorded, not fixed. The operator, whose inputs are K and the frames, stays at 3e-16. "unit of K global" is the
frame shell_global_K returns. The two "scaled matvec" rows are the fresh solver layout and the plain-values-first
layout: the same bits. dt / (2 / omega_max) = 0.483 on the four cases where it is asserted.

  c3d4                             flipped     shift1e4     shift1e6    scale1e-3     scale1e3   squash1e-4   squash_rot
    xd linear force           6.5e-16/1.00 4.1e-16/0.63 4.4e-16/1.01 6.2e-16/0.60 8.2e-16/1.65 8.1e-16/1.24 7.3e-13/0.51
    xd linear energy          1.4e-16/0.64 0.0e+00/0.00 0.0e+00/0.00 1.3e-16/0.60 3.0e-16/1.38 1.9e-16/0.88 4.8e-15/0.10
    xd svk force              6.3e-16/0.59 5.7e-16/0.84 4.9e-16/0.59 5.2e-16/0.67 7.3e-16/1.21 7.4e-16/0.95 2.0e-12/0.46
    xd svk energy             2.0e-16/0.93 2.0e-16/0.93 2.0e-16/0.93 0.0e+00/0.00 0.0e+00/0.00 1.2e-16/0.56 6.2e-14/0.87
    xd neo_hookean force      2.5e-15/1.03 1.9e-15/0.49 3.2e-15/0.96 4.1e-15/2.72 2.9e-15/1.25 1.4e-15/0.50 6.5e-12/3.30
    xd neo_hookean energy     1.4e-16/0.63 1.4e-16/0.63 0.0e+00/0.00 1.3e-16/0.58 0.0e+00/0.00 1.7e-16/0.78 1.9e-14/0.66
    xd mass                   3.6e-16/1.01 3.6e-16/1.00 3.7e-16/1.11 3.4e-16/1.01 3.8e-16/1.75 4.4e-16/1.08 5.5e-13/0.76
    xd dt_e                   3.4e-16/1.00 4.3e-16/1.00 3.7e-16/1.00 3.2e-16/0.97 3.3e-16/0.96 4.4e-16/1.16 1.2e-12/0.77
    topopt volumes            3.0e-16/1.30 3.3e-16/0.75 2.8e-16/0.80 3.8e-16/0.94 2.7e-16/1.00 2.1e-16/0.80 1.2e-12/0.77
    topopt ce                 6.2e-16/0.90 6.7e-16/1.24 7.0e-16/1.38 6.5e-16/1.01 6.5e-16/1.11 9.2e-16/1.00 1.2e-12/0.77
    topopt dct                7.3e-16/0.88 7.5e-16/1.10 7.1e-16/0.91 6.8e-16/1.11 6.2e-16/0.98 9.1e-16/0.90 1.2e-12/0.77
    topopt compliance         0.0e+00/0.00 2.1e-16/0.97 0.0e+00/0.00 2.0e-16/0.91 0.0e+00/0.00 1.4e-16/0.63 1.0e-14/0.44
    topopt scaled matvec fresh 2.9e-16/1.18 4.4e-16/1.82 3.4e-16/1.56 2.8e-16/1.17 2.9e-16/0.73 6.8e-16/1.62 5.0e-13/0.40
    topopt scaled matvec plain 2.9e-16/1.18 4.4e-16/1.82 3.4e-16/1.56 2.8e-16/1.17 2.9e-16/0.73 6.8e-16/1.62 5.0e-13/0.40

  shells                             plain     shift1e4     shift1e6    scale1e-3     scale1e3   squash1e-4   squash_rot
    s3 unit                   4.5e-16/1.00 4.0e-16/1.00 4.2e-16/1.00 4.3e-16/1.00 3.1e-16/1.00 3.7e-12/1.00 3.1e-12/1.00
    s3 local                  5.4e-16/1.00 5.2e-16/1.00 4.3e-16/0.83 4.9e-16/1.00 4.3e-16/1.00 3.7e-12/1.00 3.1e-12/1.00
    s3 J                      5.4e-16/1.00 5.2e-16/1.00 4.3e-16/0.83 4.9e-16/1.00 4.3e-16/1.00 3.7e-12/1.00 3.1e-12/1.00
    s3 grads                  6.4e-16/0.92 6.8e-16/0.97 6.1e-16/0.90 6.0e-16/0.98 6.0e-16/1.05 3.7e-12/1.00 3.4e-12/1.00
    s4 unit                   2.3e-16/1.00 1.7e-16/0.76 2.3e-16/1.00 2.3e-16/1.00 2.3e-16/1.01 5.5e-13/1.00 4.3e-13/1.00
    s4 local                  2.8e-16/1.00 2.7e-16/1.00 2.6e-16/1.01 2.8e-16/1.00 3.1e-16/1.00 5.5e-13/1.00 4.4e-13/1.00
    s4 J                      3.0e-16/1.00 3.1e-16/1.03 3.8e-16/1.29 3.0e-16/1.00 3.1e-16/1.00 5.5e-13/1.00 4.4e-13/1.00
    s4 grads                  5.3e-16/1.15 6.1e-16/1.11 6.3e-16/1.16 5.0e-16/1.00 6.2e-16/1.33 5.5e-13/1.00 8.7e-13/1.00
    s3 K                      7.1e-16/1.20 7.2e-16/0.95 7.5e-16/0.78 7.7e-16/0.80 6.5e-16/0.88 4.8e-12/1.00 5.0e-12/1.00
    s3 K global               6.7e-16/0.93 7.2e-16/0.92 8.1e-16/0.82 1.0e-15/0.82 6.7e-16/0.65 6.1e-12/1.00 5.1e-12/1.00
    s3 unit of K global       4.5e-16/1.00 4.0e-16/1.00 4.2e-16/1.00 4.3e-16/1.00 3.1e-16/1.00 3.7e-12/1.00 3.1e-12/1.00
    s4 K                      4.5e-16/0.69 4.8e-16/1.00 5.2e-16/1.33 4.5e-16/1.00 7.9e-16/1.00 7.5e-13/1.00 6.9e-13/1.00
    s4 K points               6.3e-16/1.00 4.8e-16/1.00 6.1e-16/0.97 6.1e-16/1.00 9.5e-16/1.00 9.8e-13/1.00 7.3e-13/0.79
    s4 K global               7.3e-16/1.00 6.9e-16/1.07 6.0e-16/0.90 7.3e-16/1.05 6.9e-16/1.00 7.5e-13/1.00 7.0e-13/0.74
    s4 unit of K global       2.3e-16/1.00 1.7e-16/0.76 2.3e-16/1.00 2.3e-16/1.00 2.3e-16/1.01 5.5e-13/1.00 4.3e-13/1.00
    s3 NMQ                    1.1e-15/1.00 1.0e-15/1.27 1.1e-15/1.00 1.5e-15/1.33 8.8e-16/0.92 6.8e-12/1.00 5.0e-12/1.00
    s3 operator               2.4e-16/1.00 2.4e-16/1.00 2.7e-16/0.94 3.5e-16/1.61 2.3e-16/0.95 3.4e-16/0.93 2.7e-16/1.01
    s4 NMQ                    5.4e-16/0.74 6.3e-16/1.32 5.6e-16/0.89 5.0e-16/0.93 1.0e-15/1.50 8.2e-13/1.00 2.4e-12/1.00
    s4 operator               2.0e-16/0.91 2.0e-16/0.81 2.5e-16/1.00 1.9e-16/0.78 1.8e-16/0.83 3.3e-16/1.28 3.1e-16/0.95

One fixed assertion found a kernel change, test_mass_and_volumes_do_not_depend_on_the_local_order: see its docstring
(the mass and volume rows above are from after it). The explicit threshold case is refused before any kernel runs:
see test_threshold_explicit_refuses.
"""
import pytest
import torch

import exact_ref as X
import exact_ref3 as X3
import explicit_ref as XR
from test_gpu_nonlinear import nan_padded

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
PAD = 3
E, NU, RHO = X3.E, X3.NU, X3.RHO
PENAL, S_MIN = X3.PENAL, X3.S_MIN
OMEGA_CASES = ("flipped", "shift1e4", "scale1e-3", "scale1e3")
POW2_SHIFT = 2.0 ** 20 * torch.tensor([1.0, -1.0, 1.0], dtype=F64)


def _mods():
    import fem355  # noqa: F401
    from fem355 import shell, system
    return shell, system


def _xd(gpu, c, t, material):
    _, system = _mods()
    return system.ExplicitDynamics(c.to(gpu), t.to(gpu), RHO, E, NU, material)


def _grid(c):
    """Coordinates rounded to multiples of 2^-20: a translation by POW2_SHIFT is then exact, and so is every edge."""
    return torch.round(c * 2.0 ** 20) / 2.0 ** 20


# ----------------------------------------------------------------------------- explicit dynamics
@pytest.mark.parametrize("material", X3.XD_MATERIALS)
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_explicit_force_and_energy(gpu, case, material):
    """k_xd_force: the assembled internal force per dof and the strain energy of an energy step against exact; the
    half-flipped mesh starts with status OK (xd_element divides the cofactors by the signed det and takes V = |det|)."""
    c, t = X.tet4_case(case)
    u = X3.xd_u(case, material)
    f_ex, mag, w_ex = X3.tet4_exact3(case, "xd_" + material)
    xd = _xd(gpu, c, t, material)
    try:
        f = xd.internal_force(u.to(gpu)).view(-1, 3)
        X.check(f"xd {material} force {case}", X.dof_err(f, f_ex, mag),
                X3.tet4_calibration_err3(case, "xd_" + material, "f"))
        xd.start(u0=u.to(gpu))
        assert xd.status() == ("OK", -1)
        # the energy row of step 0 is W(u0), whatever the step then does to an unbalanced finite-strain state
        res = xd.run(1, 1e-6 * xd.stable_dt()[0], energy_every=1)
        assert res.strain.numel() == 1
        X.check(f"xd {material} energy {case}", X3.rel_err(res.strain[0], w_ex),
                X3.tet4_calibration_err3(case, "xd_" + material, "w"))
    finally:
        xd.close()


@pytest.mark.parametrize("case", X.TET4_CASES)
def test_explicit_mass_and_step(gpu, case):
    """k_xd_mass and k_xd_dt against exact; every dt_e positive and finite, dt their minimum, and dt below the dense
    2 / omega_max where that eigenproblem is well conditioned."""
    c, t = X.tet4_case(case)
    xd = _xd(gpu, c, t, "linear")
    try:
        X.check(f"xd mass {case}", X3.node_err(xd.mass, X3.tet4_exact3(case, "mass")),
                X3.tet4_calibration_err3(case, "mass"))
        dt, dte = xd.stable_dt()
        X.check(f"xd dt_e {case}", X3.node_err(dte, X3.tet4_exact3(case, "dt")), X3.tet4_calibration_err3(case, "dt"))
        dte = dte.cpu()
        assert bool((dte > 0).all()) and bool(torch.isfinite(dte).all()) and dte.numel() == t.shape[0]
        assert dt == float(dte.min())
        if case in OMEGA_CASES:
            bound = 2.0 / XR.omega_max(c, t, E, NU, RHO)
            print(f"HARDGEOM xd dt {case}: dt {dt:.6e} 2 / omega_max {bound:.6e} ratio {dt / bound:.3f}")
            assert dt <= bound
    finally:
        xd.close()


def _raw_volumes(gpu, c, t):
    """fem_tet4_volumes on arrays with NaN / zero tails past N and M -> (V [M] on the host, the `bad` word)."""
    from fem355 import _capi as C
    _, system = _mods()
    lib = C.lib()
    N, M = c.shape[0], t.shape[0]
    cd = nan_padded(c, gpu)
    td = torch.cat([t, torch.zeros((PAD, 4), dtype=torch.long)]).to(gpu)
    g = system.build_graph(t.to(gpu), N)
    V = torch.full((M + PAD,), NAN, dtype=F64, device=gpu)
    Vn = torch.full((N + PAD,), NAN, dtype=F64, device=gpu)
    bad = torch.full((1,), M, dtype=torch.int64, device=gpu)
    C.check(lib.fem_tet4_volumes(C.ptr(cd), C.ptr(td), M, C.ptr(g.inc_ptr), C.ptr(g.inc), N, C.ptr(V), C.ptr(Vn),
                                 C.ptr(bad), C.stream(torch.device(gpu))), "fem_tet4_volumes")
    torch.cuda.synchronize()
    assert bool(torch.isnan(V[M:]).all()) and bool(torch.isnan(Vn[N:]).all()) and not bool(torch.isnan(V[:M]).any())
    return V[:M].cpu(), int(bad.item())


def _raw_energy(gpu, c, t, u, rho_t):
    """fem_tet4_unit_energy the same way -> (ce [M], dct [M], compliance, the `bad` word)."""
    from fem355 import _capi as C
    lib = C.lib()
    N, M = c.shape[0], t.shape[0]
    cd, ud, rd = nan_padded(c, gpu), nan_padded(u.view(N, 3), gpu), nan_padded(rho_t, gpu)
    td = torch.cat([t, torch.zeros((PAD, 4), dtype=torch.long)]).to(gpu)
    full = lambda n: torch.full((n,), NAN, dtype=F64, device=gpu)
    ce, dct, comp = full(M + PAD), full(M + PAD), full(1 + PAD)
    work = full(int(lib.fem_topopt_work_len(M)) + PAD)
    bad = torch.full((1,), M, dtype=torch.int64, device=gpu)
    C.check(lib.fem_tet4_unit_energy(C.ptr(cd), C.ptr(td), M, C.ptr(ud), NU, C.ptr(rd), PENAL, S_MIN, E, C.ptr(ce),
                                     C.ptr(dct), C.ptr(work), C.ptr(comp), C.ptr(bad), C.stream(torch.device(gpu))),
            "fem_tet4_unit_energy")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ce[M:]).all()) and bool(torch.isnan(dct[M:]).all()) and bool(torch.isnan(comp[1:]).all())
    return ce[:M].cpu(), dct[:M].cpu(), float(comp[0]), int(bad.item())


def test_mass_and_volumes_do_not_depend_on_the_local_order(gpu):
    """The lumped mass and the topopt volumes of the half-flipped mesh are the unflipped mesh's, bit for bit: |det| is a
    symmetric function of an element's nodes, and a mass or a volume that moves when an element's nodes are listed in
    another order is the defect test_tet4_mass_reordered_identical found in the consistent mass.

    Found: with |det| formed from the edges out of local node 0 (xd_cofactors in k_xd_mass, tet4_grads in k_tet4_vol)
    the order [1, 0, 2, 3] differences other edges and |det| rounds differently in the last bit: 41 of the 162 volumes
    differed (all among the 81 reordered elements), by at most 4.36e-16 relative, and 16 of the 64 lumped masses, by
    at most 2.58e-16. k_tet4_vol now calls tet4_det_sorted, and k_xd_mass sorts the element's four local node ids
    (a chunk's local nodes ascend by global id) and forms det from the LDS-resident points in that order: 0 of 162
    and 0 of 64 differ."""
    c, t = X.tet4_case("flipped")
    c0, t0 = X.tet4_case("unflipped")
    xf, x0 = _xd(gpu, c, t, "linear"), _xd(gpu, c0, t0, "linear")
    try:
        mf, m0 = xf.mass.cpu(), x0.mass.cpu()
    finally:
        xf.close()
        x0.close()
    Vf, V0 = _raw_volumes(gpu, c, t)[0], _raw_volumes(gpu, c0, t0)[0]
    for name, a, b in (("lumped mass", mf, m0), ("volumes", Vf, V0)):
        d = (a - b).abs() / b
        print(f"HARDGEOM {name} flipped vs unflipped: {int((d > 0).sum())} of {d.numel()} entries differ, "
              f"max rel {float(d.max()):.2e}")
    assert torch.equal(Vf[0::2], V0[0::2])
    assert torch.equal(mf, m0)
    assert torch.equal(Vf, V0)


# ----------------------------------------------------------------------------- topology optimisation
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_topopt_volumes_and_energy(gpu, case):
    """k_tet4_vol and k_tet4_unit_energy through the raw entry points: volumes, ce, dct and the compliance."""
    c, t = X.tet4_case(case)
    cal = lambda q, part=None: X3.tet4_calibration_err3(case, q, part)
    V, bad = _raw_volumes(gpu, c, t)
    assert bad == t.shape[0] and bool((V > 0).all())
    X.check(f"topopt volumes {case}", X3.node_err(V, X3.tet4_exact3(case, "vol")), cal("vol"))
    ce, dct, comp, bad = _raw_energy(gpu, c, t, X.tet4_u(case), X3.to_rho_t(t.shape[0]))
    ce_ex, dct_ex, c_ex = X3.tet4_exact3(case, "energy")
    assert bad == t.shape[0]
    X.check(f"topopt ce {case}", X3.node_err(ce, ce_ex), cal("energy", "ce"))
    X.check(f"topopt dct {case}", X3.node_err(dct, dct_ex), cal("energy", "dct"))
    X.check(f"topopt compliance {case}", X3.rel_err(comp, c_ex), cal("energy", "c"))


@pytest.mark.parametrize("mode", ["fresh", "plain"])
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_topopt_scaled_assembly(gpu, case, mode):
    """The bs = 3 scaled assembly with the device's SIMP scale of the seeded rho_t (k_simp_scale): its product per dof
    against exact, in the solver layout a fresh matrix takes and with the plain values requested first."""
    from fem355 import _capi as C
    _, system = _mods()
    c, t = X.tet4_case(case)
    M = t.shape[0]
    rho_t = X3.to_rho_t(M).to(gpu)
    s = torch.empty(M, dtype=F64, device=gpu)
    C.check(C.lib().fem_simp_scale(C.ptr(rho_t), M, PENAL, S_MIN, C.ptr(s), C.stream(torch.device(gpu))),
            "fem_simp_scale")
    A = system.SellMatrix(system.build_graph(t.to(gpu), c.shape[0]), 3)
    if mode == "plain":
        A.vals
    A.add_tet4(c.to(gpu), t.to(gpu), E, NU, scale=s)
    A.check_singular()
    y_ex, mag = X3.tet4_exact3(case, "matvec")
    y = A.matvec(X.tet4_x(case, "elastic").reshape(-1).to(gpu))
    X.check(f"topopt scaled matvec {mode} {case}", X.dof_err(y, y_ex, mag), X3.tet4_calibration_err3(case, "matvec"))


# ----------------------------------------------------------------------------- c3d4: translation and threshold
def test_c3d4_power_of_two_translation_is_exact(gpu):
    """The half-flipped mesh on the 2^-20 grid, moved by 2^20 (1, -1, 1): every edge difference is the same number, so
    the internal forces, the lumped mass and the volumes are the unshifted run's bits."""
    c, t = X.tet4_case("flipped")
    c = _grid(c)
    cs = c + POW2_SHIFT
    assert torch.equal(cs - POW2_SHIFT, c)
    for material in X3.XD_MATERIALS:
        u = X3.xd_u("flipped", material).to(gpu)
        a, b = _xd(gpu, c, t, material), _xd(gpu, cs, t, material)
        try:
            assert torch.equal(a.internal_force(u), b.internal_force(u)), material
            assert torch.equal(a.mass, b.mass)
        finally:
            a.close()
            b.close()
    assert torch.equal(_raw_volumes(gpu, c, t)[0], _raw_volumes(gpu, cs, t)[0])


def _threshold_u(c, material, with_singular):
    """The case "flipped"'s field scaled to the threshold mesh; the inserted element's own four nodes move by 1e-3 of
    its size (were they at rest a force from it would be zero whatever the kernel did)."""
    cf, _ = X.tet4_case("flipped")
    s = float(c[:64].abs().max() / cf.abs().max())
    u = s * X3.xd_u("flipped", material)
    if with_singular:
        g = torch.Generator().manual_seed(71)
        u = torch.cat([u, 1e-3 * 2.5e-13 ** (1.0 / 3.0) * torch.randn(4, 3, dtype=F64, generator=g)])
    return u.contiguous()


def test_threshold_accepts(gpu):
    """min |det| = 4e-12, above the absolute |det| < 1e-12 test: the explicit force of every material starts OK, and
    neither k_tet4_vol nor the unit energy names an element."""
    c, t = X.threshold_case(False)
    for material in X3.XD_MATERIALS:
        xd = _xd(gpu, c, t, material)
        try:
            xd.start(u0=_threshold_u(c, material, False).to(gpu))
            assert xd.status() == ("OK", -1), material
        finally:
            xd.close()
    assert _raw_volumes(gpu, c, t)[1] == t.shape[0]
    ce, _, _, bad = _raw_energy(gpu, c, t, _threshold_u(c, "linear", False), X3.to_rho_t(t.shape[0]))
    assert bad == t.shape[0] and bool((ce > 0).all())


@pytest.mark.parametrize("material", X3.XD_MATERIALS)
def test_threshold_explicit_refuses(gpu, material):
    """One tet of |det| = 2.5e-13 on four nodes of its own at element 140: ExplicitDynamics refuses the mesh when it
    builds its element-chunk layout (fem_mf_create applies the absolute |det| < 1e-12 test, ValueError "Singular"),
    for every material. k_xd_force's own rule for a degenerate reference element -- zero force and the status word
    lowered to the step -- therefore cannot be reached from a reference mesh through this class; the same branch is
    taken for det F <= 0, which tests/test_gpu_explicit.py drives with an inverting u0 (INVERTED at step 0, the other
    elements' forces right)."""
    c, t = X.threshold_case(True)
    with pytest.raises(ValueError, match="Singular"):
        _xd(gpu, c, t, material)
        pytest.fail("ExplicitDynamics accepted a singular element")


def test_threshold_topopt_reports(gpu):
    """topopt.hip: the lowest degenerate element's index goes to the `bad` word of k_tet4_vol and of the unit energy,
    which writes ce = dct = 0 for it; system.TopOpt raises ValueError when its volumes name an element."""
    _, system = _mods()
    c, t = X.threshold_case(True)
    M = t.shape[0]
    V, bad = _raw_volumes(gpu, c, t)
    assert bad == 140 and bool((V > 0).all())
    ce, dct, comp, bad = _raw_energy(gpu, c, t, _threshold_u(c, "linear", True), X3.to_rho_t(M))
    assert bad == 140 and float(ce[140]) == 0.0 and float(dct[140]) == 0.0
    keep = torch.arange(M) != 140
    assert bool((ce[keep] > 0).all()) and comp == comp
    F = torch.zeros(c.shape[0], 3, dtype=F64)
    F[0, 2] = -1.0
    mask = torch.zeros(3 * c.shape[0], dtype=torch.uint8)
    mask[-12:] = 1
    with pytest.raises(ValueError, match="Singular"):
        system.TopOpt(c.to(gpu), t.to(gpu), F.to(gpu), mask.to(gpu), E, NU, 0.5)


# ----------------------------------------------------------------------------- shells
def _geom(sh, c, conn, gpu):
    f = None if conn.shape[1] == 3 else X3.shell_geom_factors()
    unit, local, J, grads, _ = sh._shell_geom(c, conn, gpu, f, unit=True, local=True, J=True, grads=True)
    return unit, local, J, grads


def _local_K(sh, c, conn, gpu, single=True):
    mem, ben = X3.shell_params()
    if conn.shape[1] == 3:
        return sh.compute_s3_K_matrix(c, conn, mem, ben, device=gpu, dtype=F64)
    return sh.compute_s4_K_matrix(c, conn, mem, ben, single=single, device=gpu, dtype=F64)


def _dead_rows_are_zero(K, npe):
    dof = torch.arange(6 * npe) % 6
    dead = (dof == 2) | (dof == 5)
    return bool((K[:, dead] == 0).all()) and bool((K[:, :, dead] == 0).all())


@pytest.mark.parametrize("case", X3.SHELL_CASES)
@pytest.mark.parametrize("etype", X3.SHELL_TYPES)
def test_shell_geometry(gpu, etype, case):
    """k_shell_geom on the whole patch: the frame, the local coordinates (all three; a warped s4 has local z != 0 and
    J takes x and y only), J and the gradients at a point."""
    sh, _ = _mods()
    c, conn = X3.shell_case(etype, case)
    ex = X3.shell_exact(etype, case, "geom")
    for part, got, want in zip(X3.SHELL_GEOM_PARTS, _geom(sh, c, conn, gpu), ex):
        X.check(f"{etype} {part} {case}", X.elem_err(got, want), X3.shell_calibration_err(etype, case, "geom", part))


@pytest.mark.parametrize("case", X3.SHELL_CASES)
@pytest.mark.parametrize("etype", X3.SHELL_TYPES)
def test_shell_K(gpu, etype, case):
    """k_shell_ke in its three modes: local K, the four points' terms (s4) and the global-frame K in block order on
    the 8-element sample; on the whole patch local and global K symmetric bit for bit and the rows and columns of w
    and thz exact zeros."""
    sh, _ = _mods()
    c, conn = X3.shell_case(etype, case)
    npe = conn.shape[1]
    s = torch.tensor(X3.SHELL_SAMPLE[etype])
    K_ex, P_ex, G_ex = X3.shell_exact(etype, case, "K")
    cal = lambda part: X3.shell_calibration_err(etype, case, "K", part)
    K = _local_K(sh, c, conn, gpu).cpu()
    assert torch.equal(K, K.transpose(1, 2)) and _dead_rows_are_zero(K, npe)
    X.check(f"{etype} K {case}", X.elem_err(K[s], K_ex), cal("K"))
    if etype == "s4":
        P = _local_K(sh, c, conn, gpu, single=False).cpu()
        for p in range(4):
            assert torch.equal(P[..., p], P[..., p].transpose(1, 2)) and _dead_rows_are_zero(P[..., p], npe)
        X.check(f"{etype} K points {case}", X.elem_err(P[s], P_ex), cal("points"))
    Kg, unit = sh.shell_global_K(c, conn, *X3.shell_params(), device=gpu)
    Kg = Kg.cpu()
    assert torch.equal(Kg, Kg.transpose(1, 2))
    X.check(f"{etype} K global {case}", X.elem_err(Kg[s], G_ex), cal("global"))
    X.check(f"{etype} unit of K global {case}", X.elem_err(unit, X3.shell_exact(etype, case, "geom")[0]),
            X3.shell_calibration_err(etype, case, "geom", "unit"))


@pytest.mark.parametrize("case", X3.SHELL_CASES)
@pytest.mark.parametrize("etype", X3.SHELL_TYPES)
def test_shell_stress_and_operator(gpu, etype, case):
    """k_shell_stress (NMQ per element) and k_shell_apply (y = sum_e R_e^T K_e R_e u per dof against the magnitude
    sum) on the whole patch."""
    sh, _ = _mods()
    c, conn = X3.shell_case(etype, case)
    mem, ben = X3.shell_params()
    u = X3.shell_u()
    fn = sh.compute_s3_shell_stress if etype == "s3" else sh.compute_s4_shell_stress
    nmq = fn(c, conn, mem, ben, u, device=gpu, dtype=F64)
    X.check(f"{etype} NMQ {case}", X.elem_err(nmq, X3.shell_exact(etype, case, "stress")),
            X3.shell_calibration_err(etype, case, "stress"))
    K, unit = X3.shell_apply_inputs(etype, case)
    y = sh.compute_shell_nodal_forces(K, conn, u, unit, device=gpu, dtype=F64)
    y_ex, mag = X3.shell_exact(etype, case, "apply")
    X.check(f"{etype} operator {case}", X.dof_err(y, y_ex, mag), X3.shell_calibration_err(etype, case, "apply"))


@pytest.mark.parametrize("etype", X3.SHELL_TYPES)
def test_shell_power_of_two_translation_is_exact(gpu, etype):
    """shell_frame takes edge differences only: the patch on the 2^-20 grid moved by 2^20 (1, -1, 1) gives the same
    bits in the local K, the points' terms, the global K, the frames and the local coordinates."""
    sh, _ = _mods()
    c, conn = X3.shell_case(etype, "plain")
    c = _grid(c)
    cs = c + POW2_SHIFT
    assert torch.equal(cs - POW2_SHIFT, c)
    assert torch.equal(_local_K(sh, c, conn, gpu), _local_K(sh, cs, conn, gpu))
    if etype == "s4":
        assert torch.equal(_local_K(sh, c, conn, gpu, single=False), _local_K(sh, cs, conn, gpu, single=False))
    mem, ben = X3.shell_params()
    (Ka, ua), (Kb, ub) = sh.shell_global_K(c, conn, mem, ben, device=gpu), sh.shell_global_K(cs, conn, mem, ben, device=gpu)
    assert torch.equal(Ka, Kb) and torch.equal(ua, ub)
    for a, b in zip(_geom(sh, c, conn, gpu), _geom(sh, cs, conn, gpu)):
        assert torch.equal(a, b)
