"""GPU tier of the element kernels on hard geometry: inverted, shifted, tiny, huge and sliver elements, judged by
exact rational arithmetic (tests/exact_ref.py), not by the oracle -- the oracle's inv([1 x y z]) form loses accuracy
with distance from the origin (tests/test_exact_ref_cpu.py).

Meshes (exact_ref.tet4_case / iso_case): c3d4 kuhn_cube(3, jitter 0.15), 162 tets (three 64-element blocks of
k_tet4_ke, the last ragged) with every second element's local order [1, 0, 2, 3] (81 negative dets), then shifted by
1e4 / 1e6 (1, -0.7, 0.3), scaled by 1e-3 / 1e3, squashed by 1e-4 in z, and squashed then rotated; c3d8 / c3d6 boxes with
every second element reordered so that detJ < 0 at all its points, c3d10 followed by a z-mirrored copy (detJ > 0),
each plain, shifted by 1e3 / 1e6 and squashed (exact sample: 8 elements, 4 of each sign; the kernels run the mesh).

Comparison (exact_ref.check): element quantities by the per-element relative error max|a - b| / max|b|, assembled
products per dof against the magnitude sum, |y - y_exact| <= tol (sum_e |K_e| |x_e|)_dof. tol = 8 x max(calibration
error, 2.2e-16), computed in the test: the calibration error is that of the fp64 edge-difference form against exact
for c3d4 and of the oracle against exact for the isoparametric families (it shares the kernels' absolute-coordinate
Jacobian). Margin 8 covers another summation order, FMA contraction and the 1-ulp reciprocal of the matrix-free
element; two CPU orderings differ by < 1.5 x.

Fixed assertions: mass matrices are bit-identical between a mesh and its mirrored copy; the isoparametric stiffness
takes the sign of detJ (c3d6 single=True, B^T D B times an absolute volume, stays positive); a mesh with min|det| =
4e-12 is accepted by every c3d4 path and one tet of |det| = 2.5e-13 inside it makes every path raise (the geometric
stiffness and the body force document another rule, which is asserted as documented).

Measured on the MI355X, as "error / ratio": the kernel's error against exact, and its ratio to max(calibration
error, 2.2e-16) (the tests assert ratio <= 8; the largest is 2.11; the calibration side is CPU arithmetic and moves in
the last digit between hosts). No measured case needed a kernel change: the isoparametric kernels lose accuracy under a shift
exactly as the oracle does (1e-13 relative at 1e3, 1e-10 at 1e6), the c3d4 kernels stay at 1e-15 at any shift, and
the rotated sliver costs every c3d4 path the same 1e-12 as the fp64 edge form (the cancellation in det).

  c3d4                           flipped     shift1e4     shift1e6    scale1e-3     scale1e3   squash1e-4   squash_rot
    K_elastic                 5.4e-16/1.05 5.8e-16/1.01 7.1e-16/1.36 4.6e-16/0.87 4.7e-16/0.74 5.7e-16/0.81 1.2e-12/0.77
    K_poisson                 7.5e-16/1.36 5.6e-16/0.94 5.8e-16/1.40 4.1e-16/1.00 5.7e-16/1.09 5.8e-16/1.00 1.2e-12/0.77
    K_mass                    3.5e-16/0.91 3.8e-16/0.75 2.6e-16/0.75 3.5e-16/0.98 2.8e-16/0.77 2.4e-16/0.72 1.2e-12/0.77
    volumes                   3.0e-16/1.30 3.3e-16/0.75 2.2e-16/0.61 2.8e-16/0.68 2.7e-16/1.00 2.1e-16/0.80 1.2e-12/0.77
    B                         3.1e-16/1.00 3.1e-16/0.67 3.1e-16/1.00 3.1e-16/0.97 3.0e-16/1.05 2.7e-16/1.00 1.2e-12/0.77
    stress                    6.8e-16/1.14 6.5e-16/0.89 8.2e-16/1.06 7.4e-16/1.17 6.3e-16/1.00 7.5e-16/1.23 1.2e-12/0.77
    von Mises                 5.5e-16/1.09 6.6e-16/0.88 7.3e-16/1.30 5.7e-16/1.04 5.5e-16/0.83 6.1e-16/0.92 1.2e-12/0.77
    K_e-asm elastic jacobi    4.5e-16/1.00 4.5e-16/1.02 4.2e-16/0.75 4.5e-16/1.00 4.3e-16/0.99 4.6e-16/0.81 6.7e-13/0.47
    K_e-asm elastic matvec    3.0e-16/1.36 3.0e-16/1.36 3.8e-16/1.72 2.4e-16/1.00 3.7e-16/1.70 5.3e-16/1.24 5.0e-13/0.40
    K_e-asm poisson jacobi    3.1e-16/1.09 5.7e-16/1.83 3.0e-16/1.03 5.8e-16/1.32 2.8e-16/0.80 4.1e-16/1.12 6.7e-13/0.47
    K_e-asm poisson matvec    2.9e-16/1.00 3.0e-16/1.37 3.8e-16/1.37 3.6e-16/1.27 3.4e-16/0.67 3.2e-16/1.27 6.3e-13/0.57
    fused elastic jacobi      3.0e-16/0.66 4.4e-16/1.00 3.4e-16/0.61 4.4e-16/0.99 3.6e-16/0.82 4.6e-16/0.81 6.7e-13/0.47
    fused elastic matvec      2.5e-16/1.15 3.0e-16/1.36 3.8e-16/1.72 2.1e-16/0.84 3.7e-16/1.70 5.1e-16/1.19 5.0e-13/0.40
    fused poisson jacobi      3.1e-16/1.09 5.7e-16/1.83 3.0e-16/1.03 5.8e-16/1.32 2.8e-16/0.80 4.1e-16/1.12 6.7e-13/0.47
    fused poisson matvec      2.9e-16/1.00 3.0e-16/1.37 3.8e-16/1.37 3.6e-16/1.27 3.4e-16/0.67 3.2e-16/1.27 6.3e-13/0.57
    fused vs K_e-asm elastic  2.6e-16/1.20 1.9e-16/0.86 1.9e-16/0.86 2.4e-16/1.01 3.0e-16/1.36 3.8e-16/0.89 2.3e-16/0.00
    fused vs K_e-asm poisson  1.0e-16/0.35 1.9e-16/0.87 9.0e-17/0.32 1.4e-16/0.50 9.0e-17/0.18 0.0e+00/0.00 5.5e-17/0.00
    matfree elastic diag      6.5e-16/1.43 3.6e-16/0.83 3.7e-16/0.66 5.0e-16/1.12 3.8e-16/0.87 5.1e-16/0.89 6.7e-13/0.47
    matfree elastic matvec    3.1e-16/1.43 2.3e-16/1.04 2.1e-16/0.95 1.9e-16/0.77 1.8e-16/0.83 4.4e-16/1.02 5.0e-13/0.40
    matfree poisson diag      3.6e-16/1.26 3.5e-16/1.13 3.4e-16/1.15 3.4e-16/0.77 3.6e-16/1.03 2.4e-16/0.65 6.7e-13/0.47
    matfree poisson matvec    2.1e-16/0.71 2.9e-16/1.33 2.9e-16/1.05 2.8e-16/0.98 4.0e-16/0.77 2.5e-16/1.00 6.3e-13/0.57
  (K_e-asm: SellMatrix.add_element_matrices of the GPU's element matrices; fused: assemble_tet4_system.)

  isoparametric                    plain     shift1e3     shift1e6   squash1e-4
    c3d8 K single             5.8e-16/1.01 4.0e-13/0.76 5.4e-10/0.74 6.8e-16/0.85
    c3d8 K multi              7.7e-16/1.02 5.0e-13/0.57 7.5e-10/0.99 9.0e-16/0.81
    c3d8 mass                 5.9e-16/0.66 3.9e-13/0.92 2.7e-10/0.64 6.3e-16/0.89
    c3d8 stress               3.0e-16/1.37 4.4e-13/2.11 4.8e-10/0.75 3.0e-16/0.25
    c3d8 von Mises            3.1e-16/1.06 8.7e-14/0.85 8.9e-11/0.88 4.5e-16/0.81
    c3d8 Jacobian             2.7e-16/0.80 2.8e-13/1.08 2.9e-10/0.83 2.7e-16/1.23
    c3d8 gradients            3.5e-16/0.60 3.0e-13/0.84 5.6e-10/1.09 6.0e-16/1.53
    c3d6 K single             5.7e-16/0.90 3.3e-13/0.51 4.5e-10/0.98 1.2e-15/1.28
    c3d6 K multi              3.9e-16/0.75 2.3e-13/0.93 2.5e-10/0.86 6.4e-16/0.53
    c3d6 mass                 3.9e-16/0.67 2.3e-13/0.45 2.0e-10/0.84 4.7e-16/0.80
    c3d6 stress               4.8e-16/1.08 2.7e-13/1.25 1.6e-10/1.15 3.4e-16/0.31
    c3d6 von Mises            4.3e-16/0.71 1.1e-13/1.45 6.9e-11/1.28 2.1e-16/0.32
    c3d6 Jacobian             8.8e-17/0.26 1.3e-13/0.59 1.6e-10/0.63 4.3e-17/0.20
    c3d6 gradients            3.5e-16/0.67 2.7e-13/0.86 2.8e-10/0.66 3.4e-16/0.92
    c3d10 K single            7.1e-16/1.25 6.3e-13/0.42 8.1e-10/1.35 6.1e-16/0.75
    c3d10 K multi             9.1e-16/1.15 1.3e-12/0.57 1.7e-09/1.08 1.3e-15/0.89
    c3d10 mass                5.4e-16/0.67 7.7e-13/1.39 6.6e-10/0.95 5.1e-16/0.61
    c3d10 stress              1.0e-15/1.17 1.6e-12/0.70 1.2e-09/1.17 4.4e-16/0.30
    c3d10 von Mises           3.2e-16/0.75 1.8e-13/0.50 2.5e-10/1.70 3.9e-16/0.98
    c3d10 Jacobian            2.8e-16/0.80 9.2e-13/1.46 8.6e-10/1.21 2.8e-16/0.80
    c3d10 gradients           4.0e-16/0.78 1.0e-12/1.00 9.0e-10/0.78 4.2e-16/0.82

One fixed assertion found a kernel change, test_tet4_mass_reordered_identical: see its docstring (the K_mass row above is
from after it).
"""
import pytest
import torch

import exact_ref as X
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
E, NU, RHO, KAPPA = X.E, X.NU, X.RHO, X.KAPPA


def _mods():
    import fem355  # noqa: F401
    from fem355 import element, system
    return element, system


def _coef(kind):
    return {"elastic": E, "poisson": KAPPA, "mass": RHO}[kind]


def _tet4_ke(el, c, t, kind, gpu):
    if kind == "elastic":
        return el.compute_c3d4_K_matrix(c, t, E, NU, device=gpu, dtype=F64)
    if kind == "poisson":
        return el.compute_c3d4_poisson_K_matrix(c, t, KAPPA, device=gpu, dtype=F64)
    return el.compute_c3d4_M_matrix(c, t, RHO, device=gpu, dtype=F64)


# ----------------------------------------------------------------------------- c3d4 element quantities
@pytest.mark.parametrize("kind", ["elastic", "poisson", "mass"])
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_element_matrices(gpu, case, kind):
    el, _ = _mods()
    c, t = X.tet4_case(case)
    q = "K_" + kind
    K = _tet4_ke(el, c, t, kind, gpu)
    X.check(f"c3d4 {q} {case}", X.elem_err(K, X.tet4_exact(case, q)), X.tet4_calibration_err(case, q))


@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_volumes_and_B(gpu, case):
    el, _ = _mods()
    c, t = X.tet4_case(case)
    vol = el.compute_tetrahedral_volumes(c, t, device=gpu, dtype=F64)
    assert bool((vol > 0).all())
    X.check(f"c3d4 volumes {case}", X.elem_err(vol, X.tet4_exact(case, "vol")), X.tet4_calibration_err(case, "vol"))
    B = el.compute_c3d4_B_matrix(c, t, device=gpu, dtype=F64)
    X.check(f"c3d4 B {case}", X.elem_err(B, X.tet4_exact(case, "B")), X.tet4_calibration_err(case, "B"))


@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_stress(gpu, case):
    el, _ = _mods()
    c, t = X.tet4_case(case)
    sig, vm = el.compute_c3d4_element_stress(c, t, X.tet4_u(case), E, NU, device=gpu, dtype=F64)
    es, ev = X.tet4_exact(case, "stress")
    X.check(f"c3d4 stress {case}", X.elem_err(sig, es), X.tet4_calibration_err(case, "stress", "sigma"))
    X.check(f"c3d4 von Mises {case}", X.elem_err(vm, ev), X.tet4_calibration_err(case, "stress", "vm"))


# ----------------------------------------------------------------------------- c3d4 operators
@pytest.mark.parametrize("kind", ["elastic", "poisson"])
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_assembled_system(gpu, case, kind):
    """Fused assembly (assemble_tet4_system) and the assembly of the GPU's element matrices: product and Jacobi
    diagonal against exact, and against each other within the same bound."""
    el, system = _mods()
    c, t = X.tet4_case(case)
    cg, tg = c.to(gpu), t.to(gpu)
    y_ex, _, mag, dinv_ex = X.tet4_exact(case, "ebe_" + kind)
    cal_y = X.tet4_calibration_err(case, "ebe_" + kind, "y")
    cal_d = X.tet4_calibration_err(case, "ebe_" + kind, "diag")
    x = X.tet4_x(case, kind).reshape(-1).to(gpu)
    A = system.assemble_tet4_system(cg, tg, kind, _coef(kind), NU)
    A.check_singular()
    y = A.matvec(x).cpu()
    X.check(f"c3d4 fused {kind} matvec {case}", X.dof_err(y, y_ex, mag), cal_y)
    X.check(f"c3d4 fused {kind} jacobi {case}", X.dof_err(A.jacobi(), dinv_ex, dinv_ex.abs()), cal_d)
    Ke = _tet4_ke(el, c, t, kind, gpu)
    A2 = system.SellMatrix(A.g, A.bs).add_element_matrices(Ke, tg)
    y2 = A2.matvec(x).cpu()
    X.check(f"c3d4 K_e-assembled {kind} matvec {case}", X.dof_err(y2, y_ex, mag), cal_y)
    X.check(f"c3d4 K_e-assembled {kind} jacobi {case}", X.dof_err(A2.jacobi(), dinv_ex, dinv_ex.abs()), cal_d)
    X.check(f"c3d4 fused vs K_e-assembled {kind} {case}", X.dof_err(y, y2, mag), cal_y)


def _check_layout(A, t):
    """The invariants of test_gpu_matfree.test_layout_invariants."""
    eo, cp, sb, cn = (v.cpu().long() for v in A.layout())
    assert torch.equal(eo.sort().values, torch.arange(t.shape[0]))
    assert int((cp[1:] - cp[:-1]).max()) <= 512 and int((sb[1:] - sb[:-1]).max()) <= 256
    for ch in range(cp.numel() - 1):
        nodes = cn[sb[ch]:sb[ch + 1]]
        assert torch.all(nodes[1:] > nodes[:-1])
        assert torch.equal(nodes, torch.unique(t[eo[cp[ch]:cp[ch + 1]]].reshape(-1)))


@pytest.mark.parametrize("kind", ["elastic", "poisson"])
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_matfree(gpu, case, kind):
    _, system = _mods()
    c, t = X.tet4_case(case)
    y_ex, d_ex, mag, _ = X.tet4_exact(case, "ebe_" + kind)
    A = system.MatFreeOperator(c.to(gpu), t.to(gpu), kind, _coef(kind), NU)
    info = A.info()
    assert info["elements"] == t.shape[0] and info["nodes"] == c.shape[0]
    y = A.matvec(X.tet4_x(case, kind).reshape(-1).to(gpu))
    X.check(f"c3d4 matfree {kind} matvec {case}", X.dof_err(y, y_ex, mag),
            X.tet4_calibration_err(case, "ebe_" + kind, "y"))
    X.check(f"c3d4 matfree {kind} diag {case}", X.dof_err(A.diag(), d_ex, d_ex.abs()),
            X.tet4_calibration_err(case, "ebe_" + kind, "diag"))
    if case.startswith("squash"):
        _check_layout(A, t)


# ----------------------------------------------------------------------------- c3d4 fixed assertions
def test_tet4_mass_mirror_identical(gpu):
    """|det| does not depend on orientation: the mass of a mesh and of its mirrored copy are the same bits."""
    el, _ = _mods()
    c, t = X.tet4_case("flipped")
    M0 = el.compute_c3d4_M_matrix(c, t, RHO, device=gpu, dtype=F64)
    M1 = el.compute_c3d4_M_matrix(c * torch.tensor([1.0, 1.0, -1.0], dtype=F64), t, RHO, device=gpu, dtype=F64)
    assert torch.equal(M0, M1)
    assert bool((torch.diagonal(M0, dim1=1, dim2=2) > 0).all())
    p = torch.tensor([3, 4, 5, 0, 1, 2, 6, 7, 8, 9, 10, 11], device=M0.device)
    assert torch.equal(M0, M0[:, p][:, :, p])      # rho V (1 + delta_ab) / 20: one V per element, any node order


def test_tet4_mass_reordered_identical(gpu):
    """The mass of the half-flipped mesh is the unflipped mesh's, rows and columns permuted by [1, 0, 2, 3], bit for bit.

    This test found the one kernel change of the module: with det formed from the edges out of local node 0
    (tet4_grads, csrc/element.hpp) the order [1, 0, 2, 3] differences other edges and |det| rounded differently in the
    last bit -- 38 of the 81 reordered elements differed, by at most 3.78e-16 relative. The mass kernel now forms det
    from the nodes in ascending global id (tet4_det_sorted), so V does not depend on the local order."""
    el, _ = _mods()
    c, t = X.tet4_case("flipped")
    c0, t0 = X.tet4_case("unflipped")
    Mf = el.compute_c3d4_M_matrix(c, t, RHO, device=gpu, dtype=F64)
    M0 = el.compute_c3d4_M_matrix(c0, t0, RHO, device=gpu, dtype=F64)
    p = torch.tensor([3, 4, 5, 0, 1, 2, 6, 7, 8, 9, 10, 11], device=M0.device)
    assert torch.equal(Mf[0::2], M0[0::2])
    diff = (Mf[1::2] - M0[1::2][:, p][:, :, p]).abs().amax((1, 2)) / M0[1::2].abs().amax((1, 2))
    print(f"HARDGEOM c3d4 mass reordered: {int((diff > 0).sum())} of {diff.numel()} elements differ, "
          f"max rel {float(diff.max()):.2e}")
    assert torch.equal(Mf[1::2], M0[1::2][:, p][:, :, p])


def _tet4_paths(gpu):
    el, system = _mods()
    from fem355 import loads
    u = lambda c: 1e-9 * torch.randn(c.shape[0], 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    return {
        "K": lambda c, t: el.compute_c3d4_K_matrix(c, t, E, NU, device=gpu, dtype=F64),
        "poisson K": lambda c, t: el.compute_c3d4_poisson_K_matrix(c, t, KAPPA, device=gpu, dtype=F64),
        "B": lambda c, t: el.compute_c3d4_B_matrix(c, t, device=gpu, dtype=F64),
        "assembled elastic": lambda c, t: system.assemble_tet4_system(c.to(gpu), t.to(gpu), "elastic", E,
                                                                      NU).check_singular(),
        "assembled poisson": lambda c, t: system.assemble_tet4_system(c.to(gpu), t.to(gpu), "poisson",
                                                                      KAPPA).check_singular(),
        "matfree elastic": lambda c, t: system.MatFreeOperator(c.to(gpu), t.to(gpu), "elastic", E, NU),
        "matfree poisson": lambda c, t: system.MatFreeOperator(c.to(gpu), t.to(gpu), "poisson", KAPPA),
        "stress": lambda c, t: el.compute_c3d4_element_stress(c, t, u(c), E, NU, device=gpu, dtype=F64),
        "oracle K": lambda c, t: R.tet4_K(c, t, E, NU),
        "oracle gradients": lambda c, t: R.tet4_gradients(c, t),
        "svk tangent": lambda c, t: el.compute_c3d4_tangent_K_matrix(c, t, u(c), E, NU, "svk", device=gpu, dtype=F64),
        "neo-Hooke tangent": lambda c, t: el.compute_c3d4_tangent_K_matrix(c, t, u(c), E, NU, "neo_hookean",
                                                                           device=gpu, dtype=F64),
        "J2 update": lambda c, t: el.compute_c3d4_plastic_update(c, t, u(c), E, NU, 1e-3 * E, 0.1 * E, device=gpu,
                                                                 dtype=F64),
        "thermal load": lambda c, t: loads.compute_thermal_load(c, t, "c3d4", E, NU, 1.2e-5, 50.0, device=gpu,
                                                                dtype=F64),
        "thermal stress": lambda c, t: loads.compute_thermal_element_stress(c, t, "c3d4", u(c), E, NU, 1.2e-5, 50.0,
                                                                            device=gpu, dtype=F64),
    }


def _tet4_paths_other_rule(gpu):
    """c3d4 paths that document a rule of their own for a degenerate element (asserted as documented): the geometric
    stiffness flags only det = 0 or a non-finite det (csrc/buckling.hip), the body force needs |det| alone and
    raises for no element (loads.py)."""
    el, _ = _mods()
    from fem355 import loads
    u = lambda c: 1e-9 * torch.randn(c.shape[0], 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    return {
        "geometric stiffness": lambda c, t: el.compute_geometric_stiffness(c, t, "c3d4", u(c), E, NU, device=gpu,
                                                                           dtype=F64),
        "body force": lambda c, t: loads.compute_body_force(c, t, "c3d4", RHO, [0.0, 0.0, -9.81], device=gpu,
                                                            dtype=F64),
    }


def test_singular_threshold_accepts(gpu):
    """min|det| = 4e-12, above the absolute |det| < 1e-12 test: every path accepts the mesh."""
    c, t = X.threshold_case(False)
    for name, fn in _tet4_paths(gpu).items():
        fn(c, t)
    for name, fn in _tet4_paths_other_rule(gpu).items():
        assert bool(torch.isfinite(fn(c, t)).all()), name


def test_singular_threshold_refuses(gpu):
    """The same mesh with one tet of |det| = 2.5e-13 at element index 140: every path raises, except the two that
    document another rule."""
    c, t = X.threshold_case(True)
    for name, fn in _tet4_paths(gpu).items():
        with pytest.raises(ValueError, match="Singular"):
            fn(c, t)
            pytest.fail(f"{name} accepted a singular element")
    # the documented other rules: |det| = 2.5e-13 is neither zero nor non-finite, so both accept it with finite
    # output; with the inserted tet collapsed to one point (det = 0) the geometric stiffness raises, and the body
    # force, whose |det| / 6 is then zero, still does not
    other = _tet4_paths_other_rule(gpu)
    for name, fn in other.items():
        assert bool(torch.isfinite(fn(c, t)).all()), name
    c = c.clone()
    c[-4:] = c[-4]
    with pytest.raises(ValueError, match="Singular"):
        other["geometric stiffness"](c, t)
    assert bool(torch.isfinite(other["body force"](c, t)).all())


# ----------------------------------------------------------------------------- isoparametric families
@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_K(gpu, etype, case):
    el, _ = _mods()
    c, e, pos, s = X.iso_case(etype, case)
    Ks = el.compute_K_matrix(c, e, etype, E, NU, single=True, device=gpu, dtype=F64).cpu()
    Km = el.compute_K_matrix(c, e, etype, E, NU, single=False, device=gpu, dtype=F64).cpu()
    ex_s, ex_m = X.iso_exact(etype, case, "K")
    X.check(f"{etype} K single {case}", X.elem_err(Ks[s], ex_s), X.iso_calibration_err(etype, case, "K", 0))
    X.check(f"{etype} K multi {case}", X.elem_err(X.stack_first(Km, etype)[s], X.stack_first(ex_m, etype)),
            X.iso_calibration_err(etype, case, "K", 1))
    # sign convention on every element: the stiffness carries the signed detJ (x is no rigid-body motion)
    x = torch.randn(Ks.shape[-1], dtype=F64, generator=torch.Generator().manual_seed(31))
    want = torch.where(pos, 1.0, -1.0).to(F64)
    form = lambda K: torch.sign(torch.einsum("i,...ij,j->...", x, K, x))
    if etype == "c3d6":     # single=True: B^T D B times the absolute wedge volume; single=False: the signed sum
        assert bool((form(Ks) > 0).all())
        assert torch.equal(form(Km), want)
    else:
        assert torch.equal(form(Ks), want)
        assert torch.equal(form(Km), want.expand(Km.shape[0], -1))


@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_mass(gpu, etype, case):
    el, _ = _mods()
    c, e, pos, s = X.iso_case(etype, case)
    Me = el.compute_M_matrix(c, e, etype, RHO, device=gpu, dtype=F64)
    assert bool((torch.diagonal(Me, dim1=1, dim2=2) > 0).all())      # |detJ| for either orientation
    X.check(f"{etype} mass {case}", X.elem_err(Me.cpu()[s], X.iso_exact(etype, case, "mass")),
            X.iso_calibration_err(etype, case, "mass"))
    mirrored = el.compute_M_matrix(c * torch.tensor([1.0, 1.0, -1.0], dtype=F64), e, etype, RHO, device=gpu, dtype=F64)
    assert torch.equal(Me, mirrored)


@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_stress(gpu, etype, case):
    el, _ = _mods()
    c, e, _, s = X.iso_case(etype, case)
    sig, vm = el.compute_element_stress(c, e, X.iso_u(etype, case), E, NU, etype, single=True, device=gpu, dtype=F64)
    es, ev = X.iso_exact(etype, case, "stress")
    X.check(f"{etype} stress {case}", X.elem_err(sig.cpu()[s], es), X.iso_calibration_err(etype, case, "stress", 0))
    X.check(f"{etype} von Mises {case}", X.elem_err(vm.cpu()[s], ev), X.iso_calibration_err(etype, case, "stress", 1))


@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_jacobian_and_gradients(gpu, etype, case):
    el, _ = _mods()
    c, e, pos, s = X.iso_case(etype, case)
    pt = X.iso_geom_point(etype)
    J = getattr(el, f"compute_{etype}_Jacobian")(c, e, pt, device=gpu, dtype=F64).cpu()
    G = getattr(el, f"compute_{etype}_shape_gradients")(c, e, pt, device=gpu, dtype=F64).cpu()
    assert torch.equal(torch.det(J) > 0, pos)
    eJ, eG = X.iso_exact(etype, case, "geom")
    X.check(f"{etype} Jacobian {case}", X.elem_err(J[s], eJ), X.iso_calibration_err(etype, case, "geom", 0))
    X.check(f"{etype} gradients {case}", X.elem_err(G[s], eG), X.iso_calibration_err(etype, case, "geom", 1))
