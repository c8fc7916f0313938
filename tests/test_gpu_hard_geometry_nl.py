"""GPU tier of the second generation of element kernels on hard geometry: the hyperelastic tangent / force / energy /
stress (csrc/nonlinear.hip), the J2 return (csrc/plasticity.hip), the geometric stiffness (csrc/buckling.hip) and the
distributed loads (csrc/loads.hip) on the inverted, shifted, tiny, huge and sliver meshes of tests/exact_ref.py,
judged by exact rational arithmetic (tests/exact_ref2.py). Their own tests compare with fp64 restatements that take
their gradients from the oracle's inv([1 x y z]) form on well-shaped meshes of order 1; a restatement that shares a
kernel's formulation shares its cancellation.

Meshes and comparison are those of tests/test_gpu_hard_geometry.py: exact_ref.check asserts error <= 8 x max(calibration
error, 2.2e-16), element quantities by the per-element relative error, assembled nodal vectors per dof against the
exact magnitude sum. Calibration: for c3d4 the restatements' formulas on the fp64 edge-difference gradients and
|det| / 6; for the isoparametric families the restatements as they are (absolute-coordinate Jacobian, like the
kernels). The displacement of a case is a unit-mesh field pushed through the case's linear map, so that no input
depends on the absolute coordinates; the two tangents are compared on 16 elements (8 of each orientation, element 161
of the ragged last block among them), everything else of c3d4 on the whole mesh, the isoparametric per-element
quantities on the 8-element samples. The kernels always run the whole mesh.

Fixed assertions: the plastic flags are the exact ones on every element; Kt and Gs are symmetric bit for bit; the
body force of the half-flipped mesh and the energy of each reordered element equal the unflipped mesh's within the
measured bound; a uniform pressure on the closed boundary sums to zero within the bound on every case, the rotated
sliver included (a normal that flips on a squashed face would leave twice that face's force).

Measured on the MI355X, as "error / ratio": the kernel's error against exact, and its ratio to max(calibration
error, 2.2e-16) (the tests assert ratio <= 8; the largest is 2.95, the neo-Hooke nodal force on the rotated sliver; the
calibration side is CPU arithmetic and moves in the last digit between hosts). The c3d4 kernels stay at 1e-15 at any
shift and scale and share the rotated sliver's 1e-12 with the edge form; there the finite-strain field has F ~ 1e3
with det F ~ 1, and everything that holds det F (det F, both Cauchy stresses, the neo-Hooke tangent) sits at the
7e-10 that the rounding of F itself leaves. The isoparametric kernels lose accuracy under a shift exactly as the
restatements do (1e-13 relative at 1e3, 1e-10 at 1e6: the absolute-coordinate Jacobian, recorded, not fixed). "closed
pressure" is |sum_n F_n| / sum_n mag_n of the uniform pressure, against the bound of "surface_p_uniform".

  c3d4                             flipped     shift1e4     shift1e6    scale1e-3     scale1e3   squash1e-4   squash_rot
    svk tangent               4.3e-16/0.81 6.5e-16/1.56 3.5e-16/0.95 5.0e-16/1.00 5.8e-16/1.08 8.5e-16/1.16 3.7e-12/0.80
    svk force                 1.8e-15/1.67 1.2e-15/1.84 1.0e-15/1.25 1.0e-15/1.33 6.7e-16/1.11 1.8e-15/2.35 2.0e-12/0.46
    svk energy                1.4e-15/1.35 9.7e-16/1.06 1.2e-15/1.37 8.1e-16/1.00 1.4e-15/1.09 1.8e-15/1.26 3.7e-12/0.77
    svk Cauchy                1.0e-15/1.27 9.2e-16/0.91 8.7e-16/1.05 7.4e-16/0.90 8.9e-16/1.12 1.5e-15/0.85 7.5e-10/0.90
    det F                     3.7e-16/0.95 3.8e-16/0.99 3.7e-16/0.95 2.1e-16/0.43 4.0e-16/1.10 3.8e-16/0.53 7.5e-10/0.90
    neo_hookean tangent       7.6e-16/1.76 7.0e-16/0.95 5.6e-16/0.91 6.0e-16/1.00 6.7e-16/1.16 4.0e-16/0.52 7.5e-10/0.83
    neo_hookean force         2.8e-15/1.14 2.5e-15/0.64 3.3e-15/1.00 4.2e-15/2.80 2.8e-15/1.19 1.2e-15/0.41 5.8e-12/2.95
    neo_hookean energy        4.4e-15/0.99 6.5e-15/1.00 3.1e-15/0.47 4.4e-15/0.83 3.9e-15/0.76 1.2e-15/1.20 1.2e-12/0.77
    neo_hookean Cauchy        1.0e-15/0.46 1.4e-15/0.73 1.1e-15/0.60 9.5e-16/0.49 1.9e-15/0.93 9.9e-16/1.06 7.5e-10/0.90
    J2 virgin Kt              3.9e-16/0.85 5.9e-16/1.46 3.8e-16/0.95 6.0e-16/1.05 4.0e-16/0.88 4.9e-16/0.87 1.2e-12/0.80
    J2 virgin fe              1.5e-15/1.12 1.7e-15/1.19 1.8e-15/1.24 1.8e-15/0.91 1.5e-15/0.99 9.8e-16/1.00 1.2e-12/0.77
    J2 virgin we              7.2e-16/1.07 1.0e-15/1.17 8.0e-16/1.06 7.4e-16/0.94 6.7e-16/0.81 1.2e-15/0.76 1.2e-12/0.77
    J2 virgin sigma           1.4e-15/1.07 1.5e-15/1.00 1.7e-15/1.45 1.4e-15/0.79 1.1e-15/0.83 9.6e-16/1.00 1.2e-12/0.77
    J2 virgin ep              1.8e-15/0.86 2.2e-15/1.21 1.9e-15/1.08 2.3e-15/1.49 1.8e-15/0.83 3.6e-15/0.83 2.7e-12/0.75
    J2 virgin alpha           1.6e-15/0.80 2.1e-15/1.20 1.8e-15/1.07 2.1e-15/1.29 1.9e-15/0.99 3.8e-15/0.85 2.7e-12/0.75
    J2 hardened Kt            3.6e-16/0.97 3.7e-16/1.02 3.5e-16/0.76 3.6e-16/0.79 4.1e-16/0.86 6.0e-16/1.33 1.2e-12/0.80
    J2 hardened fe            8.9e-16/0.82 9.1e-16/1.20 1.3e-15/0.99 1.4e-15/0.96 1.1e-15/0.84 2.5e-15/1.10 1.2e-12/0.29
    J2 hardened we            7.3e-16/1.05 8.5e-16/1.31 6.8e-16/0.87 7.6e-16/1.08 6.5e-16/0.90 4.3e-15/0.96 1.2e-12/0.77
    J2 hardened sigma         6.8e-16/0.66 8.4e-16/0.82 1.0e-15/0.70 1.2e-15/0.96 1.0e-15/0.70 2.5e-15/1.09 1.6e-12/0.23
    J2 hardened ep            1.4e-15/1.03 1.5e-15/1.00 1.4e-15/0.95 1.1e-15/0.83 1.4e-15/1.00 2.7e-15/0.95 1.9e-12/0.58
    J2 hardened alpha         7.7e-16/0.94 1.0e-15/1.00 8.5e-16/0.83 7.2e-16/1.08 7.9e-16/1.00 2.4e-15/0.79 1.9e-12/0.58
    Gs u                      1.2e-15/1.39 1.0e-15/1.17 1.2e-15/0.95 1.9e-15/1.73 1.3e-15/1.19 1.2e-15/1.03 2.5e-12/0.77
    Gs sigma0                 6.9e-16/1.00 7.8e-16/1.04 5.6e-16/0.98 8.8e-16/1.73 8.3e-16/1.14 5.2e-16/0.71 1.2e-12/0.77
    Gs both                   1.0e-15/1.02 1.1e-15/1.50 1.3e-15/1.89 1.5e-15/1.22 9.3e-16/0.96 1.4e-15/1.24 2.5e-12/0.77
    body_gravity              4.2e-16/1.00 3.1e-16/0.78 4.1e-16/1.34 3.9e-16/0.90 3.3e-16/0.74 3.7e-16/1.11 5.8e-13/0.81
    body_accel                3.5e-16/0.92 3.5e-16/0.98 2.9e-16/0.74 3.7e-16/1.00 2.7e-16/0.95 3.3e-16/1.00 6.0e-13/0.50
    thermal_T_uniform         2.8e-16/1.00 2.8e-16/1.00 1.4e-16/0.50 2.7e-16/1.00 3.0e-16/0.69 4.2e-16/1.56 4.1e-16/1.15
    tstress T_uniform         8.0e-16/0.75 9.0e-16/0.76 6.6e-16/0.85 8.2e-16/0.90 9.0e-16/0.70 7.7e-16/1.32 1.2e-12/0.77
    tstress vm T_uniform      7.9e-16/0.94 7.6e-16/0.87 6.3e-16/1.00 7.1e-16/0.70 7.9e-16/1.06 6.1e-16/0.95 1.2e-12/0.77
    thermal_T_nodal           4.2e-16/1.37 4.7e-16/1.33 2.6e-16/0.91 4.3e-16/1.06 3.1e-16/0.70 3.9e-16/1.10 4.4e-16/1.36
    tstress T_nodal           9.2e-16/1.01 9.6e-16/0.95 8.5e-16/1.00 8.2e-16/0.76 9.2e-16/0.86 9.2e-16/1.59 1.2e-12/0.77
    tstress vm T_nodal        7.7e-16/1.20 6.5e-16/1.03 7.1e-16/1.09 5.8e-16/0.99 5.6e-16/1.11 6.4e-16/0.97 1.2e-12/0.77
    thermal_T_element         3.7e-16/1.04 8.4e-16/1.00 6.7e-16/1.33 3.8e-16/1.04 1.2e-15/0.88 4.1e-16/0.67 1.1e-15/0.90
    tstress T_element         8.0e-16/0.78 9.3e-16/1.00 8.2e-16/0.91 7.1e-16/0.70 8.0e-16/0.71 9.2e-16/1.44 1.2e-12/0.77
    tstress vm T_element      6.5e-16/1.09 7.9e-16/1.41 5.7e-16/0.92 5.9e-16/0.59 5.6e-16/0.92 6.4e-16/0.75 1.2e-12/0.77
    surface_p_uniform         1.3e-16/0.60 1.3e-16/0.60 1.3e-16/0.60 1.3e-16/0.57 1.4e-16/0.62 2.0e-16/0.89 1.7e-13/1.00
    closed pressure           8.5e-18/0.04 1.5e-17/0.07 3.6e-18/0.02 2.9e-18/0.01 4.5e-18/0.02 7.5e-21/0.00 1.5e-16/0.00
    surface_p_face            2.0e-16/0.93 1.8e-16/0.80 2.1e-16/0.95 1.8e-16/0.84 1.8e-16/0.84 2.2e-16/0.99 2.2e-13/1.00
    surface_t_uniform         2.7e-16/1.00 2.1e-16/0.93 2.1e-16/0.93 1.9e-16/0.89 2.9e-16/1.00 4.1e-16/1.00 1.6e-13/1.00
    surface_t_face            1.5e-16/0.68 1.9e-16/0.88 1.2e-16/0.54 1.5e-16/0.66 1.6e-16/0.73 1.8e-16/0.82 1.1e-13/1.00

  isoparametric                      plain     shift1e3     shift1e6   squash1e-4
    c3d8 Gs u                 3.5e-16/0.50 4.4e-13/1.00 9.5e-10/1.00 6.3e-16/0.82
    c3d8 Gs sigma0            4.0e-16/0.60 4.3e-13/1.00 4.7e-10/1.00 6.6e-16/0.87
    c3d8 Gs both              5.4e-16/0.84 3.3e-13/1.00 5.6e-10/1.00 7.7e-16/1.00
    c3d6 Gs u                 5.1e-16/0.63 5.2e-13/0.98 3.4e-10/0.98 7.7e-16/0.89
    c3d6 Gs sigma0            4.1e-16/0.96 5.7e-13/0.90 3.3e-10/1.09 5.4e-16/0.81
    c3d6 Gs both              5.0e-16/1.02 5.2e-13/1.16 3.0e-10/1.00 8.8e-16/1.02
    c3d10 Gs u                7.6e-16/0.96 1.9e-12/1.00 1.4e-09/1.02 6.3e-16/0.94
    c3d10 Gs sigma0           7.4e-16/1.10 8.7e-13/1.00 5.5e-10/0.98 5.1e-16/1.05
    c3d10 Gs both             1.0e-15/0.94 1.9e-12/1.00 1.4e-09/1.02 6.2e-16/0.87
    c3d8 body_gravity         4.3e-16/1.03 3.2e-13/1.22 1.7e-10/0.58 5.4e-16/1.00
    c3d8 body_accel           3.9e-16/0.63 2.6e-13/0.95 2.1e-10/0.61 5.9e-16/1.00
    c3d8 thermal_T_uniform    2.8e-16/0.82 2.7e-13/0.81 3.8e-10/0.69 3.5e-16/0.69
    c3d8 tstress T_uniform    3.0e-16/0.82 3.9e-13/1.18 4.2e-10/0.98 3.0e-16/0.21
    c3d8 tstress vm T_uniform 3.6e-16/1.00 8.7e-14/0.85 8.9e-11/0.88 3.4e-16/0.75
    c3d8 thermal_T_nodal      4.0e-16/0.94 2.9e-13/0.93 3.8e-10/0.83 5.3e-16/1.41
    c3d8 tstress T_nodal      4.7e-16/2.09 2.1e-13/1.19 4.2e-10/0.74 3.2e-16/0.25
    c3d8 tstress vm T_nodal   4.6e-16/1.18 8.7e-14/0.85 8.9e-11/0.88 3.4e-16/0.75
    c3d8 thermal_T_element    3.7e-16/1.29 2.8e-13/0.81 4.0e-10/0.73 6.5e-16/1.29
    c3d8 tstress T_element    3.8e-16/1.00 3.4e-13/1.72 4.8e-10/0.74 3.7e-16/0.33
    c3d8 tstress vm T_element 4.6e-16/1.28 8.7e-14/0.85 8.9e-11/0.88 4.5e-16/0.80
    c3d8 surface_p_uniform    2.6e-16/1.00 1.3e-13/0.59 1.9e-10/1.33 3.2e-16/1.00
    c3d8 closed pressure      1.9e-17/0.07 2.4e-14/0.11 3.9e-11/0.28 5.8e-17/0.18
    c3d8 surface_p_face       2.0e-16/0.58 1.4e-13/0.70 1.9e-10/1.51 3.0e-16/0.94
    c3d8 surface_t_uniform    2.7e-16/1.00 1.3e-13/0.28 1.2e-10/1.06 3.3e-16/1.00
    c3d8 surface_t_face       2.5e-16/0.98 1.1e-13/0.45 1.0e-10/1.39 3.0e-16/1.00
    c3d6 body_gravity         4.3e-16/0.68 1.8e-13/0.32 1.8e-10/0.53 4.0e-16/0.71
    c3d6 body_accel           4.0e-16/0.75 1.6e-13/0.29 2.0e-10/0.75 4.8e-16/1.06
    c3d6 thermal_T_uniform    6.3e-16/1.00 3.4e-13/0.34 5.8e-10/0.96 5.6e-16/0.67
    c3d6 tstress T_uniform    2.1e-16/0.50 1.1e-13/0.53 8.7e-11/1.04 5.1e-16/0.24
    c3d6 tstress vm T_uniform 2.8e-16/0.67 1.1e-13/1.45 6.9e-11/1.28 2.4e-16/0.35
    c3d6 thermal_T_nodal      6.2e-16/1.32 3.4e-13/0.34 5.9e-10/0.97 5.3e-16/0.67
    c3d6 tstress T_nodal      3.6e-16/0.66 1.8e-13/0.43 1.7e-10/1.05 5.1e-16/0.29
    c3d6 tstress vm T_nodal   4.0e-16/0.95 1.1e-13/1.44 6.9e-11/1.28 2.6e-16/0.38
    c3d6 thermal_T_element    7.7e-16/1.07 3.1e-13/0.31 5.7e-10/0.94 6.2e-16/0.70
    c3d6 tstress T_element    3.4e-16/0.39 1.7e-13/0.26 2.7e-10/1.05 5.3e-16/0.33
    c3d6 tstress vm T_element 4.4e-16/1.00 1.1e-13/1.44 6.9e-11/1.28 2.6e-16/0.38
    c3d6 surface_p_uniform    2.6e-16/1.00 9.0e-14/0.57 1.7e-10/0.67 3.2e-16/1.00
    c3d6 closed pressure      3.6e-18/0.01 1.8e-14/0.11 3.5e-11/0.13 6.7e-21/0.00
    c3d6 surface_p_face       1.8e-16/0.36 9.8e-14/0.56 1.7e-10/0.63 2.0e-16/0.68
    c3d6 surface_t_uniform    3.3e-16/1.00 9.8e-14/0.32 7.6e-11/1.27 3.3e-16/1.00
    c3d6 surface_t_face       3.2e-16/1.44 1.3e-13/0.63 1.0e-10/1.77 2.0e-16/0.91
    c3d10 body_gravity        4.7e-16/0.97 9.0e-13/0.99 5.2e-10/0.95 5.7e-16/0.69
    c3d10 body_accel          6.9e-16/1.13 1.0e-12/0.95 7.6e-10/1.19 6.9e-16/0.84

One measured comparison found a kernel change, test_tet4_hyperelastic on squash1e-4_rot: see its docstring (the rows
above are from after it).
"""
import pytest
import torch

import exact_ref as X
import exact_ref2 as X2

pytestmark = pytest.mark.gpu
F64 = torch.float64
E, NU, RHO = X2.E, X2.NU, X2.RHO
SY, HARD, ALPHA_T, T_REF = X2.SIGMA_Y, X2.HARD, X2.ALPHA_T, X2.T_REF
SAMPLE = torch.tensor(X2.TANGENT_SAMPLE)


def _mods():
    import fem355  # noqa: F401
    from fem355 import element, loads
    return element, loads


def _bit_symmetric(K):
    return torch.equal(K, K.transpose(1, 2))


# ----------------------------------------------------------------------------- c3d4 hyperelastic
@pytest.mark.parametrize("material", X2.MATERIALS)
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_hyperelastic(gpu, case, material):
    """Tangent (16-element sample), nodal internal force, energy, Cauchy stress and det F against exact.

    This test found the one kernel change of the module. On squash1e-4_rot the deformation gradient has entries of
    1e3 and a determinant of 1.2; k_tet4_nl formed det F and the cofactors of F by the plain expansion, whose products
    cancel by 1e8: det F and the svk Cauchy stress were off by 3.2e-08 and the neo-Hooke tangent by 1.8e-08, ratios 38
    and 20 to a calibration form (torch.det / torch.linalg.inv, pivoted) at 8e-10, which is what the rounding of F
    leaves. The kernel now forms each 2 x 2 cofactor as a Kahan difference of products and det F as a compensated
    3-term dot (dop, dot3c, csrc/element.hpp), and compute_c3d4_deformation_gradient returns the kernel's
    det F where it had its own plain expansion in torch."""
    el, _ = _mods()
    c, t = X.tet4_case(case)
    u, q = X2.hyper_u(case), "hyper_" + material
    ex = X2.tet4_exact2(case, q)
    cal = lambda part: X2.tet4_calibration_err2(case, q, part)
    kw = dict(material=material, device=gpu, dtype=F64)
    Kt = el.compute_c3d4_tangent_K_matrix(c, t, u, E, NU, **kw)
    assert _bit_symmetric(Kt)
    X.check(f"c3d4 {material} tangent {case}", X.elem_err(Kt[SAMPLE.to(Kt.device)], ex["Kt"]), cal("Kt"))
    fint = el.compute_c3d4_internal_forces(c, t, u, E, NU, **kw)
    X.check(f"c3d4 {material} force {case}", X.dof_err(fint, ex["fint"], ex["fint_mag"]), cal("fint"))
    we = el.compute_c3d4_strain_energy(c, t, u, E, NU, **kw)
    X.check(f"c3d4 {material} energy {case}", X.elem_err(we, ex["we"]), cal("we"))
    sig = el.compute_c3d4_cauchy_stress(c, t, u, E, NU, **kw)
    X.check(f"c3d4 {material} Cauchy {case}", X.elem_err(sig, ex["sigma"]), cal("sigma"))
    if material == "svk":     # the deformation gradient does not depend on the material
        _, detF = el.compute_c3d4_deformation_gradient(c, t, u, device=gpu, dtype=F64)
        X.check(f"c3d4 det F {case}", X.elem_err(detF, ex["detF"]), cal("detF"))


@pytest.mark.parametrize("material", X2.MATERIALS)
def test_tet4_energy_reordered_elements(gpu, material):
    """The strain energy of each element of the half-flipped mesh whose local order is [1, 0, 2, 3] equals its twin's on
    the unflipped mesh within the measured bound of the energy, and V W > 0 on both (V = |det| / 6)."""
    el, _ = _mods()
    c, t = X.tet4_case("flipped")
    c0, t0 = X.tet4_case("unflipped")
    u = X2.hyper_u("flipped")
    wf = el.compute_c3d4_strain_energy(c, t, u, E, NU, material=material, device=gpu, dtype=F64).cpu()
    w0 = el.compute_c3d4_strain_energy(c0, t0, u, E, NU, material=material, device=gpu, dtype=F64).cpu()
    assert bool((wf > 0).all()) and bool((w0 > 0).all())
    assert torch.equal(wf[0::2], w0[0::2])
    X.check(f"c3d4 {material} energy reordered vs unflipped", X.elem_err(wf[1::2], w0[1::2]),
            X2.tet4_calibration_err2("flipped", "hyper_" + material, "we"))


# ----------------------------------------------------------------------------- c3d4 J2
@pytest.mark.parametrize("which", ["virgin", "hardened"])
@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_j2(gpu, case, which):
    el, _ = _mods()
    c, t = X.tet4_case(case)
    q = "j2_" + which
    ex = X2.tet4_exact2(case, q)
    cal = lambda part: X2.tet4_calibration_err2(case, q, part)
    st = X2.j2_state(case, which)
    state = None if st is None else el.PlasticState(st[0], st[1])
    up = el.compute_c3d4_plastic_update(c, t, X2.j2_u(case, which), E, NU, SY, HARD, state=state, device=gpu, dtype=F64)
    assert torch.equal(up.plastic.cpu(), ex["plastic"])
    assert _bit_symmetric(up.K)
    name = f"c3d4 J2 {which}"
    X.check(f"{name} Kt {case}", X.elem_err(up.K[SAMPLE.to(up.K.device)], ex["Kt"]), cal("Kt"))
    X.check(f"{name} fe {case}", X.elem_err(up.forces, ex["fe"]), cal("fe"))
    X.check(f"{name} we {case}", X.elem_err(up.energy, ex["we"]), cal("we"))
    X.check(f"{name} sigma {case}", X.elem_err(up.stress, ex["sigma"]), cal("sigma"))
    X.check(f"{name} ep {case}", X.elem_err(up.state.plastic_strain, ex["ep"]), cal("ep"))
    X.check(f"{name} alpha {case}", X.elem_err(up.state.equivalent_plastic_strain, ex["alpha"]), cal("alpha"))


# ----------------------------------------------------------------------------- geometric stiffness
def _geo(el, c, e, etype, mode, u, s0, gpu):
    ua, sa = X2._geo_args(mode, u, s0)
    return el.compute_geometric_stiffness(c, e, etype, displacement=ua, E=None if ua is None else E,
                                          nu=None if ua is None else NU, prestress=sa, device=gpu, dtype=F64)


@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_geometric_stiffness(gpu, case):
    el, _ = _mods()
    c, t = X.tet4_case(case)
    for mode in X2.GEO_MODES:
        Gs = _geo(el, c, t, "c3d4", mode, X.tet4_u(case), X2.sigma0(t.shape[0]), gpu)
        assert _bit_symmetric(Gs)
        X.check(f"c3d4 Gs {mode} {case}", X.elem_err(Gs, X2.tet4_exact2(case, "geo_" + mode)),
                X2.tet4_calibration_err2(case, "geo_" + mode))


@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_geometric_stiffness(gpu, etype, case):
    el, _ = _mods()
    c, e, _, s = X.iso_case(etype, case)
    for mode in X2.GEO_MODES:
        Gs = _geo(el, c, e, etype, mode, X.iso_u(etype, case), X2.sigma0(e.shape[0]), gpu).cpu()
        assert _bit_symmetric(Gs)
        X.check(f"{etype} Gs {mode} {case}", X.elem_err(Gs[s], X2.iso_exact2(etype, case, "geo_" + mode)),
                X2.iso_calibration_err2(etype, case, "geo_" + mode))


# ----------------------------------------------------------------------------- loads
def _body(ld, c, e, etype, mode, gpu):
    return ld.compute_body_force(c, e, etype, RHO, X2.load_inputs(c.shape[0], e.shape[0])[mode], device=gpu, dtype=F64)


def _thermal(ld, c, e, etype, mode, gpu):
    T = X2.load_inputs(c.shape[0], e.shape[0])[mode]
    return ld.compute_thermal_load(c, e, etype, E, NU, ALPHA_T, T, T_REF, device=gpu, dtype=F64)


def _tstress(ld, c, e, etype, u, mode, gpu):
    T = X2.load_inputs(c.shape[0], e.shape[0])[mode]
    return ld.compute_thermal_element_stress(c, e, etype, X2.thermal_u(u), E, NU, ALPHA_T, T, T_REF, device=gpu,
                                             dtype=F64)


def _surface(ld, c, e, etype, mode, gpu):
    out = 0
    for faces, extra in X2.boundary(e, etype):
        out = out + ld.compute_surface_load(c, faces, extra, device=gpu, dtype=F64,
                                            **X2._surf_kw(mode, X2.face_inputs(faces.shape[0]))).cpu()
    return out


def _closed_pressure_sum(name, F, exact, calibration_err):
    """A uniform pressure on a closed boundary has no resultant. Every dof is within tol x mag_dof of its exact value
    (the comparison above, tol from the load's calibration error), and the exact values sum to zero, so
    |sum_n F_n| <= tol x sum_n mag_n per component: the same bound on the same calibration error."""
    _, mag = exact
    X.check(name, float((F.detach().to("cpu", F64).sum(0).abs() / mag.sum(0)).max()), calibration_err)


@pytest.mark.parametrize("case", X.TET4_CASES)
def test_tet4_loads(gpu, case):
    _, ld = _mods()
    c, t = X.tet4_case(case)
    ex = lambda q: X2.tet4_exact2(case, q)
    cal = lambda q, part=None: X2.tet4_calibration_err2(case, q, part)
    for mode in X2.BODY_MODES:
        q = "body_" + mode
        X.check(f"c3d4 {q} {case}", X.dof_err(_body(ld, c, t, "c3d4", mode, gpu), *ex(q)), cal(q))
    for mode in X2.T_MODES:
        q = "thermal_" + mode
        X.check(f"c3d4 {q} {case}", X.dof_err(_thermal(ld, c, t, "c3d4", mode, gpu), *ex(q)), cal(q))
        sig, vm = _tstress(ld, c, t, "c3d4", X.tet4_u(case), mode, gpu)
        es, ev = ex("tstress_" + mode)
        X.check(f"c3d4 tstress {mode} {case}", X.elem_err(sig, es), cal("tstress_" + mode, 0))
        X.check(f"c3d4 tstress vm {mode} {case}", X.elem_err(vm, ev), cal("tstress_" + mode, 1))
    for mode in X2.SURF_MODES:
        q = "surface_" + mode
        F = _surface(ld, c, t, "c3d4", mode, gpu)
        X.check(f"c3d4 {q} {case}", X.dof_err(F, *ex(q)), cal(q))
        if mode == "p_uniform":
            _closed_pressure_sum(f"c3d4 closed pressure {case}", F, ex(q), cal(q))


def test_tet4_body_force_flipped_equals_unflipped(gpu):
    """V = |det| / 6 for either orientation: the body force of the half-flipped mesh is the unflipped mesh's within the
    measured bound of the body force."""
    _, ld = _mods()
    c, t = X.tet4_case("flipped")
    c0, t0 = X.tet4_case("unflipped")
    for mode in X2.BODY_MODES:
        Ff, F0 = _body(ld, c, t, "c3d4", mode, gpu), _body(ld, c0, t0, "c3d4", mode, gpu)
        _, mag = X2.tet4_exact2("flipped", "body_" + mode)
        X.check(f"c3d4 body_{mode} flipped vs unflipped", X.dof_err(Ff, F0.cpu(), mag),
                X2.tet4_calibration_err2("flipped", "body_" + mode))


@pytest.mark.parametrize("case", X.ISO_CASES)
@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_loads(gpu, etype, case):
    _, ld = _mods()
    c, e, _, s = X.iso_case(etype, case)
    ex = lambda q: X2.iso_exact2(etype, case, q)
    cal = lambda q, part=None: X2.iso_calibration_err2(etype, case, q, part)
    for mode in X2.BODY_MODES:
        q = "body_" + mode
        X.check(f"{etype} {q} {case}", X.dof_err(_body(ld, c, e, etype, mode, gpu), *ex(q)), cal(q))
    if etype not in X2.ISO_THERMAL:
        return
    for mode in X2.T_MODES:
        q = "thermal_" + mode
        X.check(f"{etype} {q} {case}", X.dof_err(_thermal(ld, c, e, etype, mode, gpu), *ex(q)), cal(q))
        sig, vm = _tstress(ld, c, e, etype, X.iso_u(etype, case), mode, gpu)
        es, ev = ex("tstress_" + mode)
        X.check(f"{etype} tstress {mode} {case}", X.elem_err(sig.cpu()[s], es), cal("tstress_" + mode, 0))
        X.check(f"{etype} tstress vm {mode} {case}", X.elem_err(vm.cpu()[s], ev), cal("tstress_" + mode, 1))
    for mode in X2.SURF_MODES:
        q = "surface_" + mode
        F = _surface(ld, c, e, etype, mode, gpu)
        X.check(f"{etype} {q} {case}", X.dof_err(F, *ex(q)), cal(q))
        if mode == "p_uniform":
            _closed_pressure_sum(f"{etype} closed pressure {case}", F, ex(q), cal(q))
