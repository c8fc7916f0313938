"""CPU tier of the exact-rational element references (tests/exact_ref.py): the helper agrees with the oracle where
the oracle is accurate, the oracle's loss of accuracy away from the origin is real (which is why the hard-geometry
GPU tests do not use it on shifted c3d4 meshes), and the comparison those tests use fails wrong restatements."""
import pytest
import torch

import exact_ref as X
from oracle import ref_cpu as R

F64 = torch.float64
AGREE = 2e-15


def test_tet4_exact_matches_oracle_on_plain_mesh():
    """Unshifted, unflipped kuhn_cube(3, jitter 0.15): every c3d4 quantity within 2e-15 of the oracle."""
    case = "unflipped"
    c, t = X.tet4_case(case)
    assert bool((R.tet4_cofactors(c, t)[1] > 0).all())
    assert X.elem_err(R.tet_volumes(c, t), X.tet4_exact(case, "vol")) < AGREE
    assert X.elem_err(R.tet4_gradients(c, t), X.tet4_gradients(c, t)) < AGREE
    assert X.elem_err(R.tet4_B(c, t), X.tet4_exact(case, "B")) < AGREE
    assert X.elem_err(R.tet4_K(c, t, X.E, X.NU), X.tet4_exact(case, "K_elastic")) < AGREE
    assert X.elem_err(R.tet4_poisson_K(c, t, X.KAPPA), X.tet4_exact(case, "K_poisson")) < AGREE
    m = (torch.ones(4, 4, dtype=F64) + torch.eye(4, dtype=F64)) / 20.0       # rho V (1 + delta_ab) / 20 (x) I3
    Me = torch.kron(X.RHO * R.tet_volumes(c, t).view(-1, 1, 1) * m, torch.eye(3, dtype=F64))
    assert X.elem_err(Me, X.tet4_exact(case, "K_mass")) < AGREE
    s, v = R.tet4_stress(c, t, X.tet4_u(case), X.E, X.NU)
    es, ev = X.tet4_exact(case, "stress")
    assert X.elem_err(s, es) < AGREE and X.elem_err(v, ev) < AGREE
    for kind, K in (("elastic", R.tet4_K(c, t, X.E, X.NU)), ("poisson", R.tet4_poisson_K(c, t, X.KAPPA))):
        y, d, mag, dinv = X.tet4_exact(case, "ebe_" + kind)
        x = X.tet4_x(case, kind)
        assert X.dof_err(R.nodal_forces(K, t, x), y, mag) < AGREE
        assert X.dof_err(R.diag_preconditioner(K, t, c.shape[0], dpn=x.shape[1]), dinv, dinv.abs()) < AGREE
        assert bool((mag >= y.abs()).all()) and bool((d > 0).all())


@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_iso_exact_matches_oracle_on_plain_mesh(etype):
    """Unshifted, unflipped generator meshes (8-element sample): K single / stack, mass, stress, J and gradients
    within 2e-15 of the oracle."""
    for quantity, parts in (("K", (0, 1)), ("mass", (0,)), ("stress", (0, 1)), ("geom", (0, 1))):
        for part in parts:
            assert X.iso_calibration_err(etype, "unflipped", quantity, part) < AGREE, (quantity, part)


def test_cases_are_what_they_claim():
    """81 of the 162 tets are inverted in every c3d4 case; scale1e-3 sits above the singular threshold; each
    isoparametric mesh holds both signs of detJ, constant inside an element, and its sample 4 of each."""
    for case in X.TET4_CASES:
        c, t = X.tet4_case(case)
        det = R.tet4_cofactors(c, t)[1]
        assert t.shape[0] == 162 and int((det < 0).sum()) == 81, case
    det = R.tet4_cofactors(*X.tet4_case("scale1e-3"))[1].abs().min()
    assert 2.4e-11 < float(det) < 2.6e-11
    for etype in X.ISO_TYPES:
        for case in X.ISO_CASES:
            c, e, pos, s = X.iso_case(etype, case)
            assert int(pos[s].sum()) == 4 and s.numel() == 8, (etype, case)
            if etype == "c3d10":
                assert not bool(pos[:48].any()) and bool(pos[48:].all())      # Q2: the generator's tets have detJ < 0
            else:
                assert bool(pos[0::2].all()) and not bool(pos[1::2].any())    # the reorder flips every point


def test_oracle_loses_accuracy_under_shift():
    """At a 1e6 shift the oracle's inv([1 x y z]) form (`oracle/ref_cpu.py` tet4_gradients) is off by more than 1e-11
    while the fp64 edge-difference form stays under 2e-15."""
    c, t = X.tet4_case("shift1e6")
    exact = X.tet4_exact("shift1e6", "K_elastic")
    assert X.elem_err(R.tet4_K(c, t, X.E, X.NU), exact) > 1e-11
    assert X.elem_err(X.tet4_K_edges_fp64(c, t, X.E, X.NU), exact) < AGREE


def _signed_volume_K(c, t):
    det, _ = X.tet4_geom_edges_fp64(c, t)
    return X.tet4_K_edges_fp64(c, t, X.E, X.NU) * torch.sign(det).view(-1, 1, 1)


def test_comparator_fails_wrong_restatements():
    """The GPU tests' comparison (exact_ref.check at 8 x the calibration error) passes the calibration form itself and
    fails: a signed volume on the half-flipped mesh, coordinates rounded through float32, and the absolute-coordinate
    inverse under the 1e4 shift."""
    q = "K_elastic"
    c, t = X.tet4_case("flipped")
    exact, cal = X.tet4_exact("flipped", q), X.tet4_calibration_err("flipped", q)
    X.check("edges", X.elem_err(X.tet4_K_edges_fp64(c, t, X.E, X.NU), exact), cal)
    with pytest.raises(AssertionError):
        X.check("signed volume", X.elem_err(_signed_volume_K(c, t), exact), cal)
    with pytest.raises(AssertionError):
        X.check("float32 coordinates", X.elem_err(X.tet4_K_edges_fp64(c.float().double(), t, X.E, X.NU), exact), cal)
    c, t = X.tet4_case("shift1e4")
    with pytest.raises(AssertionError):
        X.check("absolute-coordinate inverse", X.elem_err(R.tet4_K(c, t, X.E, X.NU), X.tet4_exact("shift1e4", q)),
                X.tet4_calibration_err("shift1e4", q))
    # the per-dof comparison of assembled products bites as well: the signed-volume matrices' EBE product
    c, t = X.tet4_case("flipped")
    y, _, mag, _ = X.tet4_exact("flipped", "ebe_elastic")
    with pytest.raises(AssertionError):
        X.check("signed volume, product",
                X.dof_err(R.nodal_forces(_signed_volume_K(c, t), t, X.tet4_x("flipped", "elastic")), y, mag),
                X.tet4_calibration_err("flipped", "ebe_elastic", "y"))


def test_threshold_meshes_against_oracle():
    """min|det| = 4e-12 is accepted by the oracle; one inserted tet of |det| = 2.5e-13 at index 140 is refused."""
    c, t = X.threshold_case(False)
    det = R.tet4_cofactors(c, t)[1].abs()
    assert abs(float(det.min()) / 4e-12 - 1.0) < 1e-9
    assert bool(torch.isfinite(R.tet4_K(c, t, X.E, X.NU)).all())
    c, t = X.threshold_case(True)
    det = R.tet4_cofactors(c, t)[1].abs()
    assert t.shape[0] == 163 and int(det.argmin()) == 140 and abs(float(det[140]) / 2.5e-13 - 1.0) < 1e-9
    assert int((det < 1e-12).sum()) == 1
    with pytest.raises(ValueError, match="Singular"):
        R.tet4_gradients(c, t)
