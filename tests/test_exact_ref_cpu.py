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


# ----------------------------------------------------------------------------- second generation (tests/exact_ref2.py)
import exact_ref2 as X2  # noqa: E402

RESTATE = 1e-12
C3D4_CALIBRATION = 1e-14


def _tet4_quantities():
    """[(quantity, parts)] of exact_ref2.tet4_exact2."""
    q = [("hyper_" + m, X2.HYPER_PARTS) for m in X2.MATERIALS]
    q += [("j2_" + w, X2.J2_PARTS) for w in ("virgin", "hardened")]
    q += [("geo_" + m, (None,)) for m in X2.GEO_MODES]
    q += [("body_" + m, (None,)) for m in X2.BODY_MODES] + [("thermal_" + m, (None,)) for m in X2.T_MODES]
    q += [("surface_" + m, (None,)) for m in X2.SURF_MODES] + [("tstress_" + m, (0, 1)) for m in X2.T_MODES]
    return q


def _iso_quantities(etype):
    q = [("geo_" + m, (None,)) for m in X2.GEO_MODES] + [("body_" + m, (None,)) for m in X2.BODY_MODES]
    if etype in X2.ISO_THERMAL:
        q += [("thermal_" + m, (None,)) for m in X2.T_MODES] + [("surface_" + m, (None,)) for m in X2.SURF_MODES]
        q += [("tstress_" + m, (0, 1)) for m in X2.T_MODES]
    return q


def test_exact2_matches_restatements_on_plain_c3d4_mesh():
    """Unflipped unit mesh: the exact hyperelastic, J2, geometric-stiffness and load references within 1e-12 per
    element (per dof of the magnitude sum for the load vectors) of the fp64 restatements as their own tests use them."""
    import buckling_ref as BR
    import hyperelastic_ref as HR
    import loads_ref as LR
    import plasticity_ref as PR
    case = "unflipped"
    c, t = X.tet4_case(case)
    s = torch.tensor(X2.TANGENT_SAMPLE)
    for mat in X2.MATERIALS:
        ex, u = X2.tet4_exact2(case, "hyper_" + mat), X2.hyper_u(case)
        m = HR.Model(c, t, X2.E, X2.NU, mat)
        fe, Kt = m.element_forces_tangents(u)
        assert X.elem_err(HR.closed_form_tangent(m, u)[s], ex["Kt"]) < RESTATE
        assert X.elem_err(Kt[s], ex["Kt"]) < RESTATE and X.elem_err(fe, ex["fe"]) < RESTATE
        assert X.elem_err(m.energies(u), ex["we"]) < RESTATE and X.elem_err(m.cauchy(u), ex["sigma"]) < RESTATE
        Fm, J = m.deformation(u)
        assert X.elem_err(Fm, ex["F"]) < RESTATE and X.elem_err(J, ex["detF"]) < RESTATE
    assert PR.material("bench") == (X2.E, X2.NU, X2.SIGMA_Y, X2.HARD)
    for which in ("virgin", "hardened"):
        ex = X2.tet4_exact2(case, "j2_" + which)
        o = PR.Model(c, t, *PR.material("bench")).element(X2.j2_u(case, which), X2.j2_state(case, which))
        assert X.elem_err(o["Kt"][s], ex["Kt"]) < RESTATE
        for k in ("fe", "we", "sigma", "ep", "alpha", "f_tr"):
            assert X.elem_err(o[k], ex[k]) < RESTATE, (which, k)
        assert torch.equal(o["plastic"], ex["plastic"])
    u, s0 = X.tet4_u(case), X2.sigma0(t.shape[0])
    for mode in X2.GEO_MODES:
        ua, sa = X2._geo_args(mode, u, s0)
        Gs = BR.geo_scalar(c, t, "c3d4", ua, X2.E, X2.NU, sa)
        assert X.elem_err(Gs, X2.tet4_exact2(case, "geo_" + mode)) < RESTATE
    li = X2.load_inputs(c.shape[0], t.shape[0])
    for mode in X2.BODY_MODES:
        F, mag = X2.tet4_exact2(case, "body_" + mode)
        assert X.dof_err(LR.body_force(c, t, "c3d4", X2.RHO, li[mode]), F, mag) < RESTATE
        assert bool((mag >= F.abs()).all())
    for mode in X2.T_MODES:
        F, mag = X2.tet4_exact2(case, "thermal_" + mode)
        assert X.dof_err(LR.thermal_load(c, t, "c3d4", X2.E, X2.NU, X2.ALPHA_T, li[mode], X2.T_REF), F, mag) < RESTATE
        sig, vm = X2.tet4_exact2(case, "tstress_" + mode)
        rs, rv = LR.thermal_stress(c, t, "c3d4", X2.thermal_u(u), X2.E, X2.NU, X2.ALPHA_T, li[mode], X2.T_REF)
        assert X.elem_err(rs, sig) < RESTATE and X.elem_err(rv, vm) < RESTATE
    for mode in X2.SURF_MODES:
        assert X2.tet4_calibration_err2(case, "surface_" + mode) < RESTATE


@pytest.mark.parametrize("etype", X.ISO_TYPES)
def test_exact2_matches_restatements_on_plain_iso_mesh(etype):
    """Unflipped generator meshes: geometric stiffness (8-element sample), body force and -- where loads.py builds
    them -- thermal load, surface loads and thermal stress within 1e-12 of buckling_ref.geo_scalar / loads_ref."""
    for q, parts in _iso_quantities(etype):
        for part in parts:
            assert X2.iso_calibration_err2(etype, "unflipped", q, part) < RESTATE, (q, part)


def test_exact2_tangents_reduce_to_the_linear_stiffness():
    """As Fractions, on the tangent sample of the half-flipped mesh: the svk and neo-Hooke tangents at u = 0 and the
    J2 tangent of an all-elastic field are tet4_K_fr(..., "elastic") exactly."""
    c, t = X.tet4_case("flipped")
    K = X.tet4_K_fr(c, t, "elastic", X2.E, X2.NU)
    want = [K[e] for e in X2.TANGENT_SAMPLE]
    zero = torch.zeros_like(c)
    for mat in X2.MATERIALS:
        o = X2.tet4_hyper(c, t, zero, mat, tangent_of=X2.TANGENT_SAMPLE)
        assert o["Kt_fr"] == want
        assert not bool(o["fe"].any()) and not bool(o["we"].any())
    o = X2.tet4_j2(c, t, 1e-3 * X2.j2_u("flipped", "virgin"), tangent_of=X2.TANGENT_SAMPLE)
    assert not bool(o["plastic"].any())
    assert o["Kt_fr"] == want


def test_exact2_input_conditions():
    """Every case: 0.5 <= J <= 2 on every element of the hyperelastic field; 25-75 % of the elements yield under each
    J2 field with |f_tr| >= 1e-6 sigma_y everywhere (the exact reference alone decides); the tangent sample holds 8
    elements of each orientation and element 161."""
    det = R.tet4_cofactors(*X.tet4_case("flipped"))[1][torch.tensor(X2.TANGENT_SAMPLE)]
    assert int((det > 0).sum()) == 8 and len(set(X2.TANGENT_SAMPLE)) == 16 and 161 in X2.TANGENT_SAMPLE
    for case in X.TET4_CASES:
        for J in X2.tet4_exact2(case, "hyper_svk")["J_fr"]:
            assert 0.5 <= J <= 2, (case, float(J))
        for which in ("virgin", "hardened"):
            o = X2.tet4_exact2(case, "j2_" + which)
            share = float(o["plastic"].to(F64).mean())
            assert 0.25 <= share <= 0.75, (case, which, share)
            assert float(o["f_tr"].abs().min()) >= 1e-6 * X2.SIGMA_Y, (case, which)
        assert float(X2.j2_state(case, "hardened")[1].max()) > 0.0


def test_exact2_calibration_errors():
    """The calibration errors of every (quantity, case). c3d4: the restatements on edge-difference gradients stay below
    1e-14 on every case but the rotated sliver (the calibration form is not itself the lossy one)."""
    for case in X.TET4_CASES:
        for q, parts in _tet4_quantities():
            for part in parts:
                err = X2.tet4_calibration_err2(case, q, part)
                print(f"CALIB c3d4 {q} {part} {case}: {err:.2e}")
                assert err == err and err < 1.0
                if case != "squash1e-4_rot":
                    assert err < C3D4_CALIBRATION, (case, q, part, err)
    for etype in X.ISO_TYPES:
        for case in X.ISO_CASES:
            for q, parts in _iso_quantities(etype):
                for part in parts:
                    err = X2.iso_calibration_err2(etype, case, q, part)
                    print(f"CALIB {etype} {q} {part} {case}: {err:.2e}")
                    assert err == err and err < 1.0
