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


# ----------------------------------------------------------------------------- third generation (tests/exact_ref3.py)
import exact_ref3 as X3  # noqa: E402

C3D4_QUANTITIES3 = [("xd_" + m, p) for m in X3.XD_MATERIALS for p in ("f", "w")] + \
    [("mass", None), ("dt", None), ("vol", None), ("energy", "ce"), ("energy", "dct"), ("energy", "c"), ("matvec", None)]


def _shell_quantities(etype):
    q = [("geom", p) for p in X3.SHELL_GEOM_PARTS] + [("K", p) for p in X3.SHELL_K_PARTS if etype == "s4" or p != "points"]
    return q + [("stress", None), ("apply", None)]


def test_exact3_matches_restatements_on_plain_c3d4_mesh():
    """Unflipped unit mesh: the exact explicit force, energy, lumped mass and step and the exact topopt volumes, unit
    energy, sensitivities, compliance and scaled product within 1e-12 of explicit_ref, hyperelastic_ref and topopt_ref
    as their own tests use them."""
    import explicit_ref as XR
    import hyperelastic_ref as HR
    import topopt_ref as TR
    case = "unflipped"
    c, t = X.tet4_case(case)
    for mat in X3.XD_MATERIALS:
        f, mag, w = X3.tet4_exact3(case, "xd_" + mat)
        u = X3.xd_u(case, mat)
        m = XR.Model(c, t, X3.E, X3.NU, mat)
        assert X.dof_err(m.f_int(u.reshape(-1)).view(-1, 3), f, mag) < RESTATE, mat
        assert X3.rel_err(m.energy(u.reshape(-1)), w) < RESTATE, mat
        assert bool((mag >= f.abs()).all()) and w > 0
        if mat != "linear":
            hm = HR.Model(c, t, X3.E, X3.NU, mat)
            assert X.dof_err(hm.f_int(u), f, mag) < RESTATE and X3.rel_err(hm.energies(u).sum(), w) < RESTATE
    assert X3.node_err(XR.lumped_mass(c, t, X3.RHO), X3.tet4_exact3(case, "mass")) < RESTATE
    dt, dte = XR.element_dt(c, t, X3.E, X3.NU, X3.RHO)
    assert X3.node_err(dte, X3.tet4_exact3(case, "dt")) < RESTATE and dt == float(dte.min())
    m = TR.Model(c, t, X3.E, X3.NU)
    rho_t = X3.to_rho_t(t.shape[0])
    assert 0.2 <= float(rho_t.min()) and float(rho_t.max()) <= 1.0
    s = TR.simp(rho_t, X3.PENAL, X3.S_MIN)
    assert X3.node_err(s, X.to_tensor(X3.simp_fr(rho_t))) < AGREE
    ce_ex, dct_ex, c_ex = X3.tet4_exact3(case, "energy")
    ce = m.unit_energy(X.tet4_u(case).reshape(-1))
    assert X3.node_err(m.V, X3.tet4_exact3(case, "vol")) < RESTATE and X3.node_err(ce, ce_ex) < RESTATE
    dct = -X3.PENAL * (1.0 - X3.S_MIN) * rho_t ** (X3.PENAL - 1.0) * X3.E * ce
    assert X3.node_err(dct, dct_ex) < RESTATE and X3.rel_err((s * X3.E * ce).sum(), c_ex) < RESTATE
    y_ex, mag = X3.tet4_exact3(case, "matvec")
    assert X.dof_err(m.dense(s) @ X.tet4_x(case, "elastic").reshape(-1), y_ex, mag) < RESTATE
    for q, part in C3D4_QUANTITIES3:
        assert X3.tet4_calibration_err3(case, q, part) < RESTATE, (q, part)


def test_exact3_matches_shell_ref_and_the_recorded_elements():
    """Plain patch: every exact shell quantity within 1e-12 of tests/shell_ref.py. The eight recorded elements of
    tests/golden/shell_cells.npz per family: exact K, the s4 points' terms, frames, local coordinates, J and gradients
    within 1e-12 of the recording."""
    import shell_ref as SR
    from conftest import load_golden
    for etype in X3.SHELL_TYPES:
        for q, part in _shell_quantities(etype):
            assert X3.shell_calibration_err(etype, "plain", q, part) < RESTATE, (etype, q, part)
    g = load_golden("shell_cells")
    mem, ben = X3.shell_params()
    assert torch.equal(mem, g["membrane"]) and torch.equal(ben, g["bending"])
    Xr = X._rows(g["coords"])
    for etype in X3.SHELL_TYPES:
        Ks, Ps, units, locs = [], [], [], []
        for el in g[etype].tolist():
            xe = [Xr[n] for n in el]
            terms, unit = X3.shell_K_terms_fr(xe)
            Ks.append(X3._sum_terms(terms))
            Ps.append([[[T[i][j] for T in terms] for j in range(len(Ks[-1]))] for i in range(len(Ks[-1]))])
            units.append(unit)
            locs.append(X3.shell_frame_fr(xe)[1])
        assert X.elem_err(g[etype + "_K"], X.to_tensor(Ks)) < RESTATE
        assert X.elem_err(g[etype + "_unit"], X.to_tensor(units)) < RESTATE
        assert X.elem_err(g[etype + "_local"], X.to_tensor(locs)) < RESTATE
        if etype == "s4":
            assert X.elem_err(g["s4_K_points"], X.to_tensor(Ps)) < RESTATE
            for p, f in enumerate(SR.k_factors()):
                Jg = [X3.shell_point_fr(loc, f) for loc in locs]
                assert X.elem_err(g["s4_J"][..., p], X.to_tensor([o[0] for o in Jg])) < RESTATE
                assert X.elem_err(g["s4_grads"][..., p], X.to_tensor([o[2] for o in Jg])) < RESTATE
        else:
            Jg = [X3.shell_point_fr(loc) for loc in locs]
            assert X.elem_err(g["s3_J"], X.to_tensor([o[0] for o in Jg])) < RESTATE
            assert X.elem_err(g["s3_grads"], X.to_tensor([o[2] for o in Jg])) < RESTATE


def _shell_aspect(c, conn):
    """Longest edge squared over twice the area of the (first) triangle / the area spanned by the quad's diagonals."""
    x = c[conn]
    npe = conn.shape[1]
    L2 = max(float(((x[:, (k + 1) % npe] - x[:, k]) ** 2).sum(1).max()) for k in range(npe))
    if npe == 3:
        area2 = torch.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], dim=1).norm(dim=1)
    else:
        area2 = 0.5 * torch.cross(x[:, 2] - x[:, 0], x[:, 3] - x[:, 1], dim=1).norm(dim=1)
    lmax2 = torch.stack([((x[:, (k + 1) % npe] - x[:, k]) ** 2).sum(1) for k in range(npe)], 1).max(1).values
    assert L2 == float(lmax2.max())
    return lmax2 / area2


def test_cases3_are_what_they_claim():
    """The c3d4 cases hold 81 negative dets (and "unflipped" none). The shell cases: 72 s4 / 144 s3 elements on 90
    nodes, every second element started one place further round, every quad non-planar in exact arithmetic (plain:
    node 2 lies at least 1e-4 of the element's size off the plane of the frame), aspect ratios below 10 on the
    well-shaped cases and between 3e3 and 1e5 on the squashed ones, and the shifted patches 1e4 / 1e6 from the
    origin; the samples hold elements 0, 63, 64, the last and both start orders."""
    for case in X.TET4_CASES:
        c, t = X.tet4_case(case)
        assert int((R.tet4_cofactors(c, t)[1] < 0).sum()) == 81, case
    assert int((R.tet4_cofactors(*X.tet4_case("unflipped"))[1] < 0).sum()) == 0
    c0, quads = X3.shell_unit_patch()
    assert c0.shape == (90, 3) and quads.shape == (72, 4)
    for etype, M in (("s4", 72), ("s3", 144)):
        s = X3.SHELL_SAMPLE[etype]
        assert len(set(s)) == 8 and {0, 63, 64, M - 1} <= set(s) and {e % 2 for e in s} == {0, 1}
        for case in X3.SHELL_CASES:
            c, conn = X3.shell_case(etype, case)
            assert conn.shape == (M, int(etype[1])) and c.shape == (90, 3), (etype, case)
            base = quads if etype == "s4" else torch.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(M, 3)
            assert torch.equal(conn[0::2], base[0::2]) and torch.equal(conn[1::2], base[1::2].roll(-1, 1))
            asp = _shell_aspect(c, conn)
            if case.startswith("squash"):
                assert 3e3 < float(asp.min()) and float(asp.max()) < 1e5, (etype, case, float(asp.min()), float(asp.max()))
            else:
                assert float(asp.max()) < 10.0, (etype, case, float(asp.max()))
            if case.startswith("shift"):
                d = c.norm(dim=1) / float(case[5:])
                assert 1.2 < float(d.min()) and float(d.max()) < 1.3, (case, float(d.min()))
            if etype == "s4":
                Xr = X._rows(c)
                for el in conn.tolist():
                    p = [Xr[n] for n in el]
                    vol = X._dot(X._sub(p[1], p[0]), X._cross(X._sub(p[2], p[0]), X._sub(p[3], p[0])))
                    assert vol != 0, (case, el)
    import shell_ref as SR
    _, loc = SR.geometry(*X3.shell_case("s4", "plain"))
    assert float((loc[:, 2, 2].abs() / loc[:, :, :2].abs().amax((1, 2))).min()) > 1e-4


def test_stable_step_reference_is_below_the_dense_bound():
    """Where the dense eigenproblem is well conditioned (flipped, shift1e4, scale1e-3, scale1e3) the exact element
    step's minimum is below 2 / omega_max of explicit_ref's lumped-mass pencil: the GPU test asserts it of the device."""
    import explicit_ref as XR
    for case in ("flipped", "shift1e4", "scale1e-3", "scale1e3"):
        c, t = X.tet4_case(case)
        dt = float(X3.tet4_exact3(case, "dt").min())
        bound = 2.0 / XR.omega_max(c, t, X3.E, X3.NU, X3.RHO)
        assert 0.0 < dt <= bound and dt > 0.25 * bound, (case, dt, bound)


def _s4_frame_b_from_node_2(coords, conn):
    import shell_ref as SR
    return SR.frame(coords, conn[:, [0, 1, 3, 2]])


def _gradients_transposed(local, f=None):
    import shell_ref as SR
    dxi, det = SR.param_derivs(local.shape[1], f)
    Ji = torch.inverse(SR.jacobian(local, f))
    return torch.einsum("mba,nb->mna", Ji, torch.stack([dxi, det], -1))


def test_comparator_fails_wrong_restatements3():
    """exact_ref.check at 8 x the calibration error rejects: an explicit force with the signed volume V = det / 6, a
    lumped mass with det for |det|, a stable step without g_0 (half-flipped c3d4 mesh); an s4 frame whose b comes from
    node 2 and gradients contracted with J^-T for the reference's J^-1 (plain shell patch). The calibration forms
    themselves pass."""
    import shell_ref as SR
    case = "flipped"
    c, t = X.tet4_case(case)
    det, g = X.tet4_geom_edges_fp64(c, t)
    for mat in X3.XD_MATERIALS:
        f_ex, mag, _ = X3.tet4_exact3(case, "xd_" + mat)
        cal = X3.tet4_calibration_err3(case, "xd_" + mat, "f")
        u = X3.xd_u(case, mat)
        X.check("edges", X.dof_err(X3.force_fp64(c, t, u, mat, det.abs() / 6.0, g)[0], f_ex, mag), cal)
        with pytest.raises(AssertionError):
            X.check("signed volume", X.dof_err(X3.force_fp64(c, t, u, mat, det / 6.0, g)[0], f_ex, mag), cal)
    with pytest.raises(AssertionError):
        X.check("mass with det", X3.node_err(X3.mass_fp64(c, t, det / 6.0), X3.tet4_exact3(case, "mass")),
                X3.tet4_calibration_err3(case, "mass"))
    with pytest.raises(AssertionError):
        X.check("step without g_0", X3.node_err(X3.dt_fp64(g[:, 1:]), X3.tet4_exact3(case, "dt")),
                X3.tet4_calibration_err3(case, "dt"))
    c, conn = X3.shell_case("s4", "plain")
    ex = X3.shell_exact("s4", "plain", "geom")
    X.check("frame", X.elem_err(SR.frame(c, conn), ex[0]), X3.shell_calibration_err("s4", "plain", "geom", "unit"))
    with pytest.raises(AssertionError):
        X.check("b from node 2", X.elem_err(_s4_frame_b_from_node_2(c, conn), ex[0]),
                X3.shell_calibration_err("s4", "plain", "geom", "unit"))
    for etype in X3.SHELL_TYPES:
        c, conn = X3.shell_case(etype, "plain")
        f = None if etype == "s3" else X3.shell_geom_factors()
        _, loc = SR.geometry(c, conn)
        with pytest.raises(AssertionError):
            X.check("J^-T", X.elem_err(_gradients_transposed(loc, f), X3.shell_exact(etype, "plain", "geom")[3]),
                    X3.shell_calibration_err(etype, "plain", "geom", "grads"))


def test_exact3_calibration_errors():
    """The calibration errors of every (quantity, case) of the third generation. c3d4: the restatements on
    edge-difference gradients stay below 1e-14 on every case but the rotated sliver. Shells: shell_ref stays below
    1e-14 off the squashed cases (it differences from node 0, so a shift costs nothing) and loses what the projection
    b - (a.b / a.a) a of a 1e4 : 1 sliver loses, 1e-11, on them."""
    for case in X.TET4_CASES:
        for q, part in C3D4_QUANTITIES3:
            err = X3.tet4_calibration_err3(case, q, part)
            print(f"CALIB c3d4 {q} {part} {case}: {err:.2e}")
            assert err == err and err < 1.0
            if case != "squash1e-4_rot":
                assert err < C3D4_CALIBRATION, (case, q, part, err)
    for etype in X3.SHELL_TYPES:
        for case in X3.SHELL_CASES:
            for q, part in _shell_quantities(etype):
                err = X3.shell_calibration_err(etype, case, q, part)
                print(f"CALIB {etype} {q} {part} {case}: {err:.2e}")
                assert err == err and err < (1e-10 if case.startswith("squash") else C3D4_CALIBRATION), (etype, case, q)
