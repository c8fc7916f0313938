"""CPU tier: the topology-optimisation restatement (tests/topopt_ref.py) checked against itself -- the sensitivities
against central differences of the compliance with direct solves, the filter's adjoint identity, constants and volume,
the OC bisection's volume and monotonicity. The GPU tier (tests/test_gpu_topopt.py) compares the kernels with it."""
import functools

import pytest
import torch

import fem355  # noqa: F401
from fem355 import mesh
import topopt_ref as TR

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def case(n):
    c, t = mesh.kuhn_cube(n, jitter=0.15)
    m = TR.Model(c, t, 1.0, 0.3)
    F, mask = TR.cantilever(c)
    return m, F, mask


def seeded(M, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(M, dtype=F64, generator=g)


def test_apex_mesh_has_a_17_column_row():
    c, t = TR.apex_mesh()
    apex = c.shape[0] - 1
    nb = set(t[(t == apex).any(1)].reshape(-1).tolist())
    assert len(nb) == 17 and t.shape[0] == 162 + 18
    assert float(TR.Model(c, t).V.min()) > 1e-4


@pytest.mark.parametrize("passes", [0, 1, 2])
def test_sensitivities_match_central_differences(passes):
    """dc_e against (c(rho + h e_e) - c(rho - h e_e)) / 2h with direct solves. The compliance is smooth in rho; with
    h = 1e-6 the truncation error is ~h^2 c''' ~ 1e-11 relative and the rounding of c (cond(K) eps / h ~ 1e-7 at
    worst for the densities used here, which keep s >= 0.027) dominates: bound 1e-6 of the largest |dc|."""
    m, F, mask = case(2)
    d = TR.Design(m, F, mask, 0.4, passes=passes)
    rho = seeded(m.M, 0.3, 1.0, 1)
    _, dc, _, _, _ = d.compliance(rho)
    h, worst = 1e-6, 0.0
    for e in range(0, m.M, 5):
        rp, rm = rho.clone(), rho.clone()
        rp[e] += h
        rm[e] -= h
        fd = (d.compliance(rp)[0] - d.compliance(rm)[0]) / (2 * h)
        worst = max(worst, abs(fd - float(dc[e])))
    assert worst <= 1e-6 * float(dc.abs().max()), worst
    assert bool((dc < 0).all())


def test_compliance_is_load_work_and_quadratic_form():
    m, F, mask = case(2)
    d = TR.Design(m, F, mask, 0.4)
    rho = seeded(m.M, 0.3, 1.0, 2)
    c, _, _, s, u = d.compliance(rho)
    assert abs(c - float(F.reshape(-1) @ u)) <= 1e-10 * abs(c)
    assert abs(c - float(u @ (m.dense(s) @ u))) <= 1e-12 * abs(c)


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_filter_adjoint_identity_constants_and_volume(passes):
    m, _, _ = case(3)
    x, y = seeded(m.M, -1.0, 1.0, 3), seeded(m.M, -1.0, 1.0, 4)
    a, b = float(m.filter(x, passes) @ y), float(x @ m.filter_adjoint(y, passes))
    assert abs(a - b) <= 1e-13 * max(abs(a), float(x.norm() * y.norm()))
    const = torch.full((m.M,), 0.37, dtype=F64)
    assert float((m.filter(const, passes) - 0.37).abs().max()) <= 1e-15
    v0, v1 = float(m.V @ x.abs()), float(m.V @ m.filter(x.abs(), passes))
    assert abs(v0 - v1) <= 1e-14 * v0
    if passes == 0:
        assert torch.equal(m.filter(x, 0), x) and torch.equal(m.filter_adjoint(x, 0), x)


def oc_inputs(m, seed):
    rho = seeded(m.M, 1e-3, 1.0, seed)
    dc = seeded(m.M, -2.0, 0.5, seed + 1)
    dc[::7] = 0.0
    return rho, dc


@pytest.mark.parametrize("with_passive", [False, True])
def test_bisection_reaches_the_target_volume(with_passive):
    m, _, _ = case(3)
    rho, dc = oc_inputs(m, 5)
    passive = None
    if with_passive:
        passive = torch.zeros(m.M, dtype=torch.int8)
        passive[:6], passive[6:12] = 1, -1
    new, ch, vf, (lo, hi) = TR.oc_update(rho, dc, m.V, 0.5, 0.2, 1e-3, passive)
    lo_e, hi_e = TR.oc_bounds(rho, 0.2, 1e-3)
    free = torch.ones(m.M, dtype=torch.bool) if passive is None else passive == 0
    assert bool((new[free] >= lo_e[free]).all()) and bool((new[free] <= hi_e[free]).all())
    if with_passive:
        assert bool((new[passive > 0] == 1.0).all()) and bool((new[passive < 0] == 1e-3).all())
    # the bracket has closed to rounding, the feasible end is taken, and the volume is met to the last crossing
    assert hi / lo - 1.0 <= 1e-15 * 8 and vf <= 0.5 * (1 + 1e-12)
    assert abs(vf - 0.5) <= 1e-9
    assert ch == float((new - rho).abs().max())


def test_oc_volume_is_non_increasing_in_the_multiplier():
    m, _, _ = case(3)
    rho, dc = oc_inputs(m, 7)
    b = torch.clamp(-dc, min=0.0) / m.V
    lo, hi = TR.oc_bracket(b, 1e-3)
    ls = torch.logspace(torch.log10(torch.tensor(lo)).item(), torch.log10(torch.tensor(hi)).item(), 200, dtype=F64)
    vols = [float(m.V @ TR.oc_density(rho, b, float(l), 0.2, 1e-3)) for l in ls]
    assert all(v1 <= v0 for v0, v1 in zip(vols, vols[1:]))
    lo_e, hi_e = TR.oc_bounds(rho, 0.2, 1e-3)
    act = b > 0
    assert torch.equal(TR.oc_density(rho, b, lo, 0.2, 1e-3)[act], hi_e[act])
    assert torch.equal(TR.oc_density(rho, b, hi, 0.2, 1e-3), lo_e)


def test_no_descent_direction_leaves_the_density():
    m, _, _ = case(2)
    rho = seeded(m.M, 1e-3, 1.0, 9)
    new, ch, vf, br = TR.oc_update(rho, torch.rand(m.M, dtype=F64), m.V, 0.5, 0.2, 1e-3)
    assert br is None and torch.equal(new, rho) and ch == 0.0


def test_design_run_lowers_the_compliance_at_constant_volume():
    """The issue's optimisation case on the restatement: 12 iterations, direct solves."""
    m, F, mask = case(3)
    h = TR.Design(m, F, mask, 0.4).run(torch.full((m.M,), 0.4, dtype=F64), 12)
    c = h["compliance"]
    assert all(abs(v - 0.4) <= 1e-10 for v in h["volume_fraction"])
    assert all(c1 <= c0 * (1 + 1e-12) for c0, c1 in zip(c, c[1:]))
    assert c[-1] <= 0.6 * c[0]


def test_pcg_design_run_follows_the_direct_one():
    m, F, mask = case(2)
    rho0 = torch.full((m.M,), 0.4, dtype=F64)
    a = TR.Design(m, F, mask, 0.4).run(rho0, 4)
    d = TR.Design(m, F, mask, 0.4, linear="pcg", linear_rtol=1e-10)
    b = d.run(rho0, 4)
    assert float((a["density"] - b["density"]).abs().max()) <= 1e-7
    assert len(d.pcg_iterations) == 4 and all(it > 0 for it in d.pcg_iterations)
