"""CPU tier of the transient solver: the dense Newmark restatement of tests/newmark_ref.py is itself checked against
closed-form facts, so that the GPU tier (tests/test_gpu_transient.py) compares the device against a reference that is
known to be right, and every ValueError of solver.transient_solver fires with no device present.

Cases elastic4, poisson6, hex4, lumped5 of modal_ref.CASES, 64 steps, dt = T_1 / 20.

Mode identity: started from a dense eigenvector phi_j with v_0 = 0, no load, no damping, beta = 1/4, gamma = 1/2, the
trapezoidal rule has the exact discrete solution u_n = phi_j cos(n theta), tan(theta / 2) = omega_j dt / 2. Bound
1e-9 max|phi_j| (the eigenvector's own error leaves two orders). Energy drift of the same run <= 64 sqrt(n) 2^-53 +
1e-12.

PCG restatement (rtol 1e-8 of every step's own right-hand side, warm start u_n) against the direct one, max over the
64 steps relative to max|u|, bound 1e-5. Measured (deviation, iterations per step min..max):
    elastic4   1.0e-08    65..110
    poisson6   3.4e-08    22..42
    hex4       2.0e-09    39..59
    lumped5    1.3e-08    81..136
The direct runs measured 1.1e-12 to 8.5e-12 on the mode identity and 3.1e-15 to 9.8e-14 of energy drift.
test_pcg_restatement prints the figures of every run.

Damped run (gamma = 0.6, beta = 0.3025, alpha = 0.05 omega_1, beta_R = 0.02 / omega_1, six-mode start): the energy
u^T K u / 2 + v^T M v / 2 never increases."""
import math

import pytest
import torch

import modal_ref as MR
import newmark_ref as NR

F64 = torch.float64


@pytest.mark.parametrize("name", NR.CASES)
def test_mode_identity_and_energy(name):
    cs = MR.case(name)
    om, phi = NR.mode(cs)
    dt = NR.step_size(cs)
    run = NR.reference(name, "mode", "direct")
    theta = 2.0 * math.atan(om * dt / 2.0)
    exact = torch.cos(theta * torch.arange(NR.STEPS + 1, dtype=F64))[:, None] * phi[None, :]
    err = float((run.u - exact).abs().max() / phi.abs().max())
    drift = run.drift()
    print(f"{name}: mode identity {err:.2e}, energy drift {drift:.2e}")
    assert err <= 1e-9, err
    assert drift <= NR.STEPS * math.sqrt(cs.n) * 2.0 ** -53 + 1e-12, drift
    assert not bool(run.u[:, ~cs.free].any())


@pytest.mark.parametrize("name", NR.CASES)
def test_pcg_restatement(name):
    d, p = NR.reference(name, "mode", "direct"), NR.reference(name, "mode", "pcg")
    dev = float((p.u - d.u).abs().max() / d.u.abs().max())
    print(f"{name}: PCG restatement deviates {dev:.2e}, iterations {min(p.iters)}..{max(p.iters)}, "
          f"energy drift {p.drift():.2e}")
    assert dev < 1e-5, dev


@pytest.mark.parametrize("name", NR.CASES)
def test_damped_energy_decays(name):
    run = NR.reference(name, "damped", "direct")
    E = run.energy
    print(f"{name}: damped energy {float(E[0]):.3e} -> {float(E[-1]):.3e}")
    assert bool((E[1:] <= E[:-1]).all()), (E[1:] - E[:-1]).max()
    assert float(E[-1]) < float(E[0])


# ---------------------------------------------------------------- validation without a device
def _inputs(dpn=3, steps=4):
    from fem355 import mesh
    c, t = mesh.kuhn_cube(1)
    N, npe = c.shape[0], 4
    K = torch.zeros((t.shape[0], dpn * npe, dpn * npe), dtype=F64)
    M = torch.zeros((t.shape[0], npe, npe), dtype=F64)
    F = torch.zeros((N, dpn), dtype=F64)
    return dict(K=K, M=M, elements=t, F=F, fixed=torch.tensor([0]), num_nodes=N, dt=1e-3, steps=steps)


BAD = {
    "K shape": lambda a: a.update(K=a["K"][:, :5, :5]),
    "M shape": lambda a: a.update(M=a["M"][:, :3, :3]),
    "dpn 2": lambda a: a.update(K=torch.zeros((a["K"].shape[0], 8, 8), dtype=F64)),
    "F shape": lambda a: a.update(F=a["F"][:-1]),
    "F history length": lambda a: a.update(F=a["F"].expand(4, -1, -1)),
    "F dims": lambda a: a.update(F=a["F"].reshape(-1)),
    "mesh outside num_nodes": lambda a: a.update(num_nodes=a["num_nodes"] - 1, F=a["F"][:-1]),
    "fixed outside": lambda a: a.update(fixed=torch.tensor([a["num_nodes"]])),
    "fixed negative": lambda a: a.update(fixed=torch.tensor([-1])),
    "record outside": lambda a: a.update(record=[0, a["num_nodes"]]),
    "dt zero": lambda a: a.update(dt=0.0),
    "dt negative": lambda a: a.update(dt=-1e-3),
    "steps zero": lambda a: a.update(steps=0),
    "beta zero": lambda a: a.update(beta=0.0),
    "gamma below half": lambda a: a.update(gamma=0.49),
    "damping negative": lambda a: a.update(damping=(-1.0, 0.0)),
    "damping not a pair": lambda a: a.update(damping=0.1),
    "amplitude length": lambda a: a.update(amplitude=torch.ones(a["steps"])),
    "amplitude type": lambda a: a.update(amplitude=2.0),
    "amplitude with history": lambda a: a.update(F=a["F"].expand(a["steps"] + 1, -1, -1).clone(),
                                                 amplitude=torch.ones(a["steps"] + 1)),
    "u0 shape": lambda a: a.update(u0=torch.zeros(3)),
    "v0 shape": lambda a: a.update(v0=torch.zeros((a["num_nodes"], 1))),
    "rtol zero": lambda a: a.update(rtol=0.0),
    "energy_every negative": lambda a: a.update(energy_every=-1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_value_errors_need_no_device(what, monkeypatch):
    from fem355 import _capi, solver

    def no_device(*a, **k):
        raise AssertionError("a device call before the validation finished")

    monkeypatch.setattr(_capi, "lib", no_device)
    monkeypatch.setattr(solver, "_dev", no_device)
    args = _inputs()
    BAD[what](args)
    with pytest.raises(ValueError):
        solver.transient_solver(**args)


def test_newmark_constants():
    from fem355 import system
    c = system.newmark_constants(0.01, 0.3025, 0.6, (2.0, 1e-3))
    assert c["coef"][:3] == [c["a0"], c["a2"], c["a3"]] and len(c["coef"]) == 12
    assert c["cK"] == 1.0 + c["a1"] * 1e-3 and c["cM"] == c["a0"] + c["a1"] * 2.0
    assert list(NR.constants(0.01, 0.3025, 0.6, 2.0, 1e-3)) == [c[f"a{i}"] for i in range(6)]
    system.newmark_constants(0.01, 0.1, 0.5)   # conditionally stable: accepted
