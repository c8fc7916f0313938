"""GPU tier: the persistent PCG's diagonal-free value stream (FEM_TUNE_PK_OFFDIAG, csrc/sell_pair.hpp k_sell_offdiag,
csrc/pcg_persist.hpp OD build). The diagonal of a slice-uniform slice is kept in registers and its term is added at
its list position, so every row sum adds the same products in the same order: iterates, r.z and iteration counts
must equal the flag-off build's bit for bit. Every mesh is jittered (on the regular cube all interior diagonals are
equal, so a diagonal taken from the wrong lane or slot would pass). References that do not run the new code: the
three-kernel schedule on the unchanged matrix (1e-12 relative: its reductions sum in another order), the oracle
(oracle/ref_cpu.py) for the full solve, and the flag-off build for bit identity."""
import functools

import pytest
import torch

from conftest import rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
OFFDIAG = 32768   # FEM_TUNE_PK_OFFDIAG
WIDE = 256        # FEM_TUNE_PK_WIDE
SC1 = 4           # FEM_TUNE_PK_SC1


def _mods():
    import fem355  # noqa: F401
    from fem355 import _capi, element, mesh, system
    return _capi, element, mesh, system


def _cube(n, gpu, permute=None):
    C, _, mesh, system = _mods()
    c, t = mesh.kuhn_cube(n, jitter=0.1)
    if permute is not None:
        N = c.shape[0]
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(permute))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(N)
        c, t = c[perm], inv[t]
    f, fixed = mesh.cube_poisson_case(c)
    A = system.assemble_tet4_system(c.to(gpu), t.to(gpu), "poisson")
    mask = torch.zeros(A.n, dtype=torch.uint8, device=gpu)
    mask[fixed.to(gpu)] = 1
    b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(3)).to(gpu)
    return A, b, mask, (c, t, f, fixed)


@functools.lru_cache(maxsize=1)
def _cube20(gpu):
    """The n = 20 cube (9,261 rows, 145 slices) shared by the cases that use it, with its three-kernel references."""
    C, _, _, _ = _mods()
    A, b, mask, _ = _cube(20, gpu)
    w = A.jacobi(mask)
    wm = (mask == 0).to(F64)
    ref = {"pcg": A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=40, schedule=0).x,
           "cg": A.pcg(b, w=wm, mode=C.MODE_CG_STABLE, tol=0.0, max_iter=40, schedule=0).x}
    return A, b, w, wm, ref


def _run(A, b, w, flags, chunks, mode=1):
    """Fixed iterations on schedule 3 with the given flag set -> (facts, poll, x)."""
    _, _, _, system = _mods()
    run = system.PcgRunner(A, b, w, mode=mode, tol=0.0, schedule=3)
    try:
        run.set_tuning(flags)
        run.start()
        assert run.effective_schedule() == 3
        facts = {"od": run.offdiag_slices(), "uni": run.uniform_slices(), "build": run.persist_build()}
        for k in chunks:
            run.iterate(k)
        poll = run.poll()
        assert poll[0] == sum(chunks) and poll[1] == 0
        return facts, poll, run.x.clone()
    finally:
        run.close()


def _expected_build(nrows, wide):
    """(slots, overflow, pack) of fem_pcg_persist_build for this device: one workgroup per CU (a multiple of 8), 16
    waves each, 7 register slots per wave."""
    G = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    ns = -(-nrows // 64)
    pack = -(-(-(-ns // G)) // 16)
    ovf = int(ns > G * 16 * 7)
    slots = 7 if (wide or ovf or pack > 4) else (1 if pack == 1 else 2 if pack == 2 else 4)
    return slots, ovf, pack


@pytest.mark.parametrize("mode", ["pcg", "cg_masked"])
def test_mixed_slices_match_three_kernel_and_flag_off(gpu, mode):
    """n = 20: diagonal-free slices beside slices that keep their diagonal (the mesh's first and last ones). 40 fixed
    iterations, PCG mode and CG mode with masked (w = 0) rows."""
    C, _, _, _ = _mods()
    A, b, w, wm, ref = _cube20(gpu)
    wt, md = (w, C.MODE_PCG) if mode == "pcg" else (wm, C.MODE_CG_STABLE)
    on, p1, x1 = _run(A, b, wt, C.TUNE_DEFAULT, (40,), md)
    off, p0, x0 = _run(A, b, wt, C.TUNE_DEFAULT & ~OFFDIAG, (40,), md)
    od, ns, nbytes = on["od"]
    assert ns == 145 and 0 < od < ns and od <= on["uni"][0] < ns, on
    assert nbytes == od * 64 * 8
    assert off["od"] == (0, 145, 0)
    assert torch.equal(x1, x0) and p1 == p0
    assert rel(x1, ref["pcg" if mode == "pcg" else "cg"]) < 1e-12


def test_chunked_launches_are_bit_identical(gpu):
    """The same 40 iterations as one launch, as 10 + 10 + 20 and as 1 + 39: the state, the diagonal included, goes out
    and comes back intact."""
    C, _, _, _ = _mods()
    A, b, w, _, ref = _cube20(gpu)
    outs = [_run(A, b, w, C.TUNE_DEFAULT, ch) for ch in ((40,), (10, 10, 20), (1, 39))]
    for _, p, x in outs[1:]:
        assert p == outs[0][1] and torch.equal(x, outs[0][2])
    assert rel(outs[0][2], ref["pcg"]) < 1e-12


@pytest.mark.parametrize("n,wide", [(20, False), (40, False), (64, False), (80, False), (20, True), (64, True),
                                    (122, False)])
def test_every_build(gpu, n, wide):
    """Every build of the kernel: one slot (n = 20, 40), two slices per wave (n = 64: 274,625 rows), three (n = 80: the
    four-slot build), the 7-slot build with several occupied slots (FEM_TUNE_PK_WIDE), and the overflow build (n = 122:
    1,860,867 rows, the smallest cube past the 1,835,008-row register capacity of 256 workgroups)."""
    C, _, _, _ = _mods()
    if n == 20:
        A, b, w, _, _ = _cube20(gpu)
    else:
        A, b, mask, _ = _cube(n, gpu)
        w = A.jacobi(mask)
    k = 24
    flags = C.TUNE_DEFAULT | (WIDE if wide else 0)
    on, p1, x1 = _run(A, b, w, flags, (k,))
    assert on["build"] == _expected_build(A.n, wide), on
    assert on["od"][0] > 0 and on["od"][2] == on["od"][0] * 512, on
    off, p0, x0 = _run(A, b, w, flags & ~OFFDIAG, (k,))
    assert off["build"] == on["build"] and off["od"][0] == 0
    assert torch.equal(x1, x0) and p1 == p0
    x3 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=k, schedule=0).x
    assert rel(x1, x3) < 1e-12


@pytest.mark.parametrize("drop", [0, OFFDIAG, SC1], ids=["default", "offdiag_off", "sc1_off"])
def test_instrumented_builds(gpu, drop):
    """The phase-clock (PROF) builds, which otherwise run only from tools/: 24 fixed iterations through
    fem_pcg_persist_profile with the default flags, without the diagonal-free stream and without the sc1 gathers.
    The clocks tick, and x equals bit for bit the plain run of the same 7-slot build (FEM_TUNE_PK_WIDE)."""
    import ctypes
    C, _, _, system = _mods()
    A, b, w, _, _ = _cube20(gpu)
    flags = C.TUNE_DEFAULT & ~drop
    G = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8   # one workgroup per CU
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.set_tuning(flags)
        run.start()
        assert run.effective_schedule() == 3
        buf = (ctypes.c_ulonglong * (G * (8 + 16)))()   # [G][8 phases] then [G][16 waves]
        g = ctypes.c_int()
        C.check(run.lib.fem_pcg_persist_profile(run.h, 24, buf, ctypes.byref(g)), "fem_pcg_persist_profile")
        poll = run.poll()
        x = run.x.clone()
    finally:
        run.close()
    assert g.value == G
    assert poll[0] == 24 and poll[1] == 0
    assert buf[1] != 0   # workgroup 0, phase 1: the SpMV
    _, _, x0 = _run(A, b, w, flags | WIDE, (24,))
    assert torch.equal(x, x0)


def test_no_qualifying_slice(gpu):
    """A seeded random renumbering of the n = 20 cube has no slice-uniform slice: nothing is left out, same bits."""
    C, _, _, _ = _mods()
    A, b, mask, _ = _cube(20, gpu, permute=11)
    w = A.jacobi(mask)
    on, p1, x1 = _run(A, b, w, C.TUNE_DEFAULT, (30,))
    off, p0, x0 = _run(A, b, w, C.TUNE_DEFAULT & ~OFFDIAG, (30,))
    assert on["od"] == (0, 145, 0), on
    assert torch.equal(x1, x0) and p1 == p0
    assert rel(x1, A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=30, schedule=0).x) < 1e-12


def test_full_solve_vs_oracle(gpu):
    """n = 30 jittered, Jacobi-PCG to rtol 1e-8: against the oracle's R.pcg iterations within +-2 and u within 1e-10
    (the project's contract); against flag off the same iteration count exactly (and the same bits)."""
    C, _, _, _ = _mods()
    A, _, mask, (c, t, f, fixed) = _cube(30, gpu)
    w = A.jacobi(mask)
    b = f.reshape(-1).to(gpu).to(F64)
    tol = 1e-8 * float(torch.sqrt(torch.dot(b, w * b)))
    r1 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=C.TUNE_DEFAULT)
    r0 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=C.TUNE_DEFAULT & ~OFFDIAG)
    assert r1.status == r0.status == C.PCG_CONVERGED
    assert r1.iterations == r0.iterations and torch.equal(r1.x, r0.x)
    K = R.tet4_poisson_K(c, t)
    dinv = R.diag_preconditioner(K, t, c.shape[0], dpn=1)
    dinv[fixed] = 0.0
    u_ref, it_ref, st = R.pcg(K, t, f.to(F64), dinv, tol=tol, max_iter=5000)
    assert st == "converged" and abs(r1.iterations - it_ref) <= 2, (r1.iterations, it_ref)
    assert rel(r1.x, u_ref.reshape(-1)) < 1e-10


@pytest.mark.parametrize("case", ["kuhn20", "tet10_mass"])
def test_layout_round_trip(gpu, case):
    """The plain SELL values rebuilt from the diagonal-free stream and the dense diagonal equal plain_values() bit for
    bit: the n = 20 cube, and the scalar mass of a small tet10 cube (mixed odd and even slice widths)."""
    C, element, mesh, system = _mods()
    if case == "kuhn20":
        A, b, w, _, _ = _cube20(gpu)
    else:
        c, e = mesh.tet10_cube(5, jitter=0.1)
        c, e = c.to(gpu), e.to(gpu)
        Me = element.compute_M_matrix(c, e, "c3d10", 7850.0, device=gpu, dtype=F64, scalar=True)
        A = system.SellMatrix(system.build_graph(e, c.shape[0]), 1).add_element_matrices(Me, e)
        b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(4)).to(gpu)
        w = A.jacobi(None)
        sp = A.g.slice_ptr.cpu()
        widths = ((sp[1:] - sp[:-1]) // 64).tolist()
        assert any(x % 2 for x in widths) and any(x % 2 == 0 for x in widths), widths
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.start()
        assert run.effective_schedule() == 3
        od = run.offdiag_slices()
        vals = run.debug_offdiag_values()
    finally:
        run.close()
    if case == "kuhn20":
        assert od[0] > 0
    plain = A.plain_values()
    assert torch.equal(vals.view(torch.int64)[: plain.numel()], plain.view(torch.int64)), od
