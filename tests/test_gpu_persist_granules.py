"""GPU tier: the persistent PCG's reduction through tagged granules (FEM_TUNE_PK_GRAN, csrc/pcg_persist_sync.hpp
pk_gran_*, csrc/pcg_persist.hpp). Every workgroup publishes its d and g partials as {epoch, half a double} granules;
wave 0 of every workgroup re-reads the d records it misses, and its last wave the g records, until all carry the
epoch, then sums them in the counter barrier's order (in the builds the default flag set reaches; every other build
keeps the barrier). Every iterate must equal the flag-off run's bit for bit, across launch boundaries of either epoch
parity, in every build, under uneven arrival, through every stop, on a restarted context (stale tags zeroed) and when
the flag changes between launches. References that run none of the new code: the flag-off run (the counter barrier;
bit identity of x and of the poll tuple) and the three-kernel schedule (1e-12 relative: its reductions sum in another
order). The matrices are those of test_gpu_persist_desc.py (jittered cubes, the strip matrix of uneven slice
widths)."""
import ctypes
import functools

import pytest
import torch

from conftest import rel
from test_gpu_persist_desc import _cube, _cube20, _expected_build, _strip

pytestmark = pytest.mark.gpu
F64 = torch.float64
GRAN = 131072     # FEM_TUNE_PK_GRAN
SMALL = 262144    # FEM_TUNE_PK_GRAN_SMALL: the two- and four-slot builds too (opt-in)
WIDE = 256        # FEM_TUNE_PK_WIDE


def _mods():
    import fem355  # noqa: F401
    from fem355 import _capi, system
    return _capi, system


def _run(A, b, w, flags, chunks, mode=1):
    """Fixed iterations on schedule 3 with the given flag set -> (facts, poll, x)."""
    _, system = _mods()
    run = system.PcgRunner(A, b, w, mode=mode, tol=0.0, schedule=3)
    try:
        run.set_tuning(flags)
        run.start()
        assert run.effective_schedule() == 3
        facts = {"gran": run.persist_granules(), "build": run.persist_build()}
        for k in chunks:
            run.iterate(k)
        poll = run.poll()
        assert poll[0] == sum(chunks) and poll[1] == 0
        return facts, poll, run.x.clone()
    finally:
        run.close()


def _on(extra=0):
    """The default flag set with the granule reduction in every build that has one."""
    C, _ = _mods()
    return C.TUNE_DEFAULT | GRAN | SMALL | extra


def _off(extra=0):
    C, _ = _mods()
    return (C.TUNE_DEFAULT & ~(GRAN | SMALL)) | extra


def _same(x1, x0):
    return torch.equal(x1.view(torch.int64), x0.view(torch.int64))


@functools.lru_cache(maxsize=1)
def _cube20_off(gpu):
    """40 flag-off iterations on the n = 20 cube, one launch: what every chunking below must reproduce."""
    C, _ = _mods()
    A, b, w, _, _ = _cube20(gpu)
    return _run(A, b, w, _off(), (40,))


def test_flag_is_in_the_default_set():
    C, _ = _mods()
    assert C.TUNE_PK_GRAN == GRAN and C.TUNE_DEFAULT & GRAN
    assert C.TUNE_PK_GRAN_SMALL == SMALL and not C.TUNE_DEFAULT & SMALL


@pytest.mark.parametrize("n,want", [(20, True), (64, False), (80, False)])
def test_default_set_by_build(gpu, n, want):
    """The default flag set reduces through granules in the one-slot build and keeps the counter barrier in the two-
    and four-slot builds (where granules measured slower or no faster); FEM_TUNE_PK_GRAN_SMALL adds those."""
    C, _ = _mods()
    if n == 20:
        A, b, w, _, _ = _cube20(gpu)
    else:
        A, b, mask = _cube(n, gpu)
        w = A.jacobi(mask)
    dflt, _, _ = _run(A, b, w, C.TUNE_DEFAULT, (2,))
    both, _, _ = _run(A, b, w, C.TUNE_DEFAULT | SMALL, (2,))
    assert dflt["gran"] is want and both["gran"] is True


@pytest.mark.parametrize("mode", ["pcg", "cg_masked"])
def test_flag_off_bit_identity(gpu, mode):
    """n = 20: 145 slices on one workgroup per CU, so most workgroups publish zeros. 40 fixed iterations, PCG mode and
    CG mode with masked (w = 0) rows: the granule path ran in one run and the counter barrier in the other, x and the
    poll tuple are equal."""
    C, _ = _mods()
    A, b, w, wm, ref = _cube20(gpu)
    wt, md = (w, C.MODE_PCG) if mode == "pcg" else (wm, C.MODE_CG_STABLE)
    on, p1, x1 = _run(A, b, wt, _on(), (40,), md)
    off, p0, x0 = _run(A, b, wt, _off(), (40,), md)
    assert on["gran"] is True and off["gran"] is False
    assert on["build"] == off["build"]
    assert _same(x1, x0) and p1 == p0
    assert rel(x1, ref["pcg" if mode == "pcg" else "cg"]) < 1e-12


@pytest.mark.parametrize("chunks", [(40,), (10, 10, 20), (1, 39), (1, 1, 1, 1, 1, 1, 34)], ids=str)
def test_launch_boundaries_and_epoch_parity(gpu, chunks):
    """The same 40 iterations cut into launches: every launch spends one more epoch on its chunk-end reduction, so the
    cuts put the first iteration of a launch (d alone, g from the state) and the chunk end (g alone) on both banks."""
    C, _ = _mods()
    A, b, w, _, _ = _cube20(gpu)
    _, p0, x0 = _cube20_off(gpu)
    on, p1, x1 = _run(A, b, w, _on(), chunks)
    assert on["gran"] is True
    assert _same(x1, x0) and p1 == p0


@pytest.mark.parametrize("n,wide", [(20, False), (40, False), (64, False), (80, False), (20, True), (64, True),
                                    (122, False)])
def test_every_build(gpu, n, wide):
    """Flag on against flag off over 24 iterations as 11 + 13 in every build: one slot (n = 20, 40), two (n = 64), four
    (n = 80), seven with one and with several slots occupied (FEM_TUNE_PK_WIDE), and the overflow build (n = 122)."""
    C, _ = _mods()
    if n == 20:
        A, b, w, _, _ = _cube20(gpu)
    else:
        A, b, mask = _cube(n, gpu)
        w = A.jacobi(mask)
    flags = _on(WIDE if wide else 0)
    on, p1, x1 = _run(A, b, w, flags, (11, 13))
    off, p0, x0 = _run(A, b, w, _off(WIDE if wide else 0), (11, 13))
    assert on["build"] == off["build"] == _expected_build(A.n, wide), (on, off)
    assert on["build"][1] == int(n == 122)
    assert on["gran"] is True and off["gran"] is False
    assert _same(x1, x0) and p1 == p0


def test_instrumented_build(gpu):
    """The phase-clock build: 24 iterations through fem_pcg_persist_profile with the flag on and off. The clocks tick
    (the SpMV phase and the reduction phase), and x equals bit for bit the plain seven-slot runs."""
    C, system = _mods()
    A, b, w, _, _ = _cube20(gpu)
    G = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8   # one workgroup per CU
    xs = {}
    for flags in (_on(), _off()):
        run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
        try:
            run.set_tuning(flags)
            run.start()
            assert run.effective_schedule() == 3 and run.persist_granules() == bool(flags & GRAN)
            buf = (ctypes.c_ulonglong * (G * (8 + 16)))()   # [G][8 phases] then [G][16 waves]
            g = ctypes.c_int()
            C.check(run.lib.fem_pcg_persist_profile(run.h, 24, buf, ctypes.byref(g)), "fem_pcg_persist_profile")
            poll = run.poll()
            xs[flags] = run.x.clone()
        finally:
            run.close()
        assert g.value == G and poll[0] == 24 and poll[1] == 0
        assert buf[1] != 0 and buf[3] != 0   # workgroup 0: the SpMV, the reduction
    _, _, x7 = _run(A, b, w, _on(WIDE), (24,))
    assert _same(xs[_on()], x7) and _same(xs[_off()], x7)


@pytest.mark.parametrize("wide", [False, True], ids=["two_slots", "seven_slots"])
def test_uneven_arrival(gpu, wide):
    """The strip matrix (slice widths 1 to 18 within every block of 64 slices, so the workgroups reach the reduction
    at different times), 12 iterations as 5 + 7."""
    C, _ = _mods()
    A, b, w = _strip(gpu)
    flags = _on(WIDE if wide else 0)
    on, p1, x1 = _run(A, b, w, flags, (5, 7))
    off, p0, x0 = _run(A, b, w, _off(WIDE if wide else 0), (5, 7))
    assert on["gran"] is True and off["gran"] is False and on["build"] == off["build"]
    assert bool(torch.isfinite(x1).all()) and float(x1.abs().max()) > 0.0
    assert _same(x1, x0) and p1 == p0


def test_full_solve_matches_flag_off(gpu):
    """n = 30 jittered, Jacobi-PCG to rtol 1e-8 (the stop falls inside a launch): the same iteration count, status and
    bits as flag off."""
    C, _ = _mods()
    A, _, mask = _cube(30, gpu)
    w = A.jacobi(mask)
    b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(5)).to(gpu)
    tol = 1e-8 * float(torch.sqrt(torch.dot(b, w * b)))
    r1 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=_on())
    r0 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=_off())
    assert r1.schedule == r0.schedule == 3
    assert r1.status == r0.status == C.PCG_CONVERGED
    assert r1.iterations == r0.iterations and r1.rz == r0.rz and _same(r1.x, r0.x)


def test_max_iter_inside_a_launch(gpu):
    """max_iter = 7 with launches of 64: the step stops the launch in its eighth iteration, after a reduction and
    before the update that would publish the next g."""
    C, _ = _mods()
    A, b, w, _, _ = _cube20(gpu)
    r1 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=7, chunk=64, schedule=3, tune=_on())
    r0 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=7, chunk=64, schedule=3, tune=_off())
    assert r1.schedule == r0.schedule == 3
    assert (r1.iterations, r1.status, r1.rz) == (r0.iterations, r0.status, r0.rz) == (7, C.PCG_MAXITER,
                                                                                              r0.rz)
    assert _same(r1.x, r0.x)


@pytest.mark.parametrize("first,second", [((12,), (12,)), ((1,), (1, 11)), ((2,), (1, 11))], ids=str)
def test_restart_on_one_context(gpu, first, second):
    """A solve, then start() again on the same context with another b and 12 more iterations: the epochs restart from
    zero over a granule block that still holds the first solve's tags unless start() zeroed it. A first solve of one
    iteration leaves d tagged 1 in bank 1 and g tagged 2 in bank 0, one of two iterations d tagged 2 in bank 0: the tags
    the restarted solve's first two reductions wait for, so a block left as it was would be taken for published and
    sum the first solve's partials. (After 12 iterations the stale tags are 11 to 13 and only the zeroing's presence,
    not its need, is exercised.) The result equals a fresh context's bit for bit."""
    C, system = _mods()
    A, b, w, _, _ = _cube20(gpu)
    b2 = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(9)).to(gpu)
    _, pf, xf = _run(A, b2, w, _on(), (12,))
    _, p0, x0 = _run(A, b2, w, _off(), (12,))
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.set_tuning(_on())
        run.start()
        assert run.persist_granules()
        for k in first:
            run.iterate(k)
        assert run.poll()[:2] == (sum(first), 0)
        run.b.copy_(b2)
        run.x.zero_()
        torch.cuda.synchronize()
        run.start()
        for k in second:
            run.iterate(k)
        p1 = run.poll()
        x1 = run.x.clone()
    finally:
        run.close()
    assert p1 == pf == p0 and _same(x1, xf) and _same(x1, x0)


def test_flag_changed_between_launches(gpu):
    """fem_pcg_set_tuning on a started context between launches: 5 iterations through granules, 5 through the counter
    barrier, 5 through granules again. The counters did not advance during the granule launches and the tags not
    during the counter one, so each change starts the epochs over; the 15 iterations equal the flag-off run's."""
    C, system = _mods()
    A, b, w, _, _ = _cube20(gpu)
    _, p0, x0 = _run(A, b, w, _off(), (15,))
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.set_tuning(_on())
        run.start()
        seen = []
        for flags in (_on(), _off(), _on()):
            run.set_tuning(flags)
            seen.append(run.persist_granules())
            run.iterate(5)
        p1 = run.poll()
        x1 = run.x.clone()
    finally:
        run.close()
    assert seen == [True, False, True]
    assert p1 == p0 and _same(x1, x0)


def test_flag_without_a_granule_build(gpu):
    """Only the builds the default flag set reaches have a granule form (records + sc1 gathers + diagonal-free stream,
    or the overflow build): with FEM_TUNE_PK_DESC off the flag changes nothing and the query says so."""
    C, _ = _mods()
    A, b, w, _, _ = _cube20(gpu)
    desc = 65536
    on, p1, x1 = _run(A, b, w, _on() & ~desc, (12,))
    off, p0, x0 = _run(A, b, w, _off() & ~desc, (12,))
    assert on["gran"] is False and off["gran"] is False
    assert _same(x1, x0) and p1 == p0
