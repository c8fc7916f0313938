"""GPU tier: the persistent PCG's per-slice descriptor records (FEM_TUNE_PK_DESC, csrc/sell_pair.hpp PkDesc and
sell_row_pair_rec, csrc/pcg_persist.hpp DESC builds). A slot's value base, width, diagonal position and delta list
come from one record read by scalar loads, one slot ahead; the row sum adds the same products in the same order, so
every iterate must equal the flag-off build's bit for bit. Every mesh is jittered (on the regular cube every interior
slice has the same list and diagonal position, so a record taken from the wrong slice would pass). References that
run none of the new code: the flag-off build (bit identity), the three-kernel schedule (1e-12 relative: its
reductions sum in another order), and a host computation of the records from the shared solver layout."""
import ctypes
import functools

import pytest
import torch

from conftest import rel

pytestmark = pytest.mark.gpu
F64 = torch.float64
DESC = 65536      # FEM_TUNE_PK_DESC
WIDE = 256        # FEM_TUNE_PK_WIDE
CAP = 16          # streamed list entries a record holds (csrc/sell_pair.hpp PKD_CAP)
KIND_OD, KIND_FULL, KIND_LANE = 0, 1, 2


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
    _, fixed = mesh.cube_poisson_case(c)
    A = system.assemble_tet4_system(c.to(gpu), t.to(gpu), "poisson")
    mask = torch.zeros(A.n, dtype=torch.uint8, device=gpu)
    mask[fixed.to(gpu)] = 1
    b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(3)).to(gpu)
    return A, b, mask


@functools.lru_cache(maxsize=1)
def _cube20(gpu):
    """The n = 20 cube (9,261 rows, 145 slices) shared by the cases that use it, with its three-kernel references."""
    C, _, _, _ = _mods()
    A, b, mask = _cube(20, gpu)
    w = A.jacobi(mask)
    wm = (mask == 0).to(F64)
    ref = {"pcg": A.pcg(b, w=w, mode=C.MODE_PCG, tol=0.0, max_iter=40, schedule=0).x,
           "cg": A.pcg(b, w=wm, mode=C.MODE_CG_STABLE, tol=0.0, max_iter=40, schedule=0).x}
    return A, b, w, wm, ref


@functools.lru_cache(maxsize=1)
def _tet10_mass(gpu):
    """Scalar mass of a small jittered tet10 cube: odd and even slice widths, rows too irregular for a slice-uniform
    list (every slice keeps per-lane deltas, so none runs from a record)."""
    _, element, mesh, system = _mods()
    c, e = mesh.tet10_cube(5, jitter=0.1)
    c, e = c.to(gpu), e.to(gpu)
    Me = element.compute_M_matrix(c, e, "c3d10", 7850.0, device=gpu, dtype=F64, scalar=True)
    A = system.SellMatrix(system.build_graph(e, c.shape[0]), 1).add_element_matrices(Me, e)
    b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(4)).to(gpu)
    return A, b, A.jacobi(None)


def _strip_lists():
    """Neighbour positions of the 64 slice positions of one block of _strip: cliques of positions, with or without
    their self loops (the diagonal), chosen so that the slices' delta lists cover what the cubes never give."""
    nb = [set() for _ in range(64)]

    def clique(ps, loops=True):
        for i in ps:
            for j in ps:
                if i != j or loops:
                    nb[i].add(j)

    def edge(i, j):
        nb[i].add(j)
        nb[j].add(i)

    clique(range(0, 4))            # streamed width 3 with the diagonal at list index 0, 1, 2 (= w1 - 1), 3 (= w1)
    clique(range(5, 8))            # position 4 has no diagonal: a list without 0, width 3
    for j in (5, 6, 7):
        edge(4, j)
    clique([9])                    # 8: a list of one entry without 0; 9: streamed width 1, the diagonal after it
    edge(8, 9)
    clique(range(12, 15))          # 10, 11: lists without 0 of even width 4
    edge(10, 11)
    for i in (10, 11):
        for j in (12, 13, 14):
            edge(i, j)
    clique(range(15, 32))          # 17 entries: streamed width 16, exactly a record's capacity
    clique(range(32, 50))          # 18 entries: streamed width 17, past it
    clique(range(50, 64))          # 14 entries: streamed width 13, several rounds and the odd tail
    return [sorted(x) for x in nb]


def _strip_arrays(blocks, dev):
    """SELL arrays of the strip matrix: row (slice k, lane l) holds the columns (k', l) of the slices k' its position's
    list names inside its block of 64 slices. Every lane of a slice has the same deltas (multiples of 64), so every
    slice is slice-uniform; the values differ per row (the jitter). Symmetric; diagonally dominant where a diagonal
    exists. -> (n, slice_ptr, cols, dcols, vals, widest)"""
    nb = _strip_lists()
    K = 64 * blocks
    width = torch.tensor([len(x) for x in nb], dtype=torch.int64).repeat(blocks)
    sp = torch.zeros(K + 1, dtype=torch.int64)
    sp[1:] = torch.cumsum(64 * width, 0)
    ent = int(sp[-1])
    cols = torch.empty(ent, dtype=torch.int64)
    lanes = torch.arange(64)
    for pos in range(64):
        ks = torch.arange(pos, K, 64)
        for j, q in enumerate(nb[pos]):
            idx = (sp[ks] + 64 * j)[:, None] + lanes
            cols[idx] = ((ks - pos + q) * 64)[:, None] + lanes
    sl = torch.repeat_interleave(torch.arange(K), 64 * width)
    row = sl * 64 + (torch.arange(ent) - sp[sl]) % 64
    lo, hi = torch.minimum(row, cols).to(F64), torch.maximum(row, cols).to(F64)
    vals = torch.where(row == cols, 20.0 + torch.sin(lo), 0.5 * torch.sin(0.37 * lo + 1.91 * hi + 0.1))
    return (64 * K, sp.to(dev), cols.to(torch.int32).to(dev), (cols - row).to(torch.int16).to(dev), vals.to(dev),
            max(len(x) for x in nb))


@functools.lru_cache(maxsize=1)
def _strip(gpu):
    """A synthetic matrix of 8,192 slices (two per wave on 256 workgroups) whose slice-uniform lists have odd and even
    streamed widths, the diagonal at every list position including the last two, lists without a 0, and lists at and
    past a record's capacity. Its pattern is given directly (no mesh produces a row without its diagonal)."""
    _, _, _, system = _mods()
    n, sp, cols, dcols, vals, widest = _strip_arrays(128, gpu)
    e = torch.empty(0, dtype=torch.int32, device=gpu)
    g = system.Graph(n, 0, e, e, e, e, e, sp, cols)
    g.dcols = dcols
    g.max_width = widest
    A = system.SellMatrix(g, 1)
    A.vals.copy_(vals)
    b = torch.randn(n, dtype=F64, generator=torch.Generator().manual_seed(6)).to(gpu)
    w = (1.0 / (20.0 + torch.sin(torch.arange(n, dtype=F64)))).to(gpu)
    return A, b, w


def _run(A, b, w, flags, chunks, mode=1):
    """Fixed iterations on schedule 3 with the given flag set -> (facts, poll, x)."""
    _, _, _, system = _mods()
    run = system.PcgRunner(A, b, w, mode=mode, tol=0.0, schedule=3)
    try:
        run.set_tuning(flags)
        run.start()
        assert run.effective_schedule() == 3
        facts = {"desc": run.desc_slices(), "od": run.offdiag_slices(), "uni": run.uniform_slices(),
                 "build": run.persist_build()}
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


def _host_records(A):
    """The records a started context must hold, from the shared solver layout alone: per slice (p0, streamed width, kd,
    kind, tail delta, streamed deltas zero-padded to CAP)."""
    sl = A.g.solver_layout()
    sp = A.g.slice_ptr.cpu().tolist()
    uoff = sl.uoff.cpu().tolist()
    ucol = sl.ucol.cpu().tolist()
    out = []
    for s in range(len(sp) - 1):
        p0, w = sp[s], (sp[s + 1] - sp[s]) // 64
        uo = uoff[s]
        if uo < 0:
            out.append((p0, w, -1, KIND_LANE, 0, [0] * CAP))
            continue
        full = ucol[uo:uo + w]
        kd = full.index(0) if 0 in full else -1
        st = [d for d in full if d != 0] if kd >= 0 else full
        if len(st) > CAP:
            out.append((p0, len(st), -1, KIND_LANE, 0, [0] * CAP))
            continue
        tail = st[-1] if len(st) % 2 else 0
        out.append((p0, len(st), kd, KIND_OD if kd >= 0 else KIND_FULL, tail, st + [0] * (CAP - len(st))))
    return out


def _decode(rec):
    """debug_desc_records() -> the same tuples (word layout: csrc/sell_pair.hpp PkDesc)."""
    out = []
    for r in rec.tolist():
        u = [x & 0xffffffff for x in r]
        p0 = u[0] | (u[1] << 32)
        kd = u[3] & 0xff
        kd = kd - 256 if kd >= 128 else kd
        s16 = lambda v: v - 65536 if v >= 32768 else v   # noqa: E731
        dl = []
        for wd in u[4:4 + CAP // 2]:
            dl += [s16(wd & 0xffff), s16(wd >> 16)]
        out.append((p0, u[2], kd, (u[3] >> 8) & 0xff, s16(u[3] >> 16), dl))
    return out


def _n_record_slices(A):
    return sum(1 for r in _host_records(A) if r[3] != KIND_LANE)


@pytest.mark.parametrize("mode", ["pcg", "cg_masked"])
def test_flag_off_bit_identity(gpu, mode):
    """n = 20: diagonal-free slices beside slices that keep their diagonal. 40 fixed iterations, PCG mode and CG mode
    with masked (w = 0) rows: x and the poll tuple equal the flag-off run's."""
    C, _, _, _ = _mods()
    A, b, w, wm, ref = _cube20(gpu)
    wt, md = (w, C.MODE_PCG) if mode == "pcg" else (wm, C.MODE_CG_STABLE)
    on, p1, x1 = _run(A, b, wt, C.TUNE_DEFAULT, (40,), md)
    off, p0, x0 = _run(A, b, wt, C.TUNE_DEFAULT & ~DESC, (40,), md)
    nrec = _n_record_slices(A)
    assert 0 < on["od"][0] <= nrec < 145, (on, nrec)   # records: the diagonal-free slices and uniform full-row ones
    assert on["desc"] == (nrec, 145) and nrec == on["uni"][0], on
    assert off["desc"] == (0, 145) and off["od"] == on["od"]
    assert torch.equal(x1, x0) and p1 == p0
    assert rel(x1, ref["pcg" if mode == "pcg" else "cg"]) < 1e-12


def test_chunked_launches_are_bit_identical(gpu):
    """The same 40 iterations as one launch, as 10 + 10 + 20 and as 1 + 39: the first slot's record is requested before
    the u-flag wait on both sweep parities, in the first iteration of a launch and in later ones."""
    C, _, _, _ = _mods()
    A, b, w, _, ref = _cube20(gpu)
    outs = [_run(A, b, w, C.TUNE_DEFAULT, ch) for ch in ((40,), (10, 10, 20), (1, 39))]
    assert outs[0][0]["desc"][0] > 0
    for _, p, x in outs[1:]:
        assert p == outs[0][1] and torch.equal(x, outs[0][2])
    assert rel(outs[0][2], ref["pcg"]) < 1e-12


@pytest.mark.parametrize("n,wide", [(20, False), (40, False), (64, False), (80, False), (20, True), (64, True)])
def test_every_build(gpu, n, wide):
    """Flag on against flag off over 24 iterations in every build that reads records: one slot (n = 20, 40), two slots
    (n = 64), the four-slot build (n = 80), the seven-slot build with one and with several slots occupied
    (FEM_TUNE_PK_WIDE)."""
    C, _, _, _ = _mods()
    if n == 20:
        A, b, w, _, _ = _cube20(gpu)
    else:
        A, b, mask = _cube(n, gpu)
        w = A.jacobi(mask)
    flags = C.TUNE_DEFAULT | (WIDE if wide else 0)
    on, p1, x1 = _run(A, b, w, flags, (24,))
    off, p0, x0 = _run(A, b, w, flags & ~DESC, (24,))
    assert on["build"] == off["build"] == _expected_build(A.n, wide), (on, off)
    assert on["desc"][0] > 0 and off["desc"][0] == 0, (on, off)
    assert torch.equal(x1, x0) and p1 == p0


def test_no_qualifying_slice(gpu):
    """A seeded random renumbering of the n = 20 cube has no slice-uniform slice: no slice runs from a record (every
    record says so), same bits."""
    C, _, _, _ = _mods()
    A, b, mask = _cube(20, gpu, permute=11)
    w = A.jacobi(mask)
    on, p1, x1 = _run(A, b, w, C.TUNE_DEFAULT, (30,))
    off, p0, x0 = _run(A, b, w, C.TUNE_DEFAULT & ~DESC, (30,))
    assert on["desc"] == (0, 145) and off["desc"] == (0, 145), on
    assert torch.equal(x1, x0) and p1 == p0


def test_tet10_mass_mixed_widths(gpu):
    """The scalar mass of tet10_cube(5, jitter = 0.1): odd and even slice widths, all with per-lane deltas, so every
    slot reads its record and then takes the kept path. 20 iterations, bit identity to flag off. (The record path's
    odd widths, lists without a 0 and lists past the capacity: test_strip_*.)"""
    C, _, _, _ = _mods()
    A, b, w = _tet10_mass(gpu)
    sp = A.g.slice_ptr.cpu()
    widths = ((sp[1:] - sp[:-1]) // 64).tolist()
    assert any(x % 2 for x in widths) and any(x % 2 == 0 for x in widths), widths
    on, p1, x1 = _run(A, b, w, C.TUNE_DEFAULT, (20,))
    off, p0, x0 = _run(A, b, w, C.TUNE_DEFAULT & ~DESC, (20,))
    assert on["desc"] == (_n_record_slices(A), len(widths)), on
    assert torch.equal(x1, x0) and p1 == p0


def _strip_records(gpu):
    _, _, _, system = _mods()
    A, b, w = _strip(gpu)
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.start()
        assert run.effective_schedule() == 3
        return run.debug_desc_records(), run.desc_slices()
    finally:
        run.close()


def test_strip_record_round_trip(gpu):
    """The strip matrix's records equal the host's, and hold what the cubes never give: both kinds of record slice,
    odd and even streamed widths, non-zero tail deltas of both signs, the diagonal at list index w1 - 1 and w1 of an
    odd width, a streamed width equal to the capacity, and a slice-uniform list past it (kept path)."""
    A, _, _ = _strip(gpu)
    rec, (nrec, ns) = _strip_records(gpu)
    got, want = _decode(rec), _host_records(A)
    assert len(got) == len(want) == ns == 8192
    for s, (g, h) in enumerate(zip(got, want)):
        assert g == h, (s, g, h)
    sl = A.g.solver_layout()
    assert bool((sl.uoff >= 0).all())   # every slice is slice-uniform: kind 2 here means "past the capacity"
    recs = [r for r in got if r[3] != KIND_LANE]
    assert nrec == len(recs)
    n = lambda f: sum(1 for r in recs if f(r))   # noqa: E731  (r = (p0, w1, kd, kind, tail, deltas))
    assert n(lambda r: r[3] == KIND_OD) > 0 and n(lambda r: r[3] == KIND_FULL) > 0
    assert n(lambda r: r[3] == KIND_FULL and r[1] % 2) > 0 and n(lambda r: r[3] == KIND_FULL and r[1] % 2 == 0) > 0
    assert n(lambda r: r[3] == KIND_OD and r[1] % 2) > 0 and n(lambda r: r[3] == KIND_OD and r[1] % 2 == 0) > 0
    assert n(lambda r: r[4] > 0) > 0 and n(lambda r: r[4] < 0) > 0
    assert n(lambda r: r[1] % 2 and r[1] > 1 and r[2] == r[1] - 1) > 0 and n(lambda r: r[1] % 2 and r[2] == r[1]) > 0
    assert n(lambda r: r[1] == 1) > 0                      # no pair at all: the tail alone
    assert n(lambda r: r[1] == CAP) > 0                    # all eight delta words
    assert sum(1 for r in got if r[3] == KIND_LANE and r[1] == CAP + 1) > 0


@pytest.mark.parametrize("wide", [False, True], ids=["two_slots", "seven_slots"])
def test_strip_bit_identity(gpu, wide):
    """12 iterations on the strip matrix as launches of 5 + 7 (both sweep directions, a launch boundary), in the
    two-slot build and the seven-slot one: x and the poll tuple equal the flag-off run's bit for bit."""
    C, _, _, _ = _mods()
    A, b, w = _strip(gpu)
    flags = C.TUNE_DEFAULT | (WIDE if wide else 0)
    on, p1, x1 = _run(A, b, w, flags, (5, 7))
    off, p0, x0 = _run(A, b, w, flags & ~DESC, (5, 7))
    assert on["build"] == off["build"] == _expected_build(A.n, wide), (on, off)
    assert on["desc"][0] > 0 and off["desc"][0] == 0, (on, off)
    assert bool(torch.isfinite(x1).all()) and float(x1.abs().max()) > 0.0
    assert torch.equal(x1.view(torch.int64), x0.view(torch.int64)) and p1 == p0


@pytest.mark.parametrize("case", ["kuhn20", "tet10_mass"])
def test_record_round_trip(gpu, case):
    """The debug read-back equals, field for field, the records formed on the host from slice_ptr and the shared
    solver layout's uoff and lists (the streamed list is the shared one without its 0, kd the 0's position)."""
    _, _, _, system = _mods()
    if case == "kuhn20":
        A, b, w, _, _ = _cube20(gpu)
    else:
        A, b, w = _tet10_mass(gpu)
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.start()
        assert run.effective_schedule() == 3
        rec = run.debug_desc_records()
    finally:
        run.close()
    got, want = _decode(rec), _host_records(A)
    assert len(got) == len(want)
    for s, (g, h) in enumerate(zip(got, want)):
        assert g == h, (s, g, h)
    if case == "kuhn20":
        kinds = {r[3] for r in want}
        assert {KIND_OD, KIND_LANE} <= kinds, kinds


def test_instrumented_build(gpu):
    """The phase-clock build that reads records: 24 iterations through fem_pcg_persist_profile. The clocks tick, and x
    equals bit for bit the plain seven-slot run (FEM_TUNE_PK_WIDE) and the flag-off one."""
    C, _, _, system = _mods()
    A, b, w, _, _ = _cube20(gpu)
    G = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8   # one workgroup per CU
    run = system.PcgRunner(A, b, w, tol=0.0, schedule=3)
    try:
        run.set_tuning(C.TUNE_DEFAULT)
        run.start()
        assert run.effective_schedule() == 3 and run.desc_slices()[0] > 0
        buf = (ctypes.c_ulonglong * (G * (8 + 16)))()   # [G][8 phases] then [G][16 waves]
        g = ctypes.c_int()
        C.check(run.lib.fem_pcg_persist_profile(run.h, 24, buf, ctypes.byref(g)), "fem_pcg_persist_profile")
        poll = run.poll()
        x = run.x.clone()
    finally:
        run.close()
    assert g.value == G and poll[0] == 24 and poll[1] == 0
    assert buf[1] != 0   # workgroup 0, phase 1: the SpMV
    _, _, x7 = _run(A, b, w, C.TUNE_DEFAULT | WIDE, (24,))
    _, _, x0 = _run(A, b, w, (C.TUNE_DEFAULT | WIDE) & ~DESC, (24,))
    assert torch.equal(x, x7) and torch.equal(x, x0)


def test_full_solve_matches_flag_off(gpu):
    """n = 30 jittered, Jacobi-PCG to rtol 1e-8: the same iteration count and the same bits as flag off."""
    C, _, mesh, _ = _mods()
    A, _, mask = _cube(30, gpu)
    w = A.jacobi(mask)
    b = torch.randn(A.n, dtype=F64, generator=torch.Generator().manual_seed(5)).to(gpu)
    tol = 1e-8 * float(torch.sqrt(torch.dot(b, w * b)))
    r1 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=C.TUNE_DEFAULT)
    r0 = A.pcg(b, w=w, mode=C.MODE_PCG, tol=tol, max_iter=5000, schedule=3, tune=C.TUNE_DEFAULT & ~DESC)
    assert r1.status == r0.status == C.PCG_CONVERGED
    assert r1.iterations == r0.iterations and torch.equal(r1.x, r0.x)
