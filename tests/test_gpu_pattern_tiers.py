"""GPU: the pattern build (csrc/pattern.hip) at the edges of its tiers. Every row, bucket and node segment is routed
to one of several kernels by a size threshold; each case here sits exactly on one side of one threshold, says which
side (with the deferral flags of k_graph_small, with what the incidence's bucket sort leaves in its workspace, and
with the host count that decides the route where the route itself cannot be seen), and compares every integer array of the build -- inc_ptr, inc, rowptr, colidx, diagpos,
slice_ptr, cols, dcols, csr2sell -- bit for bit with the host references of tests/pattern_ref.py and
`R.node_pattern`. The generic k_graph_small instantiation and the exported count / fill and SELL entry points that
build_graph itself does not call are run against the same references."""
import pytest
import torch

import pattern_ref as P
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
I32, I64, I16 = torch.int32, torch.int64, torch.int16

# constants of csrc/pattern.hip, under the names they have there
G_TCAP = 32            # k_graph_small keeps rows of at most this many neighbours
G_SCAP = 384           # candidate capacity of k_graph_small at 64 lanes per node
G_SMALL_LPN = 32       # its lanes per node: rows over G_SCAP * LPN / 64 candidates defer before hashing
G_UCAP = 512           # k_graph keeps rows of at most this many neighbours (longer: k_graph_big)
G_HT2 = 2048           # k_graph's hash table: 2 C slots up to this size
INB_G1 = 512           # workgroups of the incidence's level 1 (counts per bucket)
INB_MAXB = 16384       # buckets of the incidence's level 1
INB_CAP = 3584         # entries of a bucket sorted in LDS
INC_BIG = 4096         # node segments longer than this are sorted by k_inc_big
INB_MAXSH = 8          # at most 2^8 nodes per bucket (larger meshes: the radix form)
GB_WORDS = 32768       # bitmap words of the big-row kernels: a window of 32 * GB_WORDS ids
SCAP = G_SCAP * G_SMALL_LPN // 64
GB_WINDOW = 32 * GB_WORDS


def inb_shift(N):
    b = 7
    while (N + (1 << b) - 1) >> b > INB_MAXB:
        b += 1
    return b


def _mods():
    import fem355  # noqa: F401
    from fem355 import _capi as C, mesh, system
    return C, mesh, system


class Ref:
    """Host references of one connectivity (computed once per case)."""

    def __init__(self, t, N, graph=True):
        self.t, self.N = t, N
        self.inc_ptr, self.inc = P.incidence_ref(t, N)
        if graph:
            self.rowptr, self.colidx = R.node_pattern(t, N)
            self.diagpos = P.diagpos_ref(self.rowptr, self.colidx)
            self.slice_ptr, self.cols, self.c2s, self.dcols, self.far = P.sell_ref(self.rowptr, self.colidx, N)

    def seg(self, node):
        return int(self.inc_ptr[node + 1] - self.inc_ptr[node])

    def row(self, node):
        return int(self.rowptr[node + 1] - self.rowptr[node])


def _same(dev, want, what):
    assert dev.dtype in (I32, I64, I16), what
    got = dev.cpu().long()
    assert got.shape == want.shape and torch.equal(got, want), what


def _check_incidence(ip, inc, ref, what):
    _same(ip, ref.inc_ptr, (what, "inc_ptr"))
    _same(inc, ref.inc, (what, "inc"))


def _check_graph(g, ref, what):
    _check_incidence(g.inc_ptr, g.inc, ref, what)
    _same(g.rowptr, ref.rowptr, (what, "rowptr"))
    _same(g.colidx, ref.colidx, (what, "colidx"))
    _same(g.diagpos, ref.diagpos, (what, "diagpos"))
    _same(g.slice_ptr, ref.slice_ptr, (what, "slice_ptr"))
    _same(g.cols, ref.cols, (what, "cols"))
    assert (g.dcols is not None) == (not ref.far), (what, "far")
    if g.dcols is not None:
        _same(g.dcols[: ref.cols.numel()], ref.dcols, (what, "dcols"))
    _same(g.csr2sell[: ref.colidx.numel()], ref.c2s, (what, "csr2sell"))


def _incidence_capi(C, el, N):
    lib, st = C.lib(), C.stream(el.device)
    M, npe = el.shape
    inc_ptr = torch.empty(N + 1, dtype=I32, device=el.device)
    inc = torch.empty(M * npe, dtype=I32, device=el.device)
    C.check(lib.fem_incidence(C.ptr(el), M, npe, N, C.ptr(inc_ptr), C.ptr(inc), None, st), "fem_incidence")
    return inc_ptr, inc


def _incidence_route(C, el, N):
    """fem_incidence on a workspace of the test's own, filled with -7 (no slot is negative) -> (inc_ptr, inc, the
    bucket sort's global scratch, its hub flag). The workspace of the bucket form is three int32 arrays of M npe
    entries, each padded to 256 bytes -- (node, slot) pairs in the first two, the scratch in which k_inc_l2 lines up
    the buckets too large for LDS in the third -- then the (bucket, workgroup) counts, with the flag that k_inc_l2
    raises for k_inc_big behind them. A bucket sorted in LDS leaves its stretch of the scratch untouched."""
    lib = C.lib()
    M, npe = el.shape
    total = M * npe
    inc_ptr = torch.empty(N + 1, dtype=I32, device=el.device)
    inc = torch.empty(total, dtype=I32, device=el.device)
    nbytes = int(lib.fem_incidence_work_bytes(total, N))
    work = torch.full(((nbytes + 3) // 4,), -7, dtype=I32, device=el.device)
    C.check(lib.fem_incidence(C.ptr(el), M, npe, N, C.ptr(inc_ptr), C.ptr(inc), C.ptr(work), C.stream(el.device)),
            "fem_incidence")
    a4 = ((4 * total + 255) & ~255) // 4
    bsh = inb_shift(N)
    ncnt = ((N + (1 << bsh) - 1) >> bsh) * INB_G1
    assert 3 * a4 + ncnt < work.numel()
    return inc_ptr, inc, work[2 * a4: 2 * a4 + total].cpu(), int(work[3 * a4 + ncnt])


def _scan_i32(C, row_len, N):
    lib, dev = C.lib(), row_len.device
    rowptr = torch.empty(N + 1, dtype=I32, device=dev)
    work = torch.empty(int(lib.fem_scan_work_len(N)) + 1, dtype=I32, device=dev)
    C.check(lib.fem_scan_i32(C.ptr(row_len), N, C.ptr(rowptr), C.ptr(work), C.stream(dev)), "fem_scan_i32")
    return rowptr


def _small_tier(C, el, N, inc_ptr, inc):
    """fem_graph_count2 with a tmp of the test's own -> (row_len, tmp, deferral byte per node, deferred-row count):
    tmp is N rows of G_TCAP slots, then one byte per node (1: k_graph_small left the row to k_graph), padded to
    whole ints, then the number of deferred rows."""
    lib, dev = C.lib(), el.device
    assert int(lib.fem_graph_tmp_len(N)) == N * G_TCAP + (N + 3) // 4 + 1
    row_len = torch.empty(N, dtype=I32, device=dev)
    tmp = torch.full((N * G_TCAP + (N + 3) // 4 + 1,), -7, dtype=I32, device=dev)
    C.check(lib.fem_graph_count2(C.ptr(el), el.shape[1], C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(row_len), C.ptr(tmp),
                                 None, C.stream(dev)), "fem_graph_count2")
    flags = tmp[N * G_TCAP: N * G_TCAP + (N + 3) // 4].view(torch.uint8)[:N].cpu()
    return row_len, tmp, flags, int(tmp[N * G_TCAP + (N + 3) // 4])


def _count_fill_pair(C, el, N, inc_ptr, inc):
    """fem_graph_count + fem_scan_i32 + fem_graph_fill: k_graph for every row (no small tier, no deferral flags),
    k_graph_big for the rows it flags -> (rowptr, colidx, diagpos, far)."""
    lib, dev, st = C.lib(), el.device, C.stream(el.device)
    row_len = torch.empty(N, dtype=I32, device=dev)
    ovf = torch.full((1,), 5, dtype=I32, device=dev)
    C.check(lib.fem_graph_count(C.ptr(el), el.shape[1], C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(row_len), C.ptr(ovf),
                                st), "fem_graph_count")
    rowptr = _scan_i32(C, row_len, N)
    colidx = torch.empty(int(rowptr[N]), dtype=I32, device=dev)
    diagpos = torch.empty(N, dtype=I32, device=dev)
    C.check(lib.fem_graph_fill(C.ptr(el), el.shape[1], C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(rowptr), C.ptr(colidx),
                               C.ptr(diagpos), st), "fem_graph_fill")
    return rowptr, colidx, diagpos, int(ovf)


def _sell_chain(C, rowptr, colidx, N):
    """fem_sell_widths + fem_scan_i64 + fem_sell_fill + fem_sell_delta16 + fem_sell_csr2sell of a device CSR ->
    (slice_ptr, cols, csr2sell of fem_sell_fill, dcols, far, csr2sell of fem_sell_csr2sell)."""
    lib, dev, st = C.lib(), rowptr.device, C.stream(rowptr.device)
    ns = (N + 63) // 64
    width = torch.empty(ns, dtype=I64, device=dev)
    C.check(lib.fem_sell_widths(C.ptr(rowptr), N, C.ptr(width), st), "fem_sell_widths")
    slice_ptr = torch.empty(ns + 1, dtype=I64, device=dev)
    work = torch.empty(int(lib.fem_scan_work_len(ns)) + 1, dtype=I64, device=dev)
    C.check(lib.fem_scan_i64(C.ptr(width), ns, C.ptr(slice_ptr), C.ptr(work), st), "fem_scan_i64")
    ent, nnz = int(slice_ptr[ns]), int(colidx.numel())
    cols = torch.full((max(ent, 1),), -7, dtype=I32, device=dev)
    c2s = torch.full((max(nnz, 1),), -7, dtype=I64, device=dev)
    C.check(lib.fem_sell_fill(C.ptr(rowptr), C.ptr(colidx), N, C.ptr(slice_ptr), C.ptr(cols), C.ptr(c2s), st),
            "fem_sell_fill")
    dcols = torch.full((max(ent, 1),), -7, dtype=I16, device=dev)
    ovf = torch.zeros(1, dtype=I32, device=dev)
    C.check(lib.fem_sell_delta16(C.ptr(cols), N, C.ptr(slice_ptr), C.ptr(dcols), C.ptr(ovf), st), "fem_sell_delta16")
    c2s2 = torch.full((max(nnz, 1),), -7, dtype=I64, device=dev)
    C.check(lib.fem_sell_csr2sell(C.ptr(rowptr), N, C.ptr(slice_ptr), C.ptr(c2s2), st), "fem_sell_csr2sell")
    return slice_ptr, cols[:ent], c2s[:nnz], dcols[:ent], int(ovf), c2s2[:nnz]


def _check_sell_chain(C, rowptr, colidx, ref, what):
    sp, cols, c2s, dcols, far, c2s2 = _sell_chain(C, rowptr, colidx, ref.N)
    _same(sp, ref.slice_ptr, (what, "slice_ptr"))
    _same(cols, ref.cols, (what, "cols"))
    _same(c2s, ref.c2s, (what, "csr2sell of fem_sell_fill"))
    _same(c2s2, ref.c2s, (what, "csr2sell of fem_sell_csr2sell"))
    _same(dcols, ref.dcols, (what, "dcols"))
    assert bool(far) == ref.far, (what, "far")


# ---------------------------------------------------------------- graph tiers
def _fan600(top):
    t = P.fan(600)
    return torch.where(t == 602, torch.full_like(t, top), t), top + 1


# name -> (connectivity and node count, the hub's claimed count: C candidates / U neighbours / W id range of its
# candidates, and whether k_graph_small defers it)
GRAPH_CASES = {
    "row_at_tcap": (lambda: (P.fan(29), 32), dict(U=G_TCAP, deferred=False)),
    "row_over_tcap": (lambda: (P.fan(30), 33), dict(U=G_TCAP + 1, deferred=True)),
    "cand_at_scap": (lambda: (P.tiled(P.fan(8), 6), 11), dict(C=SCAP, U=11, deferred=False)),
    "cand_over_scap": (lambda: (torch.cat([P.tiled(P.fan(8), 6), P.fan(8)[:1]]), 11),
                       dict(C=SCAP + 4, U=11, deferred=True)),
    "table_at_64": (lambda: (P.fan(16), 19), dict(C=64, deferred=False)),
    "table_over_64": (lambda: (P.fan(17), 20), dict(C=68, deferred=False)),
    "table_at_ht2": (lambda: (P.fan(256), 259), dict(C=G_HT2 // 2, deferred=True)),
    "table_over_ht2": (lambda: (P.fan(257), 260), dict(C=G_HT2 // 2 + 4, deferred=True)),
    "row_at_ucap": (lambda: (P.fan(509), 512), dict(U=G_UCAP, deferred=True)),
    "row_over_ucap": (lambda: (P.fan(510), 513), dict(U=G_UCAP + 1, deferred=True)),
    "one_window": (lambda: _fan600(GB_WINDOW - 1), dict(U=603, W=GB_WINDOW, deferred=True)),
    "two_windows": (lambda: _fan600(GB_WINDOW), dict(U=603, W=GB_WINDOW + 1, deferred=True)),
}


@pytest.mark.parametrize("rev", [False, True], ids=["hub_first", "hub_last"])
@pytest.mark.parametrize("case", list(GRAPH_CASES))
def test_graph_tier_edges(gpu, case, rev):
    """One hub row on one side of one threshold of the node-graph kernels, the other rows far inside the small tier;
    with the hub as the first node and, ids reversed, as the last (another lane owns the row's own node)."""
    C, _, system = _mods()
    make, claim = GRAPH_CASES[case]
    t, N = make()
    hub = 0
    if rev:
        t, hub = P.reversed_ids(t, N), N - 1
    ref = Ref(t, N)
    # which side of which threshold: the hub's host counts, against the constants mirrored above
    cand, nbr = ref.seg(hub) * t.shape[1], ref.row(hub)
    if "C" in claim:
        assert cand == claim["C"]
    if "U" in claim:
        assert nbr == claim["U"]
    assert (cand > SCAP or nbr > G_TCAP) == claim["deferred"]
    if "W" in claim:   # k_graph_big's bitmap windows cover [lowest, highest] candidate id of the row
        ids = t[(t == hub).any(1)]
        assert nbr > G_UCAP and int(ids.max() - ids.min()) + 1 == claim["W"]
    others = torch.ones(N, dtype=torch.bool)
    others[hub] = False
    rl = ref.rowptr[1:] - ref.rowptr[:-1]
    assert int(rl[others].max()) <= 7 and int((ref.inc_ptr[1:] - ref.inc_ptr[:-1])[others].max()) * 4 <= SCAP

    el = t.to(gpu).contiguous()
    inc_ptr, inc = _incidence_capi(C, el, N)
    _check_incidence(inc_ptr, inc, ref, case)
    row_len, _, flags, ndefer = _small_tier(C, el, N, inc_ptr, inc)
    assert int(flags[hub]) == int(claim["deferred"]), "the hub row is on the other side of the small tier"
    assert int(flags.sum()) == ndefer == int(claim["deferred"])
    _same(row_len, rl, (case, "row_len"))

    _check_graph(system.build_graph(el, N), ref, case)
    rowptr, colidx, diagpos, far = _count_fill_pair(C, el, N, inc_ptr, inc)     # k_graph for every row
    _same(rowptr, ref.rowptr, (case, "fem_graph_count"))
    _same(colidx, ref.colidx, (case, "fem_graph_fill colidx"))
    _same(diagpos, ref.diagpos, (case, "fem_graph_fill diagpos"))
    assert bool(far) == ref.far


# ---------------------------------------------------------------- incidence tiers
def _slot_window_mesh(mesh):
    """~263,000 rows whose first 2,050 and last 2,050 are the tets of a 4,100-tet fan: the hub's 4,100 slots span
    more than 2^20, so k_inc_big's slot bitmap takes two windows. Between them kuhn_cube(35) on nodes of its own,
    followed by its first 1,700 tets once more (the cube alone leaves the span 3,179 slots short of 2^20)."""
    f = P.fan(4100)
    cube = mesh.kuhn_cube(35)[1] + 4103
    return torch.cat([f[:2050], cube, cube[:1700], f[2050:]]), 4103 + 36 ** 3


INC_CASES = ["bucket_at_cap", "bucket_over_cap", "segment_at_big", "segment_over_big", "slot_windows"]


@pytest.mark.parametrize("case", INC_CASES)
def test_incidence_tier_edges(gpu, case):
    """Bucket 0 at / over the LDS capacity of k_inc_l2, the hub's segment at / over the length k_inc_big takes, and a
    hub segment whose slots cross a bitmap window. The host counts that decide the route are asserted against the
    mirrored constants, and the route taken is read from the workspace: bucket 0's stretch of the global scratch is
    written iff the bucket did not fit in LDS, and the hub flag is raised iff a segment was left to k_inc_big."""
    C, mesh, system = _mods()
    if case == "slot_windows":
        t, N = _slot_window_mesh(mesh)
    else:
        m = {"bucket_at_cap": 3206, "bucket_over_cap": 3207, "segment_at_big": 4096, "segment_over_big": 4097}[case]
        t, N = P.fan(m), m + 3
    ref = Ref(t, N)
    bsh = inb_shift(N)
    assert bsh == 7 and bsh <= INB_MAXSH
    bucket0 = int((t.reshape(-1) >> bsh == 0).sum())     # bucket of the hub
    if case == "bucket_at_cap":
        assert bucket0 == INB_CAP and ref.seg(0) <= INC_BIG
    elif case == "bucket_over_cap":
        assert bucket0 == INB_CAP + 1 and ref.seg(0) <= INC_BIG
    elif case == "segment_at_big":
        assert bucket0 > INB_CAP and ref.seg(0) == INC_BIG
    elif case == "segment_over_big":
        assert bucket0 > INB_CAP and ref.seg(0) == INC_BIG + 1
    else:
        slots = ref.inc[ref.inc_ptr[0]:ref.inc_ptr[1]]
        assert bucket0 > INB_CAP and ref.seg(0) == 4100 > INC_BIG
        assert int(slots[-1] - slots[0]) + 1 > GB_WINDOW and t.shape[0] < 264_000
    el = t.to(gpu).contiguous()
    ip, inc, scratch, hub_flag = _incidence_route(C, el, N)
    _check_incidence(ip, inc, ref, case)
    if bucket0 <= INB_CAP:
        assert bool((scratch[:bucket0] == -7).all()), "bucket 0 went through the global scratch"
    else:
        assert bool((scratch[:bucket0] >= 0).all()), "bucket 0 did not go through the global scratch"
    assert hub_flag == int(ref.seg(0) > INC_BIG), "the hub segment is on the other side of k_inc_big"
    _check_incidence(*system.incidence(el, N), ref, case)
    _check_graph(system.build_graph(el, N), ref, case)


@pytest.mark.parametrize("N", [3_000_000, 4_194_304, 4_194_305])
def test_incidence_size_ranges(gpu, N):
    """Buckets of 256 nodes (2,097,152 < N <= 4,194,304: byte-wide bucket-relative node ids up to 255, four counts per
    lane in the bucket's scan) and, past that, the radix form chosen by size alone. A few thousand elements: a small
    cube spread over the id range and a 300-tet fan on the last 303 nodes."""
    C, mesh, system = _mods()
    cube = mesh.kuhn_cube(8)[1]
    t = torch.cat([P.spread(cube, (N - 304) // 728), P.fan(300) + (N - 303)])
    assert int(t.max()) == N - 1 and int(cube.max()) == 728
    bsh = inb_shift(N)
    if N == 3_000_000:
        assert bsh == INB_MAXSH and bool(((t.reshape(-1) & ((1 << bsh) - 1)) >= 128).any())
    elif N == 4_194_304:
        assert bsh == INB_MAXSH and (N + (1 << bsh) - 1) >> bsh == INB_MAXB
    else:
        assert bsh > INB_MAXSH
    graph = N == 3_000_000
    ref = Ref(t, N, graph=graph)
    el = t.to(gpu).contiguous()
    _check_incidence(*system.incidence(el, N), ref, N)
    if graph:
        _check_graph(system.build_graph(el, N), ref, N)


# ---------------------------------------------------------------- the generic k_graph_small instantiation
def test_generic_small_kernel_unaligned_connectivity(gpu):
    """A contiguous connectivity at an odd int64 offset of a buffer (8-byte but not 16-byte aligned): the 16-byte row
    loads of the npe-specific instantiations do not apply, the generic one builds the same pattern."""
    C, mesh, system = _mods()
    c, t = mesh.hex_box(3)
    N = c.shape[0]
    ref = Ref(t, N)
    assert torch.equal(ref.rowptr, R.node_pattern(t, N)[0])
    aligned = t.to(gpu).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=I64, device=gpu)
    view = buf[1:].view(t.shape)
    view.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    ga, gv = system.build_graph(aligned, N), system.build_graph(view, N)
    _check_graph(ga, ref, "aligned")
    _check_graph(gv, ref, "offset 1")
    for name in ("inc_ptr", "inc", "rowptr", "colidx", "diagpos", "slice_ptr", "cols", "dcols", "csr2sell"):
        assert torch.equal(getattr(ga, name), getattr(gv, name)), name


@pytest.mark.parametrize("cols", [[0, 1, 2], [7, 2, 4], [0, 1, 2, 3, 4], [6, 0, 3, 5, 1]])
def test_generic_small_kernel_other_npe(gpu, cols):
    """npe = 3 and 5 (column subsets of the hex connectivity): no npe-specific instantiation exists."""
    C, mesh, system = _mods()
    c, t = mesh.hex_box(3)
    t = t[:, cols].contiguous()
    N = c.shape[0] + 2
    _check_graph(system.build_graph(t.to(gpu), N), Ref(t, N), cols)


def test_generic_small_kernel_by_environment(gpu, monkeypatch):
    """FEM355_GRAPH_SLOTS sends npe = 4 through the generic instantiation: the same arrays as without it."""
    C, mesh, system = _mods()
    c, t = mesh.kuhn_cube(5)
    N = c.shape[0]
    el = t.to(gpu)
    monkeypatch.delenv("FEM355_GRAPH_SLOTS", raising=False)
    g0 = system.build_graph(el, N)
    monkeypatch.setenv("FEM355_GRAPH_SLOTS", "1")
    g1 = system.build_graph(el, N)
    monkeypatch.delenv("FEM355_GRAPH_SLOTS", raising=False)
    ref = Ref(t, N)
    _check_graph(g0, ref, "default")
    _check_graph(g1, ref, "FEM355_GRAPH_SLOTS")
    for name in ("rowptr", "colidx", "diagpos", "slice_ptr", "cols", "dcols", "csr2sell"):
        assert torch.equal(getattr(g0, name), getattr(g1, name)), name


# ---------------------------------------------------------------- entry points build_graph does not call
def _entry_mesh(mesh, name):
    if name == "tet10_x9":
        c, t = mesh.tet10_cube(3)
        return P.tiled(t, 9), c.shape[0]
    if name == "fan700":
        return torch.cat([P.fan(700), torch.tensor([[5, 9, 400, 702]])]), 703
    c, t = mesh.kuhn_cube(5)
    return t, c.shape[0] + 9


@pytest.mark.parametrize("name", ["tet10_x9", "fan700", "cube_unused_nodes"])
def test_separate_entry_points_equal_build_graph(gpu, name):
    """fem_graph_count + fem_scan_i32 + fem_graph_fill (k_graph for every row), and fem_graph_count2 +
    fem_graph_fill2 + fem_sell_widths + fem_scan_i64 + fem_sell_fill + fem_sell_delta16 + fem_sell_csr2sell (what
    csr_abi.hip and foreign callers use), on rows of every tier: the arrays of build_graph and of the references."""
    C, mesh, system = _mods()
    lib = C.lib()
    t, N = _entry_mesh(mesh, name)
    ref = Ref(t, N)
    el = t.to(gpu).contiguous()
    g = system.build_graph(el, N)
    _check_graph(g, ref, name)
    inc_ptr, inc = _incidence_capi(C, el, N)
    rowptr, colidx, diagpos, far = _count_fill_pair(C, el, N, inc_ptr, inc)
    assert torch.equal(rowptr, g.rowptr) and torch.equal(colidx, g.colidx) and torch.equal(diagpos, g.diagpos)
    _same(rowptr, ref.rowptr, (name, "fem_graph_count"))
    _same(colidx, ref.colidx, (name, "fem_graph_fill colidx"))
    _same(diagpos, ref.diagpos, (name, "fem_graph_fill diagpos"))
    assert bool(far) == ref.far
    row_len, tmp, _, _ = _small_tier(C, el, N, inc_ptr, inc)
    rowptr2 = _scan_i32(C, row_len, N)
    colidx2 = torch.full((int(rowptr2[N]),), -7, dtype=I32, device=gpu)
    diagpos2 = torch.full((N,), -7, dtype=I32, device=gpu)
    C.check(lib.fem_graph_fill2(C.ptr(el), el.shape[1], C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(rowptr2), C.ptr(tmp),
                                C.ptr(colidx2), C.ptr(diagpos2), C.stream(gpu)), "fem_graph_fill2")
    assert torch.equal(rowptr2, g.rowptr) and torch.equal(colidx2, g.colidx) and torch.equal(diagpos2, g.diagpos)
    _check_sell_chain(C, rowptr2, colidx2, ref, name)
    sp, cols, c2s, dcols, _, _ = _sell_chain(C, rowptr2, colidx2, N)
    assert torch.equal(sp, g.slice_ptr) and torch.equal(cols, g.cols) and torch.equal(c2s, g.csr2sell[: c2s.numel()])
    assert g.dcols is not None and torch.equal(dcols, g.dcols[: dcols.numel()])


@pytest.mark.parametrize("N", [63, 64, 65, 1])
def test_sell_chain_ragged_last_slice(gpu, N):
    """The separate SELL chain where the last slice is ragged (padding N - 1 in the lanes past the last row), exactly
    full, or a single row of an empty second slice: kuhn_cube(3) (64 nodes) cut to the elements of its first N nodes;
    N = 1: one node under a collapsed element."""
    C, mesh, system = _mods()
    lib = C.lib()
    if N == 1:
        t = torch.zeros(1, 4, dtype=I64)
    else:
        t = mesh.kuhn_cube(3)[1]
        t = t[(t < N).all(1)].contiguous()
    ref = Ref(t, N)
    el = t.to(gpu).contiguous()
    inc_ptr, inc = _incidence_capi(C, el, N)
    row_len, tmp, _, _ = _small_tier(C, el, N, inc_ptr, inc)
    rowptr = _scan_i32(C, row_len, N)
    colidx = torch.full((int(rowptr[N]),), -7, dtype=I32, device=gpu)
    diagpos = torch.full((N,), -7, dtype=I32, device=gpu)
    C.check(lib.fem_graph_fill2(C.ptr(el), 4, C.ptr(inc_ptr), C.ptr(inc), N, C.ptr(rowptr), C.ptr(tmp), C.ptr(colidx),
                                C.ptr(diagpos), C.stream(gpu)), "fem_graph_fill2")
    _same(rowptr, ref.rowptr, (N, "rowptr"))
    _same(colidx, ref.colidx, (N, "colidx"))
    _same(diagpos, ref.diagpos, (N, "diagpos"))
    _check_sell_chain(C, rowptr, colidx, ref, N)
    last = ref.cols[int(ref.slice_ptr[-2]):].view(-1, 64)
    if N == 65:      # the unused node 64 is alone in a slice of width 0
        assert last.numel() == 0 and ref.row(64) == 0
    elif N % 64:     # the lanes past the last row hold N - 1
        assert last.numel() and bool((last[:, N % 64:] == N - 1).all())
    _check_graph(system.build_graph(el, N), ref, N)
