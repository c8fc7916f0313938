"""Host references of the pattern build (csrc/pattern.hip) and of the dof-level CSR (csrc/csr_abi.hip), in plain
torch, with no code from the package: the node -> slot incidence, the SELL-64 layout of a CSR pattern and the
coalesced dof CSR with its diagonal positions, plus the small meshes whose rows, buckets and segments sit at the size
thresholds of the kernels (fans around one hub node, repeated and spread connectivities).

Every result here is the unique right answer of an integer computation, so the GPU tests compare bit for bit."""
import torch

from oracle import ref_cpu as R

F64, I64 = torch.float64, torch.int64
SLICE = 64            # rows per SELL slice
DELTA_MAX = 32767     # largest |col - row| a 16-bit delta holds


# ---------------------------------------------------------------- meshes
def fan(m):
    """m tets [0, a, a + 1, a + 2], a = 1 .. m, around the hub node 0 (m + 3 nodes): the hub has m incidences, 4 m
    candidates and m + 3 neighbours (itself included)."""
    a = torch.arange(1, m + 1)
    return torch.stack([torch.zeros_like(a), a, a + 1, a + 2], 1)


def helix_fan(m):
    """(coords, fan(m)) with the m + 2 outer nodes on a helix, so that no tet is degenerate."""
    th = torch.arange(1, m + 3, dtype=F64) * 0.3
    pts = torch.stack([torch.cos(th), torch.sin(th), 0.05 * th], 1)
    return torch.cat([torch.zeros(1, 3, dtype=F64), pts]), fan(m)


def tiled(t, r):
    """The connectivity repeated r times (every element r times: r times the incidences, the same neighbours)."""
    return t.repeat(r, 1)


def spread(t, stride):
    """Node ids multiplied by `stride` (the same graph over stride times the id range, unused nodes between)."""
    return t * stride


def reversed_ids(t, N):
    """Node id v -> N - 1 - v (the hub of a fan becomes the last node)."""
    return N - 1 - t


# ---------------------------------------------------------------- incidence
def incidence_ref(t, N):
    """(inc_ptr [N + 1], inc [M npe]) of a connectivity [M, npe]: the slots e * npe + local grouped by node, ascending
    inside every node -- the stable argsort of the flattened connectivity -- and the cumulative node counts."""
    flat = t.reshape(-1)
    inc = torch.sort(flat, stable=True)[1]
    inc_ptr = torch.zeros(N + 1, dtype=I64)
    inc_ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=N), 0)
    return inc_ptr, inc


def diagpos_ref(rowptr, colidx):
    """Position of every row's diagonal entry in a CSR pattern, -1 for a row without one."""
    n = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    on = colidx == rows
    dpos = torch.full((n,), -1, dtype=I64)
    dpos[rows[on]] = torch.nonzero(on, as_tuple=True)[0]
    return dpos


# ---------------------------------------------------------------- SELL-64
def sell_ref(rowptr, colidx, N):
    """SELL-64 layout of a CSR pattern of N rows, as csrc/pattern.hip documents it -> (slice_ptr [S + 1], cols,
    csr2sell [nnz], dcols, far). Slice s holds rows 64 s .. 64 s + 63 and is as wide as its longest row; entry k of the
    row in lane `lane` sits at slice_ptr[s] + 64 k + lane. Padding is the row's own index, N - 1 for the lanes past
    the last row. dcols = col - (64 s + lane), 0 where |delta| > 32767, and `far` says that some delta was."""
    S = (N + SLICE - 1) // SLICE
    rlen = torch.zeros(S * SLICE, dtype=I64)
    rlen[:N] = rowptr[1:] - rowptr[:-1]
    width = rlen.view(S, SLICE).max(1)[0] if S else rlen
    slice_ptr = torch.zeros(S + 1, dtype=I64)
    slice_ptr[1:] = torch.cumsum(width * SLICE, 0)
    ent = int(slice_ptr[-1])
    s = torch.repeat_interleave(torch.arange(S), width * SLICE)
    off = torch.arange(ent) - slice_ptr[s]
    k, lane = off // SLICE, off % SLICE
    r = s * SLICE + lane
    real = k < rlen[r]
    rp = torch.zeros(S * SLICE, dtype=I64)
    rp[:N] = rowptr[:-1]
    cols = torch.where(r < N, r, torch.full_like(r, N - 1))
    cols[real] = colidx[(rp[r] + k)[real]]
    csr2sell = torch.empty(colidx.numel(), dtype=I64)
    csr2sell[(rp[r] + k)[real]] = torch.arange(ent)[real]
    d = cols - r
    out = d.abs() > DELTA_MAX
    dcols = torch.where(out, torch.zeros_like(d), d)
    return slice_ptr, cols, csr2sell, dcols, bool(out.any())


def sell_dense(slice_ptr, cols, N):
    """0 / 1 matrix [N, N] with a one wherever the SELL pattern names a column (padding: the diagonal)."""
    A = torch.zeros(N, N, dtype=I64)
    S = slice_ptr.numel() - 1
    for s in range(S):
        e0, e1 = int(slice_ptr[s]), int(slice_ptr[s + 1])
        blk = cols[e0:e1].view(-1, SLICE)          # [width, lane]
        for lane in range(min(SLICE, N - s * SLICE)):
            A[s * SLICE + lane, blk[:, lane]] = 1
    return A


# ---------------------------------------------------------------- dof CSR
def dof_csr_ref(K, t, dpn, N):
    """The coalesced COO of the element matrices K [M, npe dpn, npe dpn] (`R.coo_to_csr`) as a CSR of N dpn rows (the
    rows of unused trailing nodes empty) -> (rowptr, colidx, vals, diagpos, mag, cnt): diagpos -1 where the row has no
    diagonal, mag the same coalesce of |K| (the magnitude sum behind every entry) and cnt the number of contributions
    to every entry -- what a rounding bound of the entry's sum needs."""
    rp, ci, vals = R.coo_to_csr(K, t, dpn)
    _, ci2, mag = R.coo_to_csr(K.abs(), t, dpn)
    _, ci3, cnt = R.coo_to_csr(torch.ones_like(K), t, dpn)
    assert torch.equal(ci, ci2) and torch.equal(ci, ci3)
    rowptr = torch.full((N * dpn + 1,), int(rp[-1]), dtype=I64)
    rowptr[: rp.numel()] = rp
    return rowptr, ci, vals, diagpos_ref(rowptr, ci), mag, cnt.round().long()


def sum_bound(mag, cnt):
    """|a - b| allowed between two fp64 sums, in any two orders, of the same n = max(cnt) terms whose magnitudes add
    up to mag: each is within (n - 1) 2^-53 mag of the exact sum, so the two differ by less than 2 n 2^-53 mag."""
    return 2.0 * float(cnt.max()) * 2.0 ** -53 * mag
