"""CPU tier of the pattern references (tests/pattern_ref.py): the helpers agree with what the oracle already has
(`R.node_pattern`, `R.coo_to_csr`) and with a dense restatement, and the arithmetic that puts the GPU tests' meshes
exactly on the kernels' size thresholds is pinned here, so that a GPU test cannot quietly miss its edge."""
import pytest
import torch

import pattern_ref as P
from oracle import ref_cpu as R

F64 = torch.float64


def _meshes():
    import fem355  # noqa: F401
    from fem355 import mesh
    return [mesh.kuhn_cube(3), mesh.hex_box(2)]


def _dense_pattern(t, N):
    A = torch.zeros(N, N, dtype=torch.long)
    for a in range(t.shape[1]):
        for b in range(t.shape[1]):
            A[t[:, a], t[:, b]] = 1
    return A


@pytest.mark.parametrize("k", [0, 1])
def test_incidence_ref_is_the_sorted_slot_list(k):
    c, t = _meshes()[k]
    N = c.shape[0] + 3                                       # three unused trailing nodes
    ip, inc = P.incidence_ref(t, N)
    assert ip.numel() == N + 1 and int(ip[0]) == 0 and int(ip[-1]) == t.numel()
    flat = t.reshape(-1)
    for n in range(N):
        seg = inc[ip[n]:ip[n + 1]]
        want = torch.nonzero(flat == n, as_tuple=True)[0]    # ascending slots of node n
        assert torch.equal(seg, want), n


@pytest.mark.parametrize("k", [0, 1])
def test_sell_ref_rebuilds_the_node_pattern(k):
    c, t = _meshes()[k]
    for N in (c.shape[0], c.shape[0] + 5):
        rp, ci = R.node_pattern(t, N)
        A = _dense_pattern(t, N)
        rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
        B = torch.zeros_like(A)
        B[rows, ci] = 1
        assert torch.equal(A, B)                                        # the oracle's pattern, dense
        sp, cols, c2s, dcols, far = P.sell_ref(rp, ci, N)
        S = (N + 63) // 64
        assert sp.numel() == S + 1 and int(sp[-1]) == cols.numel() and not far
        # the SELL pattern names exactly the pattern's columns, plus the diagonal in every row shorter than its
        # slice is wide (padding)
        D = P.sell_dense(sp, cols, N)
        width = (sp[1:] - sp[:-1]) // 64
        padded = width[torch.arange(N) // 64] > rp[1:] - rp[:-1]
        assert torch.equal(D, torch.clamp(A + torch.diag(padded.long()), max=1))
        assert torch.equal(cols[c2s], ci)                               # the map points at the entry's column
        assert c2s.unique().numel() == ci.numel()
        e = torch.arange(cols.numel())
        s = torch.searchsorted(sp, e, right=True) - 1
        r = s * 64 + (e - sp[s]) % 64
        assert torch.equal(dcols, cols - r)
        pad = torch.ones(cols.numel(), dtype=torch.bool)
        pad[c2s] = False
        assert torch.equal(cols[pad], torch.clamp(r[pad], max=N - 1))   # own row, N - 1 past the last row
        assert torch.equal(P.diagpos_ref(rp, ci) >= 0, A.diagonal() > 0)


def test_sell_ref_far_columns():
    rp = torch.tensor([0, 2, 3])
    N = 40000
    rowptr = torch.full((N + 1,), 3)
    rowptr[:3] = rp
    ci = torch.tensor([0, 32767, 32769])                # row 0: delta 32767 fits; row 1: delta 32768 does not
    sp, cols, c2s, dcols, far = P.sell_ref(rowptr, ci, N)
    assert far and dcols[c2s].tolist() == [0, 32767, 0] and cols[c2s].tolist() == [0, 32767, 32769]
    _, _, _, _, far = P.sell_ref(rowptr, torch.tensor([0, 32767, 32768]), N)
    assert not far


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("dpn", [1, 3])
def test_dof_csr_ref_against_dense(k, dpn):
    c, t = _meshes()[k]
    N = c.shape[0] + 2
    d = t.shape[1] * dpn
    K = torch.randn(t.shape[0], d, d, dtype=F64, generator=torch.Generator().manual_seed(3))
    rp, ci, vals, dpos, mag, cnt = P.dof_csr_ref(K, t, dpn, N)
    rp0, ci0, v0 = R.coo_to_csr(K, t, dpn)
    assert torch.equal(rp[: rp0.numel()], rp0) and torch.equal(ci, ci0) and torch.equal(vals, v0)
    assert rp.numel() == N * dpn + 1 and bool((rp[rp0.numel():] == rp0[-1]).all())
    dofs = R.dof_map(t, dpn)
    A = torch.zeros(N * dpn, N * dpn, dtype=F64)
    Amag = torch.zeros_like(A)
    Acnt = torch.zeros_like(A)
    for e in range(t.shape[0]):
        A[dofs[e][:, None], dofs[e][None, :]] += K[e]
        Amag[dofs[e][:, None], dofs[e][None, :]] += K[e].abs()
        Acnt[dofs[e][:, None], dofs[e][None, :]] += 1.0
    rows = torch.repeat_interleave(torch.arange(N * dpn), rp[1:] - rp[:-1])
    assert torch.equal(Acnt[rows, ci].long(), cnt) and int((Acnt > 0).sum()) == ci.numel()
    assert bool(((A[rows, ci] - vals).abs() <= P.sum_bound(mag, cnt)).all())
    assert bool(((Amag[rows, ci] - mag).abs() <= P.sum_bound(mag, cnt)).all())
    assert torch.equal(dpos[: c.shape[0] * dpn], torch.nonzero(ci == rows, as_tuple=True)[0])
    assert bool((dpos[c.shape[0] * dpn:] == -1).all())
    if dpn == 1:                                          # the node pattern is the dpn = 1 dof pattern
        nrp, nci = R.node_pattern(t, N)
        assert torch.equal(rp, nrp) and torch.equal(ci, nci)


def test_mesh_builders():
    t = P.fan(5)
    assert t.tolist() == [[0, 1, 2, 3], [0, 2, 3, 4], [0, 3, 4, 5], [0, 4, 5, 6], [0, 5, 6, 7]]
    c, t2 = P.helix_fan(5)
    assert torch.equal(t, t2) and c.shape == (8, 3) and float(R.tet_volumes(c, t2).abs().min()) > 0
    assert torch.equal(P.tiled(t, 3), torch.cat([t, t, t])) and torch.equal(P.spread(t, 7), 7 * t)
    assert torch.equal(P.reversed_ids(t, 8), 7 - t)


@pytest.mark.parametrize("m", [8, 29, 30, 509, 510])
def test_fan_hub_counts(m):
    """The hub of fan(m): m incidences, 4 m candidates, m + 3 neighbours; every other node has at most 3 incidences
    and 7 neighbours, so the hub is the only row near a tier's edge."""
    t = P.fan(m)
    N = m + 3
    ip, _ = P.incidence_ref(t, N)
    rp, _ = R.node_pattern(t, N)
    assert int(ip[1] - ip[0]) == m and 4 * int(ip[1] - ip[0]) == 4 * m and int(rp[1] - rp[0]) == m + 3
    assert int((ip[2:] - ip[1:-1]).max()) <= 3 and int((rp[2:] - rp[1:-1]).max()) <= 7
    tr = P.reversed_ids(t, N)
    ipr, _ = P.incidence_ref(tr, N)
    rpr, _ = R.node_pattern(tr, N)
    assert int(ipr[N] - ipr[N - 1]) == m and int(rpr[N] - rpr[N - 1]) == m + 3
    t6 = P.tiled(t, 6)
    ip6, _ = P.incidence_ref(t6, N)
    assert int(ip6[1] - ip6[0]) == 6 * m and torch.equal(R.node_pattern(t6, N)[1], R.node_pattern(t, N)[1])


def test_bucket_zero_fill_of_a_fan():
    """Entries of the incidence's bucket 0 (nodes 0 .. 127) of fan(m): 3,584 at m = 3,206 and 3,585 at m = 3,207."""
    assert int((P.fan(3206).reshape(-1) >> 7 == 0).sum()) == 3584
    assert int((P.fan(3207).reshape(-1) >> 7 == 0).sum()) == 3585
