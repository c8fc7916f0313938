"""Node renumbering (opt-in RCM, csrc/reorder.hip) -- CPU tier: the oracle's rule (oracle/rcm_ref.py) gives a
permutation, undoes a random numbering of the Kuhn cube down to the bandwidth of scipy's reverse Cuthill-McKee, and
handles several components and nodes no element touches. The device implementation equals this oracle exactly
(tests/test_gpu_reorder.py).

The level-by-level restatement of the same rule (tests/rcm_levels_ref.py), which stands in for the oracle where the
oracle's Python edge walk is too slow, equals the oracle exactly on every graph family of the edge tests
(tests/test_gpu_reorder_edges.py) up to the 262,145-wide one, and every family reaches the kernel path it is there
for, by the restatement's level structure."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import reverse_cuthill_mckee
import torch

import fem355  # noqa: F401
from fem355 import mesh
from oracle import ref_cpu as R
from oracle import rcm_ref
import rcm_levels_ref as L


def _permuted_cube(n, seed):
    c, t = mesh.kuhn_cube(n)
    perm = torch.randperm(c.shape[0], generator=torch.Generator().manual_seed(seed))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return c[perm], inv[t]


def _renumbered_pattern(t, N, inv):
    return R.node_pattern(torch.as_tensor(inv)[t], N)


def test_rcm_oracle_restores_a_narrow_band():
    c, t = _permuted_cube(9, 3)
    N = c.shape[0]
    rp, ci = R.node_pattern(t, N)
    bw0 = rcm_ref.bandwidth(rp, ci)
    perm, inv = rcm_ref.rcm(rp.numpy(), ci.numpy(), N)
    assert np.array_equal(np.sort(perm), np.arange(N)) and np.array_equal(inv[perm], np.arange(N))
    rp2, ci2 = _renumbered_pattern(t, N, inv)
    bw = rcm_ref.bandwidth(rp2, ci2)
    A = sp.csr_matrix((np.ones(ci.numel()), ci.numpy(), rp.numpy()), shape=(N, N))
    q = reverse_cuthill_mckee(A, symmetric_mode=True)
    qi = np.empty(N, dtype=np.int64)
    qi[q] = np.arange(N)
    rp3, ci3 = _renumbered_pattern(t, N, qi)
    bw_scipy = rcm_ref.bandwidth(rp3, ci3)
    assert bw0 > 5 * bw and bw <= 1.5 * bw_scipy, (bw0, bw, bw_scipy)
    # the lexicographic cube's bandwidth is (n+1)^2 + (n+1) + 1; RCM stays within a small factor of it
    assert bw <= 3 * (10 * 10 + 10 + 1)


def test_rcm_oracle_components_and_unused_nodes():
    c, t = mesh.kuhn_cube(3)
    N1 = c.shape[0]
    t2 = torch.cat([t, t + N1 + 5])       # two cubes, 5 unused nodes between them, 3 after
    N = 2 * N1 + 8
    rp, ci = R.node_pattern(t2, N)
    perm, inv = rcm_ref.rcm(rp.numpy(), ci.numpy(), N)
    assert np.array_equal(np.sort(perm), np.arange(N))
    unused = list(range(N1, N1 + 5)) + list(range(2 * N1 + 5, N))
    assert list(perm[N - 8:]) == unused                  # nodes without elements last, ascending
    # each component is contiguous in the new numbering
    new_first = inv[:N1]
    assert new_first.max() - new_first.min() == N1 - 1


@pytest.mark.parametrize("name", [n for n in L.NAMES if n != "spoked-1048577"])
def test_level_restatement_equals_oracle(name):
    """The 1,048,577-wide case is left to the restatement alone (the oracle's edge walk takes too long there)."""
    _, N, rp, ci, s = L.case(name)
    perm, inv = rcm_ref.rcm(rp, ci, N)
    assert np.array_equal(s.perm, perm) and np.array_equal(s.inv, inv)
    assert sum(int(c.sum()) for comp in s.counts for c in comp) + s.components == sum(map(sum, s.widths))


@pytest.mark.parametrize("name", L.NAMES)
def test_edge_families_reach_their_regime(name):
    _, N, rp, _, s = L.case(name)
    assert np.array_equal(np.sort(s.perm), np.arange(N)) and np.array_equal(s.inv[s.perm], np.arange(N))
    L.assert_regime(name, N, rp, s)
