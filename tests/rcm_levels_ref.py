"""Level-by-level restatement of the renumbering rule of oracle/rcm_ref.py in numpy, and the graph families of the
renumbering's edge tests -- TEST INFRASTRUCTURE ONLY, written from the rule in rcm_ref's docstring; it calls neither the
package nor the device code.

oracle/rcm_ref.py walks every edge in Python, which is fine up to a few hundred thousand nodes. This file states the
same rule one BFS level at a time: gather the frontier's CSR rows, keep the unvisited targets, give each its parent
(the frontier neighbour with the smallest CM index), number the children by (parent CM index, node id). The first
sweep starts at the lowest-(degree, id) node, later components at the lowest-id unvisited node that has neighbours,
nodes without any come last in id order, and the CM order of the swept nodes is reversed. tests/test_reorder_cpu.py
pins it to rcm_ref.rcm exactly.

Besides (perm, inv) it returns the level structure, from which a test asserts that its input reaches the path of
csrc/reorder.hip it is meant for: per component the widths of the non-empty frontiers, per level every frontier node's
child count (what k_cm_count writes to `cnt`) and the number of children that had more than one candidate parent."""
import functools

import numpy as np
import torch

from oracle import ref_cpu as R
from pattern_ref import fan, spread
from twolevel_ref import kuhn_box


class Sweep:
    """perm, inv: int64 numpy (new node k = old node perm[k]; old node v -> inv[v]).
    starts[c]: start node of component c. widths[c]: its non-empty frontier widths, the start node's 1 first.
    counts[c][l]: child count of every node of that frontier, in CM order. shared[c][l]: how many nodes of the level
    after it had two or more neighbours in that frontier (a real choice of parent)."""

    def __init__(self):
        self.perm = self.inv = None
        self.starts, self.widths, self.counts, self.shared = [], [], [], []

    @property
    def components(self):
        return len(self.starts)

    @property
    def levels(self):
        return sum(len(w) for w in self.widths)

    @property
    def launches(self):
        """Count launches of fem_rcm until the device says it is done: one per non-empty frontier, and one per
        component for the empty frontier after its last level (which starts the next component, or finishes)."""
        return self.levels + self.components


def _rows(rowptr, colidx, nodes):
    """The concatenated CSR rows of `nodes` -> (targets, index into `nodes` of every target's source)."""
    lens = rowptr[nodes + 1] - rowptr[nodes]
    src = np.repeat(np.arange(nodes.size), lens)
    first = np.cumsum(lens) - lens
    q = np.arange(int(lens.sum())) - np.repeat(first, lens) + np.repeat(rowptr[nodes], lens)
    return colidx[q], src


def rcm(rowptr, colidx, n):
    """The renumbering of oracle.rcm_ref.rcm, with its level structure -> Sweep."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    deg = rowptr[1:] - rowptr[:-1]
    live = deg > 0
    seen = ~live                      # nodes without neighbours are never swept
    out = Sweep()
    order = []                        # frontiers in CM order
    ncm = 0
    if live.any():
        ids = np.nonzero(live)[0]
        start = int(ids[np.argmin(deg[ids] * (1 << 32) + ids)])
        cursor = 0
        while True:
            frontier = np.array([start], dtype=np.int64)
            seen[start] = True
            widths, counts, shared = [], [], []
            while frontier.size:
                order.append(frontier)
                widths.append(int(frontier.size))
                tgt, src = _rows(rowptr, colidx, frontier)
                keep = ~seen[tgt]
                tgt, src = tgt[keep], src[keep]
                # src ascends, so a target's first occurrence names its parent: the smallest CM index
                child, first, cand = np.unique(tgt, return_index=True, return_counts=True)
                par = src[first]
                by_parent = np.argsort(par, kind="stable")     # child ascends: ties stay in node-id order
                counts.append(np.bincount(par, minlength=frontier.size))
                shared.append(int((cand > 1).sum()))
                frontier = child[by_parent]
                seen[frontier] = True
                ncm += widths[-1]
            out.starts.append(start)
            out.widths.append(widths)
            out.counts.append(counts)
            out.shared.append(shared)
            rest = np.nonzero(~seen[cursor:])[0]
            if rest.size == 0:
                break
            start = cursor + int(rest[0])
            cursor = start + 1
    cm = np.concatenate(order) if order else np.empty(0, dtype=np.int64)
    iso = np.nonzero(~live)[0]
    out.perm = np.concatenate([cm[::-1], iso])
    out.inv = np.empty(n, dtype=np.int64)
    out.inv[out.perm] = np.arange(n)
    return out


# ---------------------------------------------------------------- graph families (connectivity only)
def spoked(W):
    """fan(W + 1) -- hub 0, outer nodes 1 .. W + 3 -- whose outer nodes v >= 4 with v % 3 != 0 each carry a leaf tet
    [v, x, x + 1, x + 2], x = W + 4 + 2 k for the k-th such node, so consecutive spokes share the leaf node x + 2.
    The sweep starts at node 1, level 1 is {0, 2, 3}, level 2 the W nodes 4 .. W + 3 (all children of the hub) and
    level 3 the leaf nodes: a frontier of W nodes whose child counts vary node by node. -> (tets, N)."""
    v = torch.arange(4, W + 4)
    v = v[v % 3 != 0]
    x = W + 4 + 2 * torch.arange(v.numel())
    leaves = torch.stack([v, x, x + 1, x + 2], 1)
    return torch.cat([fan(W + 1), leaves]), W + 4 + 2 * v.numel() + 1


def beam(k):
    """kuhn_box(1, 1, k): 4 (k + 1) nodes in k + 2 levels from a corner."""
    c, t = kuhn_box(1, 1, k)
    return t, c.shape[0]


def permuted(t, N, seed):
    """The connectivity under a seeded random renumbering of its N nodes."""
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    return inv[t]


def disjoint_tets(M, stride=1, tail=0):
    """M tets on 4 M distinct nodes, ids multiplied by `stride`, `tail` unused nodes after the last -> (tets, N)."""
    t = spread(torch.arange(4 * M).view(M, 4), stride)
    return t, int(t.max()) + 1 + tail


def tile_edge(N):
    """spread(fan(300), 7) cut to the tets below N (N = 1: one tet on node 0 alone): unused ids between the fan's
    nodes all the way up to N - 1. -> (tets, N)."""
    if N == 1:
        return torch.zeros(1, 4, dtype=torch.long), 1
    t = spread(fan(300), 7)
    return t[(t < N).all(1)], N


FAMILIES = {
    **{f"spoked-{W}": functools.partial(spoked, W) for W in (255, 256, 257, 513, 262145, 1048577)},
    **{f"beam-{k}": functools.partial(beam, k) for k in (44, 45, 46, 92, 93, 94)},
    "tets-120": functools.partial(disjoint_tets, 120),
    "tets-12-spread": functools.partial(disjoint_tets, 12, 40000, 4),
    **{f"tile-{N}": functools.partial(tile_edge, N) for N in (2047, 2048, 2049, 1)},
}
# cases too large for the edge-walking oracle within a few seconds: compared with the restatement
LARGE = ("spoked-262145", "spoked-1048577")


@functools.lru_cache(maxsize=2)
def case(name):
    """(tets, N, rowptr, colidx, Sweep) of a family, built once and shared by the regime assertions and the
    comparison of a test (the last two cases stay cached)."""
    if name == "cube-24":
        import fem355  # noqa: F401
        from fem355 import mesh
        c, t = mesh.kuhn_cube(24)
        N = c.shape[0]
        t = permuted(t, N, 5)
    else:
        t, N = FAMILIES[name]()
    rp, ci = R.node_pattern(t, N)
    rp, ci = rp.numpy(), ci.numpy()
    return t, N, rp, ci, rcm(rp, ci, N)


NAMES = tuple(FAMILIES) + ("cube-24",)


# ---------------------------------------------------------------- which path of csrc/reorder.hip a family reaches
# Copies of the kernel's constants. Retuning one of them moves the edges these families sit on: the assertions
# below then fail until the families move with it.
CM_G = 256              # CM_G: workgroups of k_cm_count / k_cm_write, so a chunk is ceil(width / CM_G) frontier nodes
CM_NT = 1024            # CM_NT: their threads = counts per block scan of k_cm_write
CM_CHUNK = 4096         # CM_CHUNK: counts per LDS round of k_cm_write
CURSOR_STRIDE = 16384   # ids per round of cm_scan_step's search for the next component (16 CM_NT)
BATCH = 48              # BATCH: count / write launch pairs of fem_rcm between two host reads of the state words
SCAN_TILE = 2048        # SCAN_TILE of fem_scan_i32 (runtime.hip), which places the nodes without neighbours
SCAN_BLOCK = 256        # SCAN_BLOCK: tile sums per round of its second pass


def chunk_len(width):
    return -(-width // CM_G)


def assert_regime(name, N, rowptr, s):
    """What the family `name` is in the suite for, asserted on the reference's level structure `s` alone: a
    condition on the test's input, checked before it touches the device."""
    kind, _, arg = name.partition("-")
    deg = rowptr[1:] - rowptr[:-1]
    iso = np.nonzero(deg == 0)[0]
    if kind == "spoked":
        W = int(arg)
        assert s.components == 1 and s.widths[0][:3] == [1, 3, W], s.widths
        cnt = s.counts[0][2]
        assert cnt.size == W and 4 * int((cnt > 0).sum()) >= W and len(set(cnt.tolist())) >= 3
        assert s.shared[0][2] >= 1                      # a leaf node between two spokes: atomicMin chooses
        c = chunk_len(W)
        want = {255: W < CM_G and c == 1,               # fewer nodes than workgroups: empty chunks at the end
                256: W == CM_G and c == 1,              # one node in every workgroup
                257: W == CM_G + 1 and c == 2,          # the first width of two-node chunks, the last chunks empty
                513: c == 3,
                262145: CM_NT < c <= CM_CHUNK,          # several block scans in one LDS round
                1048577: c > CM_CHUNK}[W]               # several LDS rounds
        assert want, (W, c)
        # the carries matter: children on both sides of the first scan / round edge of a chunk
        for edge in (CM_NT, CM_CHUNK):
            if c > edge:
                assert cnt[:edge].any() and cnt[edge:c].any()
    elif kind == "beam":
        k = int(arg)
        want = {44: BATCH - 1, 45: BATCH, 46: BATCH + 1, 92: 2 * BATCH - 1, 93: 2 * BATCH, 94: 2 * BATCH + 1}[k]
        assert s.components == 1 and s.launches == want == k + 3, (s.launches, want)
    elif kind == "cube":
        wide = [(w, c, sh) for w, c, sh in zip(s.widths[0], s.counts[0], s.shared[0]) if chunk_len(w) >= 2]
        assert s.components == 1 and max(s.widths[0]) == 625 and len(wide) >= 10
        assert all(c.any() and sh > 0 for _, c, sh in wide)      # real counts, many-parent nodes in every wide level
        assert s.launches > BATCH
    elif name == "tets-120":
        assert s.components == 120 and s.launches == 360 and -(-s.launches // BATCH) == 8 and iso.size == 0
    elif name == "tets-12-spread":
        assert s.components == 12 and N == 1_880_005 and iso.size == N - 48
        assert int(np.diff(s.starts).min()) > 9 * CURSOR_STRIDE            # some ten rounds per search
        assert N > SCAN_BLOCK * SCAN_TILE                                  # a second round of tile sums
    elif kind == "tile":
        assert N in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 1)
        if N == 1:
            assert s.widths == [[1]] and iso.size == 0
        else:
            assert iso.size > N // 2 and iso[0] < 7 and iso[-1] == N - 1   # unused ids up to the last one
            assert s.perm[-1] == N - 1 and (N <= SCAN_TILE or iso[-2] == SCAN_TILE - 1)
    else:
        raise KeyError(name)
