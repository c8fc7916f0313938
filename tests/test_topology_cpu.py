"""CPU: the inputs of `tests/test_gpu_topology_keys.py` (sparse node ids, non-manifold meshes), checked on the oracle.

`fem_topo_create` packs a face's sorted node ids at ceil(log2 N) bits each, N = max id + 1, into one 64-bit key or a
(hi, lo) pair (`csrc/topology.hip`). `relabel` moves a small mesh's ids into [0, top) with the largest at top - 1, so
that N == top exactly and a few hundred elements reach every key width; `nonmanifold` adds duplicated and partly
duplicated elements, so that faces of multiplicity 1, 2, 3 and 4 and a face with a repeated node occur.
Relabelling must not change the topology: on every `top` of the GPU sweep the oracle's shared (element, face) pairs
and boundary (element, face) set of the relabelled mesh are those of the original mesh.
"""
import pytest
import torch

from oracle import ref_cpu as R

TRI_TOPS = [2**21 - 1, 2**21, 2**21 + 1, 2**22 + 3, 2**31 + 5, 2**32]     # 3 * bits <= 64 up to N = 2^21
QUAD_TOPS = [2**16 - 1, 2**16, 2**16 + 1, 2**20, 2**32]                  # 4 * bits <= 64 up to N = 2^16
WEDGE_TOPS = sorted(set(QUAD_TOPS + TRI_TOPS))                           # quad group and triangle group
EDGE_TOPS = [2**31, 2**32 - 1, 2**32]                                    # always one word; 64 key bits at 2^32


def _mods():
    from fem355 import mesh, topology
    return mesh, topology


def relabel(elements, top, seed, monotone):
    """(connectivity with the used node ids mapped injectively into [0, top), id map [max old id + 1], -1 at unused
    ids). The largest new id is top - 1. monotone keeps the order of the ids; otherwise the new ids are assigned
    in random order, so the sorted order inside a face changes."""
    used = torch.unique(elements)
    k = used.numel()
    assert 0 < k <= top
    gen = torch.Generator().manual_seed(seed)
    if top - 1 < 8 * k:
        rest = torch.randperm(top - 1, generator=gen)[: k - 1]
    else:
        draw = torch.unique(torch.randint(0, top - 1, (4 * k,), generator=gen))
        rest = draw[torch.randperm(draw.numel(), generator=gen)[: k - 1]]
    assert rest.numel() == k - 1
    new = torch.cat([torch.sort(rest)[0], torch.tensor([top - 1])])
    if not monotone:
        new = new[torch.randperm(k, generator=gen)]
    idmap = torch.full((int(used[-1]) + 1,), -1, dtype=torch.long)
    idmap[used] = new
    return idmap[elements], idmap


def scatter_coords(coords, idmap, top):
    """[top, 3] coordinates of the relabelled mesh; NaN in the rows no element uses."""
    out = torch.full((top, coords.shape[1]), float("nan"), dtype=coords.dtype)
    old = torch.nonzero(idmap >= 0, as_tuple=True)[0]
    out[idmap[old]] = coords[old]
    return out


def unlabel(ids, idmap):
    """Old ids of relabelled ids (inverse of the id map; no dense table, top may be 2^32)."""
    old = torch.nonzero(idmap >= 0, as_tuple=True)[0]
    new, order = torch.sort(idmap[old])
    pos = torch.searchsorted(new, ids.reshape(-1))
    assert torch.equal(new[pos], ids.reshape(-1))
    return old[order][pos].reshape(ids.shape)


_KEEP = {4: 3, 8: 4}     # leading nodes that are one face: tet 012, hex 0321


def nonmanifold(t):
    """`t` (tets or hexes) plus duplicated elements (t[:5], then t[:2] again), two partial duplicates that keep
    one face of an element and take the other nodes from a distant element, and one element of the original
    with a repeated node: faces of multiplicity 1, 2, 3 and 4 occur."""
    M, npe = t.shape
    k = _KEEP[npe]
    part = t[[M // 3, M // 3]].clone()
    part[0, k:] = t[M - 1, k:]
    part[1, k:] = t[M - 2, k:]
    out = torch.cat([t, t[:5], t[:2], part], 0).clone()
    out[M // 2, 1] = out[M // 2, 0]
    return out


def multiplicities(elements, table):
    flat = torch.sort(elements[:, torch.tensor(table)], dim=2)[0].reshape(-1, len(table[0]))
    return torch.unique(flat, dim=0, return_counts=True)[1]


def prep(elements, seed, keep=0.95):
    """Seeded shuffle of the element order with 5% of the elements removed (inner surfaces)."""
    p = torch.randperm(elements.shape[0], generator=torch.Generator().manual_seed(seed))
    return elements[p[: int(keep * elements.shape[0])]].contiguous()


def _pair_set(pairs):
    return {frozenset(((int(p[0, 0]), int(p[0, 1])), (int(p[1, 0]), int(p[1, 1])))) for p in pairs}


def _boundary_set(elements, table, extra):
    """(element, face) of every boundary face, recovered from the faces: a boundary face has one owner."""
    owner = {}
    for f, row in enumerate(table):
        for e, nodes in enumerate(elements[:, list(row)].tolist()):
            owner.setdefault(tuple(nodes), []).append((e, f, int(elements[e, extra[f]])))
    faces, xs = R.boundary_faces(elements, table, extra)
    out = set()
    for nodes, x in zip(faces.tolist(), xs.tolist()):
        hits = [h for h in owner[tuple(nodes)] if h[2] == x]
        assert len(hits) == 1
        out.add(hits[0][:2])
    assert len(out) == faces.shape[0]
    return out


def family(kind):
    mesh, T = _mods()
    if kind == "tet":
        return prep(mesh.kuhn_cube(6, jitter=0.1)[1], 11), [(T.TET_SHARED, T.TET_SHARED_X)]
    if kind == "hex":
        return prep(mesh.hex_box(6)[1], 12), [(T.HEX, T.HEX_SURFACE_X)]
    return prep(mesh.wedge_box(6)[1], 13), [(T.WEDGE_QUAD, T.WEDGE_QUAD_X), (T.WEDGE_TRI, T.WEDGE_TRI_X)]


_BASE = {}


def _base(kind):
    """The original mesh's pair and boundary sets, formed once per family."""
    if kind not in _BASE:
        el, tabs = family(kind)
        _BASE[kind] = el, tabs, [(_pair_set(R.shared_faces(el, tab)), _boundary_set(el, tab, x)) for tab, x in tabs]
    return _BASE[kind]


CASES = ([("tet", top) for top in TRI_TOPS] + [("hex", top) for top in QUAD_TOPS] +
         [("wedge", top) for top in WEDGE_TOPS])


@pytest.mark.parametrize("monotone", [True, False])
@pytest.mark.parametrize("kind,top", CASES)
def test_relabel_keeps_topology(kind, top, monotone):
    el, tabs, base = _base(kind)
    new, idmap = relabel(el, top, seed=top % 1000 + 7, monotone=monotone)
    assert int(new.max()) == top - 1 and int(new.min()) >= 0
    assert torch.equal(unlabel(new, idmap), el)
    used = idmap[idmap >= 0]
    assert torch.unique(used).numel() == used.numel() == torch.unique(el).numel()
    if monotone:
        assert bool((used[1:] > used[:-1]).all())
    else:
        assert not bool((used[1:] > used[:-1]).all())
    for (tab, x), (pairs0, bnd0) in zip(tabs, base):
        assert _pair_set(R.shared_faces(new, tab)) == pairs0
        assert _boundary_set(new, tab, x) == bnd0
        assert len(bnd0) > 0 and len(pairs0) > 0


def test_scatter_coords_rows():
    mesh, _ = _mods()
    c, t = mesh.kuhn_cube(3, jitter=0.1)
    t = prep(t, 5)
    top = 2**12 + 1
    new, idmap = relabel(t, top, seed=3, monotone=False)
    big = scatter_coords(c, idmap, top)
    assert big.shape == (top, 3) and torch.equal(big[new], c[t])
    assert int(torch.isnan(big[:, 0]).sum()) == top - torch.unique(t).numel()


def nonmanifold_case(kind, n=6):
    """`nonmanifold` of the n^3 tet or hex mesh in a seeded shuffled element order, and its face table."""
    mesh, T = _mods()
    el, tab = (mesh.kuhn_cube(n, jitter=0.1)[1], T.TET_SHARED) if kind == "tet" else (mesh.hex_box(n)[1], T.HEX)
    return nonmanifold(prep(el, 31 + n, keep=1.0)), tab


@pytest.mark.parametrize("kind,n", [("tet", 6), ("tet", 4), ("hex", 6)])
def test_nonmanifold_multiplicities(kind, n):
    nm, tab = nonmanifold_case(kind, n)
    cnt = multiplicities(nm, tab)
    assert {1, 2, 3, 4} <= set(cnt.tolist())
    # a face with a repeated node exists, and faces above multiplicity 2 are dropped from pairs and surface
    srt = torch.sort(nm[:, torch.tensor(tab)], dim=2)[0]
    assert bool((srt[..., 1:] == srt[..., :-1]).any())
    n1, n2 = int((cnt == 1).sum()), int((cnt == 2).sum())
    assert 2 * n2 + n1 < nm.shape[0] * len(tab)
    assert R.shared_faces(nm, tab).shape[0] == n2
    # relabelling keeps the histogram
    new, _ = relabel(nm, 2**22 + 3, seed=9, monotone=False)
    assert torch.equal(torch.sort(multiplicities(new, tab))[0], torch.sort(cnt)[0])
