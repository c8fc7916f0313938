"""GPU: the face-key widths, multiplicities and element families of `csrc/topology.hip` that
`tests/test_gpu_topology.py` does not reach.

`fem_topo_create` packs the sorted node ids of a face at bits = ceil(log2 N) each (N = max id + 1) into one 64-bit
key while fpn * bits <= 64, else into a (hi, lo) pair with its own low-word pass, gathers and stable high-word pass.
Meshes of about a thousand elements whose ids are relabelled into [0, top) (`tests/test_topology_cpu.py::relabel`,
order-keeping and order-changing) put N on both sides of every switch:
  triangles   top = 2^21 - 1, 2^21, 2^21 + 1, 2^22 + 3, 2^31 + 5, 2^32   (two words above 2^21)
  quads       top = 2^16 - 1, 2^16 (all 64 key bits), 2^16 + 1, 2^20, 2^32   (two words above 2^16)
  wedges      both lists (quad group and triangle group)
  edges       top = 2^31, 2^32 - 1, 2^32 (one word, all 64 key bits)
An id of 2^32 or more is refused (`FemError`, FEM_EARG). `nonmanifold` meshes (faces of multiplicity 1 to 4,
a duplicated element, a face with a repeated node) are grouped with one-word and two-word keys: faces seen
more than twice are neither surface nor pair, like the reference (`solver/element.py:543-579,707-762`).
Hexes and wedges are also checked at 12^3 cells with elements removed and shuffled, normals included.

Oracle: `oracle.ref_cpu.{boundary_faces, shared_faces, unique_edges, surface_normals, element_face_normals,
split_elements}` on the same relabelled mesh. Index outputs bit-exact (pairs up to the in-pair order, `canon`),
normals 1e-14 relative with NaN in every coordinate row that no element uses.
"""
import functools

import pytest
import torch

from conftest import rel
from oracle import ref_cpu as R
from test_gpu_topology import canon
from test_topology_cpu import (EDGE_TOPS, QUAD_TOPS, TRI_TOPS, WEDGE_TOPS, family, multiplicities, nonmanifold_case,
                               prep, relabel, scatter_coords)

pytestmark = pytest.mark.gpu
F64 = torch.float64
MONO = pytest.mark.parametrize("monotone", [True, False])


def _mods():
    import fem355  # noqa: F401
    from fem355 import element, mesh, topology
    return element, mesh, topology


@functools.lru_cache(maxsize=None)
def case(kind, top, monotone):
    """The 6^3 mesh of `kind` (shuffled, 5% removed) with its ids relabelled into [0, top)."""
    el, _ = family(kind)
    new, _ = relabel(el, top, seed=top % 1000 + 7, monotone=monotone)
    assert int(new.max()) + 1 == top
    return new


def sorted_unique(el, tab):
    return torch.unique(torch.sort(el[:, torch.tensor(tab)], dim=2)[0].reshape(-1, len(tab[0])), dim=0)


def check_groups(T, el, tab, gpu):
    """FaceGroups counts and unique faces against torch.unique of the sorted faces."""
    cnt = multiplicities(el, tab)
    g = T.FaceGroups(el, tab, gpu)
    try:
        assert (g.n_unique, g.n_single, g.n_pair) == (cnt.numel(), int((cnt == 1).sum()), int((cnt == 2).sum()))
        assert torch.equal(g.unique().cpu(), sorted_unique(el, tab))
    finally:
        g.close()
    return cnt


def check_shared(fn, el, tab, gpu):
    sh = fn(el, device=gpu).cpu()
    F = len(tab)
    assert sh.shape[0] > 0
    assert torch.equal(sh, canon(sh, F)) and torch.equal(sh, canon(R.shared_faces(el, tab), F))


def check_surface(got, el, stab, xtab):
    f, x = got
    fr, xr = R.boundary_faces(el, stab, xtab)
    assert fr.shape[0] > 0
    assert torch.equal(f.cpu(), fr) and torch.equal(x.cpu(), xr)


# ---------------------------------------------------------------- key-width sweep
@MONO
@pytest.mark.parametrize("top", TRI_TOPS)
def test_tet_key_widths(gpu, top, monotone):
    el, _, T = _mods()
    t = case("tet", top, monotone)
    check_shared(el.identify_tetrahedral_shared_faces, t, T.TET_SHARED, gpu)
    check_surface(el.compute_tetrahedral_surface_faces_with_fourth_node(t, device=gpu), t, T.TET_SURFACE,
                  T.TET_SURFACE_X)
    check_groups(T, t, T.TET_SHARED, gpu)


@MONO
@pytest.mark.parametrize("top", QUAD_TOPS)
def test_hex_key_widths(gpu, top, monotone):
    el, _, T = _mods()
    h = case("hex", top, monotone)
    check_shared(el.identify_hexahedral_shared_faces, h, T.HEX, gpu)
    check_surface(el.compute_hexahedral_surface_faces_with_extra_node(h, device=gpu), h, T.HEX, T.HEX_SURFACE_X)
    check_groups(T, h, T.HEX, gpu)


@MONO
@pytest.mark.parametrize("top", WEDGE_TOPS)
def test_wedge_key_widths(gpu, top, monotone):
    el, _, T = _mods()
    w = case("wedge", top, monotone)
    (fq, ft), (xq, xt) = el.compute_wedge_surface_faces_with_extra_node(w, device=gpu)
    check_surface((fq, xq), w, T.WEDGE_QUAD, T.WEDGE_QUAD_X)
    check_surface((ft, xt), w, T.WEDGE_TRI, T.WEDGE_TRI_X)
    check_groups(T, w, T.WEDGE_QUAD, gpu)
    check_groups(T, w, T.WEDGE_TRI, gpu)


@MONO
@pytest.mark.parametrize("top", EDGE_TOPS)
def test_edge_key_widths(gpu, top, monotone):
    el, _, T = _mods()
    t = case("tet", top, monotone)
    e = el.element_to_edge(t, device=gpu).cpu()
    assert torch.equal(e, R.unique_edges(t, T.EDGES))
    assert int(e.max()) == top - 1


# ---------------------------------------------------------------- element graph, splits
@MONO
@pytest.mark.parametrize("kind,top", [("tet", 2**21), ("tet", 2**21 + 1), ("hex", 2**16), ("hex", 2**16 + 1)])
def test_element_adjacency_rows_and_columns(gpu, kind, top, monotone):
    el, _, T = _mods()
    e = case(kind, top, monotone)
    M = e.shape[0]
    pairs = R.shared_faces(e, T.TET_SHARED if kind == "tet" else T.HEX)
    a, b = pairs[:, 0, 0], pairs[:, 1, 0]
    key = torch.unique(torch.cat([a, b]) * M + torch.cat([b, a]))
    ref_ptr = torch.zeros(M + 1, dtype=torch.long)
    ref_ptr[1:] = torch.cumsum(torch.bincount(key // M, minlength=M), 0)
    rowptr, cols = el.element_adjacency(e, device=gpu)
    assert int(ref_ptr[-1]) == 2 * pairs.shape[0] > 0
    assert torch.equal(rowptr.cpu(), ref_ptr) and torch.equal(cols.cpu(), key % M)


@MONO
@pytest.mark.parametrize("top", [2**31 + 5, 2**32])
def test_splits_keep_large_ids(gpu, top, monotone):
    el, mesh, T = _mods()
    h, w = case("hex", 2**32, monotone), case("wedge", 2**32, monotone)
    q, _ = relabel(mesh.tet10_cube(3)[1], top, seed=21, monotone=monotone)
    assert torch.equal(el.c3d8_to_c3d4(h, device=gpu).cpu(), R.split_elements(h, T.SPLIT[8]))
    assert torch.equal(el.c3d6_to_c3d4(w, device=gpu).cpu(), R.split_elements(w, T.SPLIT[6]))
    out = el.c3d10_to_c3d4(q, device=gpu).cpu()
    assert torch.equal(out, R.split_elements(q, T.SPLIT[10])) and int(out.max()) >= 2**31


# ---------------------------------------------------------------- ids the keys cannot hold
@pytest.mark.parametrize("bad", [2**32, 2**40])
def test_ids_from_2_32_are_refused(gpu, bad):
    """N = max id + 1 > 2^32 is FEM_EARG in fem_topo_create, which `_capi.check` raises as FemError."""
    el, _, T = _mods()
    from fem355 import _capi
    t = case("tet", 2**32, False).clone()
    h = case("hex", 2**32, False).clone()
    w = case("wedge", 2**32, False).clone()
    for m in (t, h, w):
        m[m.shape[0] // 2, 1] = bad
    calls = [(el.identify_tetrahedral_shared_faces, t), (el.compute_tetrahedral_surface_faces_with_fourth_node, t),
             (el.element_to_edge, t), (el.element_adjacency, t), (el.identify_hexahedral_shared_faces, h),
             (el.compute_hexahedral_surface_faces_with_extra_node, h),
             (el.compute_wedge_surface_faces_with_extra_node, w)]
    for fn, m in calls:
        with pytest.raises(_capi.FemError, match=r"2\^32"):
            fn(m, device=gpu)
    with pytest.raises(_capi.FemError, match=r"2\^32"):
        T.FaceGroups(t, T.EDGES, gpu)


# ---------------------------------------------------------------- non-manifold and degenerate meshes
@pytest.mark.parametrize("kind,top", [("tet", None), ("tet", 2**22 + 3), ("hex", None), ("hex", 2**20)])
def test_nonmanifold(gpu, kind, top):
    """Faces of multiplicity 1..4, a duplicated element and a face with a repeated node, with one-word
    keys (plain ids) and two-word keys."""
    el, _, T = _mods()
    m, tab = nonmanifold_case(kind)
    if kind == "tet":
        stab, xtab = T.TET_SURFACE, T.TET_SURFACE_X
        shared, surface = el.identify_tetrahedral_shared_faces, el.compute_tetrahedral_surface_faces_with_fourth_node
    else:
        stab, xtab = T.HEX, T.HEX_SURFACE_X
        shared, surface = el.identify_hexahedral_shared_faces, el.compute_hexahedral_surface_faces_with_extra_node
    if top is not None:
        m, _ = relabel(m, top, seed=33, monotone=False)
    check_shared(shared, m, tab, gpu)
    check_surface(surface(m, device=gpu), m, stab, xtab)
    assert torch.equal(el.element_to_edge(m, device=gpu).cpu(), R.unique_edges(m, T.EDGES))
    cnt = check_groups(T, m, tab, gpu)
    assert {1, 2, 3, 4} <= set(cnt.tolist())
    g = T.FaceGroups(m, tab, gpu)
    n_single, n_pair = g.n_single, g.n_pair
    g.close()
    assert 2 * n_pair + n_single < m.shape[0] * len(tab)      # faces seen three times or more exist and are dropped


# ---------------------------------------------------------------- normals
def check_normals(el, T, kind, c, e, gpu):
    """Both kinds of normals of family `kind` against the oracle; no NaN in any output."""
    if kind == "tet":
        f, x = R.boundary_faces(e, T.TET_SURFACE, T.TET_SURFACE_X)
        got = [el.compute_tetrahdral_surface_normals(c, e, device=gpu, dtype=F64),
               el.compute_tetrahedral_normals_and_area(c, e, device=gpu, dtype=F64)]
        ref = [R.surface_normals(c, f, x, 2),
               R.element_face_normals(c, e, T.TET_SHARED, T.TET_SHARED, T.TET_SHARED_X, scale=0.5)]
    elif kind == "hex":
        f, x = R.boundary_faces(e, T.HEX, T.HEX_SURFACE_X)
        got = [el.compute_hexahedral_surface_normals(c, e, device=gpu, dtype=F64),
               el.compute_hexahedral_normals_and_area(c, e, device=gpu, dtype=F64)]
        ref = [R.surface_normals(c, f, x, 2),
               R.element_face_normals(c, e, T.HEX, [[r[0], r[1], r[3]] for r in T.HEX], T.HEX_AREA_X)]
    else:
        fq, xq = R.boundary_faces(e, T.WEDGE_QUAD, T.WEDGE_QUAD_X)
        ft, xt = R.boundary_faces(e, T.WEDGE_TRI, T.WEDGE_TRI_X)
        nq, nt = el.compute_wedge_surface_normals(c, e, device=gpu, dtype=F64)
        got = [nq, nt, el.compute_wedge_normals_and_area(c, e, device=gpu, dtype=F64)]
        rows = [[r[0], r[1], r[3]] for r in T.WEDGE_QUAD] + [list(r) for r in T.WEDGE_TRI]
        ref = [R.surface_normals(c, fq, xq, 3), R.surface_normals(c, ft, xt, 2),
               R.element_face_normals(c, e, None, rows, unit=True)]
    for a, b in zip(got, ref):
        assert a.shape == b.shape and a.shape[0] > 0
        assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any())
        assert rel(a, b) < 1e-14


def jittered(mesh, kind, n):
    make = {"tet": mesh.kuhn_cube, "hex": mesh.hex_box, "wedge": mesh.wedge_box}[kind]
    return make(n, jitter=0.1)


@MONO
@pytest.mark.parametrize("kind,top", [("tet", 2**21 + 1), ("hex", 2**16 + 1), ("wedge", 2**16 + 1)])
def test_normals_on_relabelled_mesh(gpu, kind, top, monotone):
    """Two-word keys, coordinates scattered into [top, 3] with NaN in every row no element uses: a kernel that
    reads a wrong node returns NaN."""
    el, mesh, T = _mods()
    c, e = jittered(mesh, kind, 6)
    e, idmap = relabel(prep(e, 41), top, seed=42, monotone=monotone)
    check_normals(el, T, kind, scatter_coords(c, idmap, top), e, gpu)


# ---------------------------------------------------------------- medium hexes and wedges, plain ids
def test_hex_medium_vs_oracle(gpu):
    """12^3 jittered hexes, 5% removed (inner surfaces), shuffled element order; one-word keys."""
    el, mesh, T = _mods()
    c, h = jittered(mesh, "hex", 12)
    h = prep(h, 51)
    check_surface(el.compute_hexahedral_surface_faces_with_extra_node(h, device=gpu), h, T.HEX, T.HEX_SURFACE_X)
    check_shared(el.identify_hexahedral_shared_faces, h, T.HEX, gpu)
    check_groups(T, h, T.HEX, gpu)
    check_normals(el, T, "hex", c, h, gpu)


def test_wedge_medium_vs_oracle(gpu):
    """12^3 cells of jittered wedges (3,456), 5% removed, shuffled element order; one-word keys."""
    el, mesh, T = _mods()
    c, w = jittered(mesh, "wedge", 12)
    w = prep(w, 52)
    (fq, ft), (xq, xt) = el.compute_wedge_surface_faces_with_extra_node(w, device=gpu)
    check_surface((fq, xq), w, T.WEDGE_QUAD, T.WEDGE_QUAD_X)
    check_surface((ft, xt), w, T.WEDGE_TRI, T.WEDGE_TRI_X)
    check_groups(T, w, T.WEDGE_QUAD, gpu)
    check_groups(T, w, T.WEDGE_TRI, gpu)
    check_normals(el, T, "wedge", c, w, gpu)
