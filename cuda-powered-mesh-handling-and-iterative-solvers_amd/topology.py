"""Mesh topology on the device: surface faces, shared faces (the element graph the
reference's region-growing partitioner consumes, `subdivision.ipynb` cells 8-9), unique edges, face normals and
the c3d8/c3d6/c3d10 -> c3d4 splits, with the reference's names and return conventions
(`solver/element.py:543-762,963-993,1293-1581,2234-2446,2687-2713`).

Face grouping runs in one `fem_topo` context (`csrc/topology.hip`): packed sorted-node keys, a stable radix sort,
run detection; the compactions reproduce torch.unique(dim=0) row order and the reference's pairing order.
Node ids must be in [0, N) with N = max id + 1 (IndexError otherwise, like the reference's indexing).
The curvature helpers of the reference (`:621-650`, `:1376-1416`, `:2340-2375`) are not provided: they read an
undefined `face_normals` / call the normals function with a wrong signature and raise in the reference itself.
"""
from __future__ import annotations

import ctypes

import torch

try:
    from . import _capi as C
    from . import system as _sys
except ImportError:  # pragma: no cover - flat import from the package directory
    import _capi as C  # type: ignore
    import system as _sys  # type: ignore

F64 = torch.float64
LONG = torch.long
I32 = torch.int32

# face tables (local node indices) in the reference's row orders
TET_SHARED = [[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]]          # `:723-728`, `:675-680`
TET_SURFACE = [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]         # `:557-562`
TET_SURFACE_X = [3, 2, 1, 0]                                        # `:564-569`
TET_SHARED_X = [3, 2, 0, 1]                                         # `:682-687`
HEX = [[0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [0, 4, 7, 3], [0, 3, 2, 1], [4, 5, 6, 7]]   # `:1308-1315`
HEX_SURFACE_X = [2, 0, 0, 1, 4, 0]                                  # `:1317-1324`
HEX_AREA_X = [2, 0, 0, 1, 6, 0]                                     # `:1458`
WEDGE_QUAD = [[0, 1, 4, 3], [1, 2, 5, 4], [2, 0, 3, 5]]             # `:2249-2253`
WEDGE_QUAD_X = [2, 0, 1]
WEDGE_TRI = [[0, 2, 1], [3, 4, 5]]                                  # `:2260-2263`
WEDGE_TRI_X = [3, 0]
EDGES = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]            # `:2700-2704`
SPLIT = {8: [[0, 1, 3, 4], [1, 2, 3, 6], [1, 3, 4, 5], [3, 4, 5, 7], [3, 5, 6, 7], [3, 5, 6, 2]],   # `:1567-1574`
         6: [[0, 1, 2, 3], [1, 2, 3, 5], [1, 3, 4, 5]],                                            # `:2435-2439`
         10: [[0, 4, 6, 7], [4, 1, 5, 8], [6, 5, 2, 9], [7, 8, 9, 3], [4, 6, 7, 5], [6, 7, 9, 5],
              [4, 7, 8, 5], [5, 8, 7, 9]]}                                                        # `:976-985`


def _i32(tab):
    flat = [int(v) for row in tab for v in (row if isinstance(row, (list, tuple)) else [row])]
    return (ctypes.c_int32 * len(flat))(*flat)


def _dev(device):
    C.lib()
    return C.compute_device(device)


def _conn(elements, dev, npe_min):
    el = elements.to(device=dev, dtype=LONG).contiguous()
    if el.dim() != 2 or el.shape[1] < npe_min:
        raise ValueError(f"elements must be [M, >= {npe_min}], got {list(el.shape)}")
    n = int(el.max()) + 1 if el.numel() else 1
    _sys.check_connectivity(el, n)
    return el, n


class FaceGroups:
    """One fem_topo context: the faces of table `ftab` of every element, grouped by node set."""

    def __init__(self, elements, ftab, device):
        self.lib = C.lib()
        self.dev = _dev(device)
        self.el, self.N = _conn(elements, self.dev, max(max(r) for r in ftab) + 1)
        self.M, self.npe = self.el.shape
        self.F, self.fpn = len(ftab), len(ftab[0])
        self.h = ctypes.c_void_p()
        C.check(self.lib.fem_topo_create(C.ptr(self.el), self.M, self.npe, _i32(ftab), self.F, self.fpn, self.N,
                                         C.stream(self.dev), ctypes.byref(self.h)), "fem_topo_create")
        u, s, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        C.check(self.lib.fem_topo_counts(self.h, ctypes.byref(u), ctypes.byref(s), ctypes.byref(p)), "fem_topo_counts")
        self.n_unique, self.n_single, self.n_pair = u.value, s.value, p.value

    def pairs(self):
        out = torch.empty((self.n_pair, 2, 2), dtype=LONG, device=self.dev)
        C.check(self.lib.fem_topo_pairs(self.h, C.ptr(out)), "fem_topo_pairs")
        return out

    def unique(self):
        out = torch.empty((self.n_unique, self.fpn), dtype=LONG, device=self.dev)
        C.check(self.lib.fem_topo_unique(self.h, C.ptr(out)), "fem_topo_unique")
        return out

    def boundary(self, stab, smap, xtab=None):
        Fs = len(stab)
        k = ctypes.c_int64()
        C.check(self.lib.fem_topo_boundary(self.h, C.ptr(self.el), Fs, _i32(smap), _i32(stab),
                                           _i32(xtab) if xtab is not None else None, None, None, ctypes.byref(k)),
                "fem_topo_boundary")
        faces = torch.empty((k.value, self.fpn), dtype=LONG, device=self.dev)
        extra = torch.empty(k.value, dtype=LONG, device=self.dev)
        C.check(self.lib.fem_topo_boundary(self.h, C.ptr(self.el), Fs, _i32(smap), _i32(stab),
                                           _i32(xtab) if xtab is not None else None, C.ptr(faces), C.ptr(extra),
                                           ctypes.byref(k)), "fem_topo_boundary")
        return faces, extra

    def close(self):
        if self.h:
            self.lib.fem_topo_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _smap(stab, ftab):
    key = {tuple(sorted(r)): i for i, r in enumerate(ftab)}
    return [key[tuple(sorted(r))] for r in stab]


def _out(t, device):
    return t.to(torch.device(device))


# ---------------------------------------------------------------- surfaces
def compute_tetrahedral_surface_faces_with_fourth_node(elements, device="cuda:0"):
    """Faces of exactly one tet [K,3] (node order of the face table, face-major like the reference's cat) and
    the opposite node [K]. `solver/element.py:543-579`."""
    g = FaceGroups(elements, TET_SHARED, device)
    f, x = g.boundary(TET_SURFACE, _smap(TET_SURFACE, TET_SHARED), TET_SURFACE_X)
    g.close()
    return _out(f, device), _out(x, device)


def compute_hexahedral_surface_faces_with_extra_node(elements, device="cuda:0"):
    """Faces of exactly one hex [K,4] and a node off the face [K]. `solver/element.py:1293-1334`."""
    g = FaceGroups(elements, HEX, device)
    f, x = g.boundary(HEX, list(range(6)), HEX_SURFACE_X)
    g.close()
    return _out(f, device), _out(x, device)


def compute_wedge_surface_faces_with_extra_node(elements, device="cuda:0"):
    """([quad faces [Kq,4], tri faces [Kt,3]], [quad extra [Kq], tri extra [Kt]]); quads and triangles grouped
    separately like the reference. `solver/element.py:2234-2283`."""
    gq = FaceGroups(elements, WEDGE_QUAD, device)
    fq, xq = gq.boundary(WEDGE_QUAD, list(range(3)), WEDGE_QUAD_X)
    gq.close()
    gt = FaceGroups(elements, WEDGE_TRI, device)
    ft, xt = gt.boundary(WEDGE_TRI, list(range(2)), WEDGE_TRI_X)
    gt.close()
    return [_out(fq, device), _out(ft, device)], [_out(xq, device), _out(xt, device)]


def _surface_normals(coords, faces, extra, v2, device, dtype):
    lib = C.lib()
    dev = _dev(device)
    X = coords.to(device=dev, dtype=F64).contiguous()
    f = faces.to(device=dev, dtype=LONG).contiguous()
    x = extra.to(device=dev, dtype=LONG).contiguous()
    K, fpn = f.shape
    out = torch.empty((K, 3), dtype=F64, device=dev)
    C.check(lib.fem_surface_normals(C.ptr(X), C.ptr(f), C.ptr(x), K, fpn, v2, C.ptr(out), C.stream(dev)),
            "fem_surface_normals")
    return out.to(device=torch.device(device), dtype=dtype)


def compute_tetrahdral_surface_normals(coords, elements, device="cuda:0", dtype=torch.float32):
    """Outward unit normals of the tet surface faces [K,3] (the reference's spelling). `solver/element.py:581-619`."""
    f, x = compute_tetrahedral_surface_faces_with_fourth_node(elements, device=_dev(device))
    return _surface_normals(coords, f, x, 2, device, dtype)


compute_tetrahedral_surface_normals = compute_tetrahdral_surface_normals


def compute_hexahedral_surface_normals(coords, elements, device="cuda:0", dtype=torch.float32):
    """Outward unit normals of the hex surface faces [K,3] (edges p2-p1, p3-p1). `solver/element.py:1336-1374`."""
    f, x = compute_hexahedral_surface_faces_with_extra_node(elements, device=_dev(device))
    return _surface_normals(coords, f, x, 2, device, dtype)


def compute_wedge_surface_normals(coords, elements, device="cuda:0", dtype=torch.float32):
    """[quad normals [Kq,3] (edges p2-p1, p4-p1), tri normals [Kt,3]]. `solver/element.py:2285-2338`."""
    (fq, ft), (xq, xt) = compute_wedge_surface_faces_with_extra_node(elements, device=_dev(device))
    return [_surface_normals(coords, fq, xq, 3, device, dtype), _surface_normals(coords, ft, xt, 2, device, dtype)]


# ---------------------------------------------------------------- per-element face normals
def _element_normals(coords, elements, edges, cen, extra, scale, flip, unit, npe_min, device, dtype):
    lib = C.lib()
    dev = _dev(device)
    X = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    if el.dim() != 2 or el.shape[1] < npe_min:
        raise ValueError(f"elements must be [M, >= {npe_min}], got {list(el.shape)}")
    _sys.check_connectivity(el, X.shape[0])
    M, npe = el.shape
    F = len(edges)
    cen_pad = [list(r) + [0] * (4 - len(r)) for r in cen]
    out = torch.empty((M, F, 3), dtype=F64, device=dev)
    C.check(lib.fem_element_face_normals(C.ptr(X), C.ptr(el), M, npe, _i32(edges), _i32(cen_pad),
                                         _i32([len(r) for r in cen]), _i32(extra), F, float(scale), int(flip),
                                         int(unit), C.ptr(out), C.stream(dev)), "fem_element_face_normals")
    return out.to(device=torch.device(device), dtype=dtype)


def compute_tetrahedral_normals_and_area(coords, elements, device="cuda:0", dtype=torch.float32):
    """Area-weighted outward face normals [M,4,3] (faces 012, 013, 123, 023). `solver/element.py:652-705`."""
    edges = [[r[0], r[1], r[2]] for r in TET_SHARED]
    return _element_normals(coords, elements, edges, TET_SHARED, TET_SHARED_X, 0.5, True, False, 4, device, dtype)


def compute_hexahedral_normals_and_area(coords, elements, device="cuda:0", dtype=torch.float32):
    """Outward face normals (p1-p0) x (p3-p0) [M,6,3]. `solver/element.py:1418-1472`."""
    edges = [[r[0], r[1], r[3]] for r in HEX]
    return _element_normals(coords, elements, edges, HEX, HEX_AREA_X, 1.0, True, False, 8, device, dtype)


def compute_wedge_normals_and_area(coords, elements, device="cuda:0", dtype=torch.float32):
    """Unit face normals [M,5,3], three quads then two triangles, not oriented. `solver/element.py:2377-2422`."""
    edges = [[r[0], r[1], r[3]] for r in WEDGE_QUAD] + [[r[0], r[1], r[2]] for r in WEDGE_TRI]
    return _element_normals(coords, elements, edges, [[0]] * 5, [0] * 5, 1.0, False, True, 6, device, dtype)


# ---------------------------------------------------------------- shared faces / element graph / edges
def identify_tetrahedral_shared_faces(elements, device="cuda:0"):
    """[S,2,2] ((element, face), (element, face)) for every face shared by exactly two tets, in lexicographic
    order of the sorted face nodes (faces 012, 013, 123, 023). `solver/element.py:707-762`. Inside a pair the
    lower (element, face) comes first; the reference leaves that order to an unstable sort (`:748`)."""
    g = FaceGroups(elements, TET_SHARED, device)
    out = g.pairs()
    g.close()
    return _out(out, device)


def identify_hexahedral_shared_faces(elements, device="cuda:0"):
    """Hex analogue of identify_tetrahedral_shared_faces (6 faces). `solver/element.py:1474-1532`."""
    g = FaceGroups(elements, HEX, device)
    out = g.pairs()
    g.close()
    return _out(out, device)


def element_adjacency(elements, device="cuda:0"):
    """Element graph of the shared faces as CSR (rowptr [M+1] int64, cols int64, neighbours ascending): the
    coalesced symmetric adjacency `subdivision.ipynb` builds (`build_adjacency_matrix`, cell 9) for its
    partitioner. Tets (4 nodes) or hexes (8 nodes)."""
    el = elements
    npe = el.shape[1]
    pairs = (identify_tetrahedral_shared_faces if npe in (4, 10) else identify_hexahedral_shared_faces)(
        el, device=_dev(device))
    M = el.shape[0]
    a, b = pairs[:, 0, 0], pairs[:, 1, 0]
    src = torch.cat([a, b])
    dst = torch.cat([b, a])
    key = src * M + dst
    key = torch.unique(key)            # coalesce (sorted)
    rows, cols = key // M, key % M
    rowptr = torch.zeros(M + 1, dtype=LONG, device=key.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=M), 0)
    return _out(rowptr, device), _out(cols, device)


def element_to_edge(elements, device="cuda:0"):
    """Unique node edges [2,E] of tets (6 per element), columns in lexicographic order.
    `solver/element.py:2687-2713`."""
    g = FaceGroups(elements, EDGES, device)
    out = g.unique()
    g.close()
    return _out(out.t(), device)


# ---------------------------------------------------------------- element splits
def _split(elements, npe, device):
    lib = C.lib()
    dev = _dev(device)
    el = elements.to(device=dev, dtype=LONG).contiguous()
    if el.dim() != 2 or el.shape[1] != npe:
        raise ValueError(f"expected [M, {npe}] connectivity, got {list(el.shape)}")
    tab = SPLIT[npe]
    M = el.shape[0]
    out = torch.empty((M * len(tab), 4), dtype=LONG, device=dev)
    C.check(lib.fem_sub_elements(C.ptr(el), M, npe, _i32(tab), len(tab), 4, C.ptr(out), C.stream(dev)),
            "fem_sub_elements")
    return _out(out, device)


def c3d8_to_c3d4(c3d8_elements, device="cuda:0"):
    """[6M, 4] tets of every hex. `solver/element.py:1555-1581`."""
    return _split(c3d8_elements, 8, device)


def c3d6_to_c3d4(element, device="cuda:0"):
    """[3M, 4] tets of every wedge. `solver/element.py:2424-2446`."""
    return _split(element, 6, device)


def c3d10_to_c3d4(c3d10_elements, device="cuda:0"):
    """[8M, 4] linear tets of every quadratic tet. `solver/element.py:963-993`."""
    return _split(c3d10_elements, 10, device)


def to_c3d4(elements, device="cuda:0"):
    """Dispatch on nodes per element (`solver/element.py:355-364`; c3d20 out of scope -> None like an
    unmatched width)."""
    n = elements.shape[1]
    if n in SPLIT:
        return _split(elements, n, device)
    return None


# ---------------------------------------------------------------- mid-edge nodes, uniform refinement (csrc/refine.hip)
TET10_WALK = [[0, 1], [1, 2], [2, 0], [0, 3], [1, 3], [2, 3]]   # edges of c3d10 nodes 4..9, `:826-831`


def _mid_edges(el, dev, first_encounter):
    """(unique edges [E, 2] lexicographic, eid [6 M] int32: the edge of slot 6 e + k of TET10_WALK, mid_id [E]: the
    rank of the edge among the mid nodes -- by the lowest slot naming it (the reference's first-encounter order) or
    the sorted-edge order)."""
    lib = C.lib()
    g = FaceGroups(el, EDGES, dev)
    ue = g.unique().contiguous()
    g.close()
    M, E = el.shape[0], ue.shape[0]
    eid = torch.empty(6 * M, dtype=I32, device=dev)
    minslot = torch.full((E,), torch.iinfo(torch.int64).max, dtype=LONG, device=dev)
    C.check(lib.fem_refine_edge_slots(C.ptr(el), M, C.ptr(ue), E, C.ptr(eid), C.ptr(minslot), C.stream(dev)),
            "fem_refine_edge_slots")
    if M and int(eid.min()) < 0:
        raise ValueError("c3d4 mid-edge nodes: an element edge is missing from the mesh's edge list")
    mid_id = torch.arange(E, dtype=LONG, device=dev)
    if first_encounter:
        order = torch.argsort(minslot)   # the slots are distinct
        mid_id = torch.empty_like(order)
        mid_id[order] = torch.arange(E, dtype=LONG, device=dev)
    return ue, eid, mid_id


def _elevate(X, el, dev, first_encounter):
    """c3d4 -> c3d10 on the device: (coords [N + E, 3] fp64, c3d10 connectivity [M, 10], parents [N + E, 2] int32,
    unique edges, mid_id)."""
    lib = C.lib()
    N, M = X.shape[0], el.shape[0]
    _sys.check_connectivity(el, N)
    ue, eid, mid_id = _mid_edges(el, dev, first_encounter)
    E = ue.shape[0]
    if N + E > torch.iinfo(torch.int32).max:
        raise ValueError(f"c3d4 mid-edge nodes: {N + E} nodes do not fit int32 ids")
    el10 = torch.empty((M, 10), dtype=LONG, device=dev)
    C.check(lib.fem_refine_emit(C.ptr(el), M, N, C.ptr(eid), C.ptr(mid_id), C.ptr(el10), C.stream(dev)),
            "fem_refine_emit")
    Xo = torch.empty((N + E, 3), dtype=F64, device=dev)
    parents = torch.empty((N + E, 2), dtype=I32, device=dev)
    C.check(lib.fem_refine_nodes(C.ptr(X), N, C.ptr(ue), E, C.ptr(mid_id), C.ptr(Xo), C.ptr(parents), C.stream(dev)),
            "fem_refine_nodes")
    return Xo, el10, parents, ue, mid_id


def _node_set(ids, N, dev):
    """bool [N] mask of a node id list; IndexError for an id outside [0, N) (checked on the host: an index kernel
    must never see one)."""
    ids = torch.as_tensor(ids).to(device=dev, dtype=LONG).view(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise IndexError(f"node ids must be in [0, {N})")
    inside = torch.zeros(N, dtype=torch.bool, device=dev)
    inside[ids] = True
    return inside


def _carry_ids(ids, N, ue, mid_id, dev):
    """A node set after the elevation: its nodes plus every mid node with both ends in it, sorted (`:817-820`)."""
    if ids is None:
        return torch.empty(0, dtype=LONG, device=dev)
    inside = _node_set(ids, N, dev)
    both = inside[ue[:, 0]] & inside[ue[:, 1]]
    return torch.sort(torch.cat([torch.nonzero(inside).view(-1), N + mid_id[both]])).values


def c3d4_to_c3d10(coords, elements, rbe2_ids=None, rbe3_ids=None, dtype=torch.float32, device="cuda:0"):
    """Quadratic tets from linear ones (`solver/element.py:777-833`): (coords [N + E, 3] in `dtype`, connectivity
    [M, 10] int32, rbe2 ids, rbe3 ids int32). Mid-edge nodes follow the corner nodes in first-encounter order of the
    walk element by element over edges (0,1), (1,2), (2,0), (0,3), (1,3), (2,3); a mid node joins a set when both ends
    are in it (the sets come back sorted; the reference returns them in hash order). A mid coordinate is
    (cA + cB) / 2 evaluated in fp64 and rounded once to `dtype`, as the reference's Python floats are -- for coordinates
    already in `dtype` that is the sum evaluated in `dtype`."""
    dev = _dev(device)
    X = coords.to(device=dev, dtype=F64).contiguous()
    el = elements.to(device=dev, dtype=LONG).contiguous()
    if el.dim() != 2 or el.shape[1] != 4 or X.dim() != 2 or X.shape[1] != 3:
        raise ValueError(f"c3d4_to_c3d10: coords [N, 3] and elements [M, 4] are needed, got {list(X.shape)} and "
                         f"{list(el.shape)}")
    Xo, el10, _, ue, mid_id = _elevate(X, el, dev, True)
    N = X.shape[0]
    r2, r3 = (_carry_ids(ids, N, ue, mid_id, dev).to(I32) for ids in (rbe2_ids, rbe3_ids))
    return (_out(Xo.to(dtype), device), _out(el10.to(I32), device), _out(r2, device), _out(r3, device))


def refinement_table():
    """The 8-child table of the uniform (red) refinement: SPLIT[10] with every child oriented like its parent. The
    orientation of the children of the unit tet is checked here, on the host; a child the table leaves negative gets
    its last two nodes exchanged in the copy returned (SPLIT itself is not touched)."""
    c = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F64)
    x = torch.cat([c, torch.stack([0.5 * (c[a] + c[b]) for a, b in TET10_WALK])])
    tab = [list(r) for r in SPLIT[10]]
    for row in tab:
        p = x[row]
        if float(torch.linalg.det(p[1:] - p[0])) < 0:
            row[2], row[3] = row[3], row[2]
    return tab


class MeshLevel:
    """One level of a MeshHierarchy: coords [N, 3] fp64, elements [M, 4] int64, parents [N, 2] int32 (ids of the level
    below in its numbering, a == b for a carried-over node; None on level 0) and perm [N] (the level's node k is node
    perm[k] of the numbering reorder=None gives; None when the level was not renumbered)."""

    def __init__(self, coords, elements, parents=None, perm=None):
        self.coords, self.elements, self.parents, self.perm = coords, elements, parents, perm

    @property
    def n_nodes(self):
        return int(self.coords.shape[0])


class MeshHierarchy:
    """Nested c3d4 meshes from refine_c3d4: `levels[0]` the caller's mesh, `levels[-1]` the finest."""

    def __init__(self, levels, reorder):
        self.levels, self.reorder = levels, reorder
        self.device = levels[0].coords.device

    def __len__(self):
        return len(self.levels)

    @property
    def fine(self):
        last = self.levels[-1]
        return last.coords, last.elements

    def carry(self, node_ids, level=None):
        """A node set of level 0 carried to `level` (default: the finest): a node of level l + 1 is in the set when
        both its parents are (a carried-over node: when the node itself is). Sorted int64 ids."""
        level = len(self.levels) - 1 if level is None else int(level)
        if not 0 <= level < len(self.levels):
            raise ValueError(f"MeshHierarchy.carry: level {level} of {len(self.levels)}")
        with C.device_scope(self.device):
            inside = _node_set(node_ids, self.levels[0].n_nodes, self.device)
            for lv in self.levels[1:level + 1]:
                p = lv.parents.long()
                inside = inside[p[:, 0]] & inside[p[:, 1]]
            return torch.nonzero(inside).view(-1)


def refine_c3d4(coords, elements, levels=1, reorder="rcm", device=None):
    """Uniform (red) refinement of a c3d4 mesh, `levels` times -> MeshHierarchy. Level l + 1 is the c3d10 elevation of
    level l split by refinement_table() (four corner tets, the inner octahedron cut along mid(1,2)-mid(0,3)); the
    coordinates are fp64 and a mid node is one rounded 0.5 (a + b). reorder="rcm" (default) renumbers every refined
    level with system.rcm_order -- appended mid nodes would push the fine matrix off the 16-bit column-delta SELL path
    -- and `parents` absorbs the permutation; reorder=None keeps the corner nodes first and the mid nodes in
    sorted-edge order. `device`: default the coordinates' device when that is a HIP device, else the current one."""
    if reorder not in (None, "rcm"):
        raise ValueError(f"unknown reorder {reorder!r} (supported: 'rcm', None)")
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"refine_c3d4: levels must be >= 1, got {levels}")
    dev = _dev(device if device is not None else coords.device)
    with C.device_scope(dev):
        lib = C.lib()
        X = coords.to(device=dev, dtype=F64).contiguous()
        el = elements.to(device=dev, dtype=LONG).contiguous()
        if el.dim() != 2 or el.shape[1] != 4 or X.dim() != 2 or X.shape[1] != 3:
            raise ValueError(f"refine_c3d4: coords [N, 3] and elements [M, 4] are needed, got {list(X.shape)} and "
                             f"{list(el.shape)}")
        tab = _i32(refinement_table())
        out = [MeshLevel(X, el)]
        for _ in range(levels):
            Xo, el10, parents, _, _ = _elevate(X, el, dev, False)
            M = el10.shape[0]
            fine = torch.empty((8 * M, 4), dtype=LONG, device=dev)
            C.check(lib.fem_sub_elements(C.ptr(el10), M, 10, tab, 8, 4, C.ptr(fine), C.stream(dev)),
                    "fem_sub_elements")
            perm = None
            if reorder == "rcm":
                perm, inv = _sys.rcm_order(fine, Xo.shape[0])
                Xo, fine = _sys.renumber(Xo, fine, perm, inv)
                Xo, fine, parents = Xo.contiguous(), fine.contiguous(), parents[perm].contiguous()
            out.append(MeshLevel(Xo, fine, parents, perm))
            X, el = Xo, fine
        return MeshHierarchy(out, reorder)


__all__ = [
    "c3d4_to_c3d10", "refine_c3d4", "refinement_table", "MeshHierarchy", "MeshLevel",
    "compute_tetrahedral_surface_faces_with_fourth_node", "compute_hexahedral_surface_faces_with_extra_node",
    "compute_wedge_surface_faces_with_extra_node", "compute_tetrahdral_surface_normals",
    "compute_tetrahedral_surface_normals", "compute_hexahedral_surface_normals", "compute_wedge_surface_normals",
    "compute_tetrahedral_normals_and_area", "compute_hexahedral_normals_and_area", "compute_wedge_normals_and_area",
    "identify_tetrahedral_shared_faces", "identify_hexahedral_shared_faces", "element_adjacency", "element_to_edge",
    "c3d8_to_c3d4", "c3d6_to_c3d4", "c3d10_to_c3d4", "to_c3d4", "FaceGroups",
]

# every public function runs in the scope of the device its `device` argument names (_capi.on_device)
C.scope_module(globals())
