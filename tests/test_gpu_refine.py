"""GPU tier: mid-edge nodes and uniform refinement of c3d4 meshes (csrc/refine.hip, topology.c3d4_to_c3d10 /
refine_c3d4 / MeshHierarchy) against the restatement of tests/multigrid_ref.py and the reference's own output
(tests/golden/c3d4_to_c3d10.npz, tools/gen_golden_c3d10.py). Everything here is bit-exact: integer tables, and
coordinates that are one rounded 0.5 (a + b)."""
import pytest
import torch

import multigrid_ref as MG
from conftest import load_golden
from twolevel_ref import kuhn_box

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _mods():
    import fem355  # noqa: F401
    from fem355 import mesh, topology
    return mesh, topology


def _mesh(name):
    mesh, _ = _mods()
    if name == "cube2":
        return mesh.kuhn_cube(2, 0.15)
    if name == "shuffled":
        g = load_golden("c3d4_to_c3d10")
        return g["coords"], g["elements"]
    if name == "single":
        return (torch.tensor([[0.1, 0.2, 0.0], [1.3, 0.1, 0.2], [0.2, 1.1, 0.1], [0.3, 0.2, 0.9]], dtype=F64),
                torch.tensor([[0, 1, 2, 3]]))
    return kuhn_box(2, 2, 6, (1.0, 1.0, 3.0), 0.15)


SHAPES = ["cube2", "shuffled", "single", "beam"]


@pytest.mark.parametrize("name", SHAPES)
def test_refinement_and_parents_vs_restatement(gpu, name):
    _, topology = _mods()
    c, t = _mesh(name)
    h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=2, reorder=None)
    ref = MG.hierarchy_ref(c, t, 2)
    assert len(h) == 3 and h.levels[0].parents is None
    for lv, (rc, rt, rp) in zip(h.levels, ref):
        assert lv.coords.dtype == F64 and lv.elements.dtype == torch.long
        assert torch.equal(lv.elements.cpu(), rt)
        assert torch.equal(lv.coords.cpu(), rc)
        if rp is not None:
            assert lv.parents.dtype == torch.int32 and torch.equal(lv.parents.cpu().long(), rp)
    fc, fe = h.fine
    assert fc is h.levels[-1].coords and fe is h.levels[-1].elements
    assert topology.refinement_table() == MG.split_table()
    assert topology.SPLIT[10] == MG.CHILDREN   # the reference's table itself is untouched


def test_c3d4_to_c3d10_against_the_reference_output(gpu):
    _, topology = _mods()
    g = load_golden("c3d4_to_c3d10")
    nc, ne, r2, r3 = topology.c3d4_to_c3d10(g["coords"], g["elements"], g["rbe2"], g["rbe3"], dtype=torch.float32,
                                            device=gpu)
    assert nc.dtype == torch.float32 and ne.dtype == torch.int32 and r2.dtype == r3.dtype == torch.int32
    assert torch.equal(ne.cpu(), g["new_elements"])
    assert torch.equal(nc.cpu(), g["new_coords"])
    assert set(r2.cpu().tolist()) == set(g["new_rbe2"].tolist())
    assert set(r3.cpu().tolist()) == set(g["new_rbe3"].tolist())
    assert torch.equal(r2.cpu(), torch.sort(r2.cpu()).values)
    # the restatement's first-encounter numbering is the reference's too
    rc, re10, _, _ = MG.elevate_ref(g["coords"], g["elements"], True)
    assert torch.equal(re10.int(), g["new_elements"]) and torch.equal(rc.float(), g["new_coords"])
    nc2, ne2, e2, e3 = topology.c3d4_to_c3d10(g["coords"], g["elements"], device=gpu)
    assert torch.equal(ne2, ne) and torch.equal(nc2, nc) and e2.numel() == 0 and e3.numel() == 0


@pytest.mark.parametrize("name", ["cube2", "shuffled", "beam"])
def test_rcm_hierarchy_is_the_same_mesh_up_to_its_permutation(gpu, name):
    _, topology = _mods()
    c, t = _mesh(name)
    hr = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=2)
    hn = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=2, reorder=None)
    assert hr.reorder == "rcm" and hn.reorder is None
    for l in (1, 2):
        lo, lv = hr.levels[l - 1], hr.levels[l]
        perm = lv.perm.cpu()
        assert torch.equal(torch.sort(perm).values, torch.arange(lv.n_nodes))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        # undoing the stored permutation gives the plain refinement of the level below
        rc, rt, rp = MG.refine_ref(lo.coords.cpu(), lo.elements.cpu())
        assert torch.equal(lv.coords.cpu(), rc[perm])
        assert torch.equal(lv.elements.cpu(), inv[rt])
        assert torch.equal(lv.parents.cpu().long(), rp[perm])
        # and the nodes are those of the hierarchy that was never renumbered
        a, b = lv.coords.cpu(), hn.levels[l].coords.cpu()
        assert torch.equal(torch.unique(a, dim=0), torch.unique(b, dim=0))
        assert lv.elements.shape == hn.levels[l].elements.shape
    if name == "cube2":   # level 1 of both comes from the same level 0: the permutation maps one onto the other
        perm = hr.levels[1].perm
        assert torch.equal(hr.levels[1].coords, hn.levels[1].coords[perm])
        assert torch.equal(perm[hr.levels[1].elements], hn.levels[1].elements)


@pytest.mark.parametrize("reorder", [None, "rcm"])
def test_carry_follows_the_both_ends_rule(gpu, reorder):
    mesh, topology = _mods()
    c, t = _mesh("cube2")
    h = topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=2, reorder=reorder)
    host = [(lv.coords.cpu(), lv.elements.cpu(), None if lv.parents is None else lv.parents.cpu().long())
            for lv in h.levels]
    ids = mesh.face_nodes(c, 2, 0.0)
    for level in (0, 1, 2):
        got = h.carry(ids, level).cpu()
        assert torch.equal(got, MG.carry_ref(ids, host, level))
        # the clamped face of the coarse mesh is the clamped face of every level
        assert torch.equal(got, mesh.face_nodes(host[level][0], 2, 0.0))
    assert torch.equal(h.carry(ids), h.carry(ids, 2))
    scattered = torch.tensor([0, 5, 13])   # no edge has both ends in it ... unless the mesh says so: ask the rule
    assert torch.equal(h.carry(scattered, 1).cpu(), MG.carry_ref(scattered, host, 1))
    with pytest.raises(ValueError):
        h.carry(ids, 3)
    with pytest.raises(ValueError):
        topology.refine_c3d4(c.to(gpu), t.to(gpu), levels=0)
    with pytest.raises(ValueError):
        topology.refine_c3d4(c.to(gpu), t.to(gpu), reorder="amd")
