#!/usr/bin/env python3
"""Generate tests/golden/c3d4_to_c3d10.npz by running the reference's own c3d4_to_c3d10 on the host.

    python tools/gen_golden_c3d10.py /path/to/reference/solver

Input: the jittered 48-tet Kuhn cube with the element order shuffled and the nodes renumbered by a permutation, an
rbe2 and an rbe3 node set. Output: what the reference function returns (coordinates in float32, connectivity, the two
sets sorted -- the reference hands them back in hash order). Only these arrays are stored; nothing of the reference is
copied. Modules the reference imports that are not installed are replaced by empty stubs (its VTK loader alone uses
them). The reference function walks a module-level name `elems` that it never binds (SURVEY lists the function as
failing for that reason); the generator binds that name to the connectivity it passes."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import fem355  # noqa: E402,F401
from fem355 import mesh  # noqa: E402


def load_module(path):
    sys.dont_write_bytecode = True
    for _ in range(16):
        spec = importlib.util.spec_from_file_location("reference_element", path)
        mod = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(mod)
            return mod
        except ModuleNotFoundError as e:
            sys.modules[e.name] = types.ModuleType(e.name)
    raise RuntimeError(f"could not import {path}")


def case():
    coords, tets = mesh.kuhn_cube(2, 0.15)
    g = torch.Generator().manual_seed(20240611)
    node_perm = torch.randperm(coords.shape[0], generator=g)      # new node k is old node node_perm[k]
    inv = torch.empty_like(node_perm)
    inv[node_perm] = torch.arange(coords.shape[0])
    coords, tets = coords[node_perm], inv[tets]
    tets = tets[torch.randperm(tets.shape[0], generator=g)].contiguous()
    rbe2 = inv[mesh.face_nodes(mesh.kuhn_cube(2, 0.15)[0], 2, 0.0)]   # the z = 0 face
    rbe3 = inv[mesh.face_nodes(mesh.kuhn_cube(2, 0.15)[0], 0, 1.0)]   # the x = 1 face
    return coords, tets, rbe2, rbe3


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = load_module(os.path.join(sys.argv[1], "element.py"))
    coords, tets, rbe2, rbe3 = case()
    mod.elems = tets
    nc, ne, n2, n3 = mod.c3d4_to_c3d10(coords, tets, rbe2, rbe3, dtype=torch.float32)
    out = os.path.join(ROOT, "tests", "golden", "c3d4_to_c3d10.npz")
    np.savez_compressed(out, coords=coords.numpy(), elements=tets.numpy(), rbe2=rbe2.numpy(), rbe3=rbe3.numpy(),
                        new_coords=nc.numpy(), new_elements=ne.numpy(), new_rbe2=np.sort(n2.numpy()),
                        new_rbe3=np.sort(n3.numpy()))
    print(f"{out}: {os.path.getsize(out)} bytes, {nc.shape[0]} nodes, {ne.shape[0]} elements, "
          f"{n2.numel()} / {n3.numel()} set nodes")


if __name__ == "__main__":
    main()
