"""fem355 — MI355X-native (gfx950) FEM assembly + Jacobi-PCG.

Drop-in for the hot path of sml2004/CUDA-powered-mesh-handling-and-Iterative-solvers: the `element.py`
element stiffness quadrature and the `solver.py` CG / PCG loops, re-implemented as hand-written HIP
kernels behind a C-ABI (`include/fem355.h`, loaded by `_capi.py`). See DESIGN.md.
"""
import os as _os

PKG_DIR = _os.path.dirname(_os.path.abspath(__file__))

from . import mesh  # noqa: E402,F401  (pure torch, no GPU needed)

# the multigrid interface, resolved on first use (the submodules load the HIP library's binding)
_LAZY = {"c3d4_to_c3d10": "topology", "refine_c3d4": "topology", "MeshHierarchy": "topology",
         "Multigrid": "system", "multigrid_pcg_solver": "solver"}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["mesh", "PKG_DIR", *_LAZY]
