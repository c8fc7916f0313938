"""Device-resident global operator: pattern build, assembly into SELL-64, SpMV and the (P)CG driver.

This is the host runtime around the HIP kernels: it allocates device buffers with torch (plumbing only),
calls the C-ABI on the current HIP stream, and owns nothing the kernels compute. The reference has no
assembled operator (it is element-by-element, `solver/element.py:429-464`); the assembled matrix here is
the coalesced COO of `subdivision.ipynb:118-139`, so `A @ p == compute_nodal_forces(K, elements, p)`.
"""
from __future__ import annotations

import ctypes
import math
import os
import time
from dataclasses import dataclass

import torch

try:
    from . import _capi as C
except ImportError:  # pragma: no cover - flat import from the package directory (`import solver`)
    import _capi as C  # type: ignore

I32, I64, F64 = torch.int32, torch.int64, torch.float64


def _scoped(cls):
    """Class decorator: every public method (and __init__) runs with the current HIP device set to the object's
    device (`self.device`, or for __init__ the device of the first tensor argument's matrix), so the library's
    allocations and null-stream launches land where the tensors live (`_capi.device_scope`)."""
    import functools

    def wrap(fn):
        @functools.wraps(fn)
        def w(self, *args, **kwargs):
            dev = getattr(self, "device", None)
            if dev is None:   # __init__: SellMatrix(graph, bs) / PcgRunner(A, ...)
                a0 = args[0] if args else None
                dev = getattr(a0, "device", None) or getattr(getattr(a0, "cols", None), "device", None)
            if dev is None or not torch.cuda.is_available():
                return fn(self, *args, **kwargs)
            with C.device_scope(dev):
                return fn(self, *args, **kwargs)
        return w

    for name, fn in list(vars(cls).items()):
        if callable(fn) and (name == "__init__" or not name.startswith("_")) and not isinstance(fn, (staticmethod,
                                                                                                    classmethod, property)):
            setattr(cls, name, wrap(fn))
    return cls


def _dev_scalar(dev, dtype, value):
    return torch.full((1,), value, dtype=dtype, device=dev)


# (P)CG kernel schedules (csrc/pcg.hip): 0 = three kernels with in-kernel grid reductions, 1 = fused (p formed
# inside the SpMV), 2 = deferred (partials summed by the next kernel, no grid atomics), 3 = persistent (one
# cooperative launch per chunk of single-reduction iterations, csrc/pcg_persist.hpp; falls back to 2 where its
# prerequisites do not hold)
SCHED_THREE, SCHED_FUSED, SCHED_DEFERRED, SCHED_PERSIST, SCHED_AUTO = 0, 1, 2, 3, 4
# measured on MI355X (10M-tet cube, 16-bit columns, paired layout; tools/persist_check.py, tools/spmv_tune.py):
# scalar Poisson 44.0 us/it persistent vs 79.4 deferred; 3x3 elasticity: the bs = 3 persistent kernel while the state
# fits on chip (1.2M tets: 43.8 vs 63.2 us three-kernel), the three-kernel schedule past that (10M: 436 vs 633 us for
# the overflow build) -- SCHED_AUTO picks per matrix
DEFAULT_SCHEDULE = {1: SCHED_PERSIST, 3: SCHED_AUTO}


def _schedule(fused, schedule, bs=1):
    if schedule is not None:
        return int(schedule)
    return SCHED_FUSED if fused else DEFAULT_SCHEDULE.get(bs, SCHED_THREE)


@dataclass
class PcgResult:
    x: torch.Tensor
    iterations: int      # the reference's reported count (i+1 at the stop)
    status: int          # _capi.PCG_*
    rz: float            # last r.z (r.r in CG mode) — the "Residual norm" the reference prints (squared)
    pq: float            # last p.Ap (printed on breakdown)
    history: torch.Tensor = None
    schedule: int = -1   # the kernel schedule the solve ran (SCHED_*; after any fallback)


# multi-load-case kernels (csrc/pcg_multi.hip): the column counts they are built for, and the most columns one pass
# takes per block size. bs = 3 runs in passes of 4: measured on the 10M-tet elastic matrix, the 8-column SpMM takes
# 1514 us against 2 x 489 us for two 4-column ones (its gather window of 192 bytes per block column no longer fits the
# L2 of an XCD; DESIGN.md, profiles/multi_rhs_n119_wide8.json). `max_cols=8` selects the wide pass all the same.
MULTI_NV = (2, 4, 8)
MULTI_MAX = {1: 8, 3: 4}


def multi_passes(L: int, bs: int = 1, max_cols: int = None):
    """Split L right-hand sides into lock-step passes: [(first column, columns, NV)] with at most `max_cols` columns
    per pass (default MULTI_MAX[bs]) and NV the next instantiated column count (the pass is padded with NV - columns
    zero columns): 11 -> [(0, 8, 8), (8, 3, 4)] for bs = 1, [(0, 4, 4), (4, 4, 4), (8, 3, 4)] for bs = 3."""
    if L < 1:
        raise ValueError(f"at least one right-hand side is needed, got {L}")
    width = MULTI_MAX.get(bs, MULTI_NV[-1]) if max_cols is None else int(max_cols)
    if not 1 <= width <= MULTI_NV[-1]:
        raise ValueError(f"a pass takes 1 to {MULTI_NV[-1]} columns, got {width}")
    out, j = [], 0
    while j < L:
        k = min(width, L - j)
        out.append((j, k, next(v for v in MULTI_NV if v >= k)))
        j += k
    return out


@dataclass
class MultiPcgResult:
    """SellMatrix.pcg_multi: the PcgResult fields per load case (column j of x, entry j of the lists)."""
    x: torch.Tensor          # [n, L]
    iterations: list         # [L] the reference's reported count per column
    status: list             # [L] _capi.PCG_*
    rz: list                 # [L] last r.z (r.r in CG mode)
    pq: list                 # [L] last p.Ap
    history: torch.Tensor = None   # [max(iterations), L]; rows past a column's own stop are NaN

    def column(self, j: int) -> PcgResult:
        """Load case j as the PcgResult a single solve returns."""
        hist = None
        if self.history is not None:
            hist = self.history[: min(self.iterations[j], self.history.shape[0]), j]
        return PcgResult(self.x[:, j], self.iterations[j], self.status[j], self.rz[j], self.pq[j], hist)


@dataclass
class ModalResult:
    """SellMatrix.eig_lowest: the k lowest eigenpairs of K u = lambda M u on the free dofs."""
    lam: torch.Tensor              # [k] ascending (host, fp64)
    X: torch.Tensor                # [n, k] M-orthonormal, zeros on the fixed dofs (device)
    iterations: int                # LOBPCG iterations (rotations of the basis) made
    status: int                    # _capi.PCG_CONVERGED / PCG_MAXITER / PCG_BREAKDOWN
    residuals: torch.Tensor        # [k] ||K x - lam M x|| / (lam ||M x||) over the free dofs, as last measured
    restarts: int = 0              # iterations whose Rayleigh-Ritz dropped P
    history: torch.Tensor = None   # [iterations, k]: the residuals after every iteration


@dataclass
class BucklingResult:
    """SellMatrix.buckling_lowest: the k pairs of largest |theta| of G phi = theta K phi on the free dofs, i.e. the k
    load factors lambda = -1 / theta of smallest magnitude of (K + lambda K_g) phi = 0."""
    factors: torch.Tensor          # [k] signed lambda, ascending in |lambda| (host, fp64)
    theta: torch.Tensor            # [k] the Ritz values, descending in |theta| (host, fp64)
    X: torch.Tensor                # [n, k] K-orthonormal, zeros on the fixed dofs (device)
    iterations: int                # outer iterations (block solves with K) made
    linear_iterations: int         # the inner PCG iterations, summed over the solves (per solve: the slowest column)
    status: int                    # _capi.PCG_CONVERGED / PCG_MAXITER / PCG_BREAKDOWN
    residuals: torch.Tensor        # [k] ||G x - theta K x|| / (|theta| ||K x||) over the free dofs, as last measured
    history: torch.Tensor = None   # [iterations + 1, k]: the residuals of the start block and after every iteration
    inner_failed: bool = False     # PCG_MAXITER because an inner solve did not converge (not the outer cap)


# Rayleigh-Ritz guards of the block LOBPCG. MODAL_COND: the scaled Gram matrix of the mass is dropped to [X W] past
# this eigh condition number. MODAL_THETA_FLOOR: a Ritz value at or below this fraction of the largest Ritz value of
# the start block (a lower bound of lambda_max) means lambda_1 / lambda_max < 1e-12 -- the rounding of a residual,
# eps * lambda_max / lambda_1 > 1e-4, then lies far above any usable tolerance, and a clamped structure's K is
# positive definite with a ratio of the order of (h / L)^2: the matrix is singular (no clamped dof) -> breakdown.
MODAL_COND = 1e12
MODAL_THETA_FLOOR = 1e-12


def modal_block(k: int, block: int = None) -> int:
    """Block width m of the LOBPCG for k eigenpairs: the smallest multi-vector width (MULTI_NV) that is >= k + 2,
    capped at 8; `block` (k <= block <= 8) is rounded up to such a width instead."""
    if not 1 <= int(k) <= MULTI_NV[-1]:
        raise ValueError(f"eig_lowest: 1 to {MULTI_NV[-1]} eigenpairs per solve, got {k}")
    want = min(int(k) + 2, MULTI_NV[-1]) if block is None else int(block)
    if not int(k) <= want <= MULTI_NV[-1]:
        raise ValueError(f"eig_lowest: block must lie in [{k}, {MULTI_NV[-1]}], got {block}")
    return next(v for v in MULTI_NV if v >= want)


def rayleigh_ritz(GK: torch.Tensor, GM: torch.Tensor, m: int):
    """The m lowest Ritz pairs of the small pencil (GK, GM) on the host: both scaled by diag(GM)^(-1/2), GM
    Cholesky-factored, the standard symmetric problem solved by eigh. Returns (theta [m], C [am, m]) with
    C^T GM C = I, or None when GM is not safely positive definite (non-finite entries, a diagonal <= 0, a failed
    Cholesky, or an eigh condition number of the scaled GM above MODAL_COND)."""
    GK, GM = GK.to(F64), GM.to(F64)
    d = GM.diagonal()
    if not bool(torch.isfinite(GK).all() and torch.isfinite(GM).all()) or bool((d <= 0).any()):
        return None
    s = d.rsqrt()
    A = s[:, None] * GK * s[None, :]
    B = s[:, None] * GM * s[None, :]
    ev = torch.linalg.eigvalsh(B)
    if not float(ev[0]) > 0.0 or float(ev[-1] / ev[0]) > MODAL_COND:
        return None
    L, info = torch.linalg.cholesky_ex(B)
    if int(info) != 0:
        return None
    T = torch.linalg.solve_triangular(L, A, upper=False)                 # L^-1 A
    T = torch.linalg.solve_triangular(L, T.T.contiguous(), upper=False)  # L^-1 A L^-T (transposed: symmetric)
    T = 0.5 * (T + T.T)
    lam, Z = torch.linalg.eigh(T)
    Cm = s[:, None] * torch.linalg.solve_triangular(L.T.contiguous(), Z[:, :m].contiguous(), upper=True)
    return lam[:m].clone(), Cm.contiguous()


@dataclass
class Graph:
    """Node graph of a mesh: incidence + CSR pattern + SELL-64 pattern, all on one device."""
    n_nodes: int
    npe: int
    inc_ptr: torch.Tensor
    inc: torch.Tensor
    rowptr: torch.Tensor
    colidx: torch.Tensor
    diagpos: torch.Tensor
    slice_ptr: torch.Tensor
    cols: torch.Tensor
    c2s: torch.Tensor = None     # CSR -> SELL entry map, formed on first use (csr2sell)
    dcols: torch.Tensor = None   # int16 col - row deltas, or None when the bandwidth exceeds 32767
    max_width: int = 0           # widest SELL slice in columns (0: unknown)

    @property
    def csr2sell(self):
        """CSR position -> SELL entry (int64 [nnz]). The fused pattern pass skips it (the c3d4 assembly, Jacobi and
        the solvers address SELL through the slice pointer); the stored-K_e assembly and the CSR export form it
        here on first use, on the graph's device and current stream."""
        if self.c2s is None:
            with C.device_scope(self.rowptr.device):
                c2s = torch.empty(max(self.nnz, 1), dtype=I64, device=self.rowptr.device)
                C.check(C.lib().fem_sell_csr2sell(C.ptr(self.rowptr), self.n_nodes, C.ptr(self.slice_ptr),
                                                  C.ptr(c2s), C.stream(self.rowptr.device)), "fem_sell_csr2sell")
                self.c2s = c2s
        return self.c2s

    def solver_layout(self):
        """The bs = 1 solver layout of this pattern (include/fem355.h fem_sell_sl_pattern): lane-paired deltas,
        slice-uniform delta lists, and the persistent schedule's gather windows for this device's grid -- formed once
        per pattern, on first use (or by build_graph(..., solver_layout=True) in its fill pass). None without 16-bit
        deltas."""
        if self.dcols is None:
            return None
        sl = getattr(self, "_sl", None)
        if sl is None:
            dev = self.rowptr.device
            with C.device_scope(dev):
                sl = _solver_layout_arrays(dev, self.sell_entries, self.n_nodes)
                C.check(C.lib().fem_sell_sl_pattern(self.n_nodes, C.ptr(self.slice_ptr), C.ptr(self.dcols), sl.G,
                                                    C.ptr(sl.pcols), C.ptr(sl.ucol), C.ptr(sl.uoff), C.ptr(sl.win),
                                                    C.stream(dev)), "fem_sell_sl_pattern")
            self._sl = sl
        return sl

    @property
    def nnz(self):
        return int(self.colidx.numel())

    @property
    def sell_entries(self):
        return int(self.cols.numel())


@dataclass
class SolverLayout:
    """Solver layout of a bs = 1 pattern (Graph.solver_layout): paired deltas, uniform lists, gather windows."""
    pcols: torch.Tensor
    ucol: torch.Tensor
    uoff: torch.Tensor
    win: torch.Tensor
    G: int


_NCU = {}


def _cu_count(dev):
    """Compute units of `dev` (cached: this sits between the pattern build's one sync and its next launch)."""
    k = dev.index if dev.index is not None else torch.cuda.current_device()
    if k not in _NCU:
        _NCU[k] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _NCU[k]


def _solver_layout_arrays(dev, ent, n_nodes):
    """Uninitialised SolverLayout arrays of a pattern with `ent` SELL entries (G: the persistent grid of `dev`)."""
    ncu = _cu_count(dev)
    G = (ncu // 8) * 8
    ns = (n_nodes + 63) // 64
    return SolverLayout(torch.empty(max(ent, 1), dtype=torch.int16, device=dev),
                        torch.empty(2 * (ent // 64) + 2, dtype=torch.int16, device=dev),
                        torch.empty(max(ns, 1), dtype=I32, device=dev),
                        torch.empty(max(2 * G, 1), dtype=I32, device=dev), G)


def check_connectivity(elements: torch.Tensor, n_nodes: int):
    """IndexError for a node index outside [0, n_nodes) (the kernels gather without bounds checks; the
    reference's torch indexing raises IndexError on such input). One device reduction + sync."""
    if elements.numel() == 0:
        return
    lo, hi = (int(v) for v in torch.stack(torch.aminmax(elements)).cpu())   # one device-to-host copy
    if lo < 0 or hi >= n_nodes:
        raise IndexError(f"element connectivity references node {lo if lo < 0 else hi}, outside [0, {n_nodes})")


def incidence(elements: torch.Tensor, n_nodes: int, checked: bool = False):
    """Deterministic node -> (element, local) incidence of a connectivity block [M, npe] (int64, device)."""
    with C.device_scope(elements.device):
        return _incidence(elements, n_nodes, checked)


def _incidence(elements, n_nodes, checked):
    lib = C.lib()
    if not checked:
        check_connectivity(elements, n_nodes)
    dev = elements.device
    M, npe = elements.shape
    inc_ptr = torch.empty(n_nodes + 1, dtype=I32, device=dev)
    inc = torch.empty(M * npe, dtype=I32, device=dev)
    # workspace from torch's caching allocator: it is reused by the pattern arrays allocated right after
    work = torch.empty(max(int(lib.fem_incidence_work_bytes(M * npe, n_nodes)), 1), dtype=torch.uint8, device=dev)
    C.check(lib.fem_incidence(C.ptr(elements), M, npe, n_nodes, C.ptr(inc_ptr), C.ptr(inc), C.ptr(work),
                              C.stream(dev)), "fem_incidence")
    return inc_ptr, inc


def build_graph(elements: torch.Tensor, n_nodes: int, compress: bool = True, solver_layout: bool = False) -> Graph:
    """Node-graph CSR + SELL-64 pattern of `elements` (one element family, int64 [M, npe] on the device).
    The rows are the coalesced pattern of the reference's COO assembly (`subdivision.ipynb:118-139`).
    compress: also derive 16-bit column deltas (used by the SpMV when every |col - row| <= 32767).
    solver_layout: with the deltas, also form the bs = 1 solver layout (Graph.solver_layout) in the same fill pass."""
    with C.device_scope(elements.device):
        return _build_graph(elements, n_nodes, compress, solver_layout)


def _build_graph(elements, n_nodes, compress, solver_layout=False):
    lib = C.lib()
    dev = elements.device
    elements = elements.contiguous()
    M, npe = elements.shape
    st = C.stream(dev)
    # the connectivity check rides on the incidence's count pass (out-of-range slots are left out; the kernels
    # below only compare node ids, never index by them) and is read back with the sizes in the one sync below
    inc_ptr = torch.empty(n_nodes + 1, dtype=I32, device=dev)
    inc = torch.empty(M * npe, dtype=I32, device=dev)
    bad = torch.empty(1, dtype=I32, device=dev)
    work = torch.empty(max(int(lib.fem_incidence_work_bytes(M * npe, n_nodes)), 1), dtype=torch.uint8, device=dev)
    C.check(lib.fem_incidence_checked(C.ptr(elements), M, npe, n_nodes, C.ptr(inc_ptr), C.ptr(inc), C.ptr(work),
                                      C.ptr(bad), st), "fem_incidence_checked")
    del work
    row_len = torch.empty(n_nodes, dtype=I32, device=dev)
    tmp = torch.empty(max(int(lib.fem_graph_tmp_len(n_nodes)), 1), dtype=I32, device=dev)
    ovf = torch.empty(1, dtype=I32, device=dev)   # 1: some neighbour is > 32767 rows away (no 16-bit deltas)
    C.check(lib.fem_graph_count2(C.ptr(elements), npe, C.ptr(inc_ptr), C.ptr(inc), n_nodes, C.ptr(row_len),
                                 C.ptr(tmp), C.ptr(ovf), st), "fem_graph_count2")
    rowptr = torch.empty(n_nodes + 1, dtype=I32, device=dev)
    work = torch.empty(int(lib.fem_scan_work_len(n_nodes)) + 1, dtype=I32, device=dev)
    C.check(lib.fem_scan_i32(C.ptr(row_len), n_nodes, C.ptr(rowptr), C.ptr(work), st), "fem_scan_i32")
    # the SELL slice widths need only the row lengths: both sizes come back in ONE device-to-host copy
    ns = (n_nodes + 63) // 64
    width = torch.empty(ns, dtype=I64, device=dev)
    C.check(lib.fem_sell_widths(C.ptr(rowptr), n_nodes, C.ptr(width), st), "fem_sell_widths")
    slice_ptr = torch.empty(ns + 1, dtype=I64, device=dev)
    work64 = torch.empty(int(lib.fem_scan_work_len(ns)) + 1, dtype=I64, device=dev)
    C.check(lib.fem_scan_i64(C.ptr(width), ns, C.ptr(slice_ptr), C.ptr(work64), st), "fem_scan_i64")
    sizes = torch.empty(5, dtype=I64, device=dev)   # {nnz, entries, bad, far, widest slice}: one launch
    C.check(lib.fem_graph_sizes(C.ptr(rowptr), C.ptr(slice_ptr), C.ptr(width), n_nodes, C.ptr(bad), C.ptr(ovf),
                                C.ptr(sizes), st), "fem_graph_sizes")
    nnz, ent, nbad, far, maxw = (int(v) for v in sizes.cpu())
    if nbad:   # the sync of the build; the message names the offending node like check_connectivity
        check_connectivity(elements, n_nodes)
    # int32 row pointers / column slots: the int32 scan would wrap past 2^31 entries; the int64 slice scan cannot
    # (per-row lengths stay exact under wrap-around), and nnz <= ent
    if ent >= 2**31:
        raise ValueError(f"fem355: {ent} SELL entries (>= node-graph entries) exceed the int32 pattern "
                         "(split the mesh over GPUs)")
    colidx = torch.empty(nnz, dtype=I32, device=dev)
    diagpos = torch.empty(n_nodes, dtype=I32, device=dev)
    cols = torch.empty(ent, dtype=I32, device=dev)
    dcols = torch.empty(max(ent, 1), dtype=torch.int16, device=dev) if compress and not far else None
    sl = None
    if dcols is not None and solver_layout and os.environ.get("FEM355_SL_SEPARATE") is None:
        sl = _solver_layout_arrays(dev, ent, n_nodes)
        C.check(lib.fem_graph_sell_fill_sl(C.ptr(elements), npe, C.ptr(inc_ptr), C.ptr(inc), n_nodes, C.ptr(rowptr),
                                           C.ptr(tmp), C.ptr(slice_ptr), C.ptr(colidx), C.ptr(diagpos), C.ptr(cols),
                                           C.ptr(dcols), sl.G, C.ptr(sl.pcols), C.ptr(sl.ucol), C.ptr(sl.uoff),
                                           C.ptr(sl.win), st), "fem_graph_sell_fill_sl")
    else:
        C.check(lib.fem_graph_sell_fill(C.ptr(elements), npe, C.ptr(inc_ptr), C.ptr(inc), n_nodes, C.ptr(rowptr),
                                        C.ptr(tmp), C.ptr(slice_ptr), C.ptr(colidx), C.ptr(diagpos), C.ptr(cols),
                                        C.ptr(dcols), None, None, st), "fem_graph_sell_fill")
    del tmp
    g = Graph(n_nodes, npe, inc_ptr, inc, rowptr, colidx, diagpos, slice_ptr, cols)
    if sl is not None:
        g._sl = sl
    g.dcols = dcols
    g.max_width = maxw // 64 if ns > 0 else 0   # widest slice, in columns (the value kernels' window choice)
    return g


def rcm_order(elements: torch.Tensor, n_nodes: int, graph: Graph = None):
    """Reverse Cuthill-McKee renumbering of the mesh nodes, computed on the device (csrc/reorder.hip) ->
    (perm, inv), int64 on the elements' device: new node k is old node perm[k], old node v becomes inv[v].
    Opt-in: meshes read in file order (`vtk_loader_to_torch`, `solver/element.py:39-90`) scatter the SELL slices'
    gathers and can need int32 columns; the renumbered mesh's operator is the same matrix under a symmetric
    permutation, so solutions map back exactly up to summation order."""
    with C.device_scope(elements.device):
        lib = C.lib()
        g = graph if graph is not None else build_graph(elements, n_nodes, compress=False)
        dev = elements.device
        perm = torch.empty(n_nodes, dtype=I32, device=dev)
        inv = torch.empty(n_nodes, dtype=I32, device=dev)
        work = torch.empty(max(int(lib.fem_rcm_work_len(n_nodes)), 1), dtype=I32, device=dev)
        lv = ctypes.c_int(0)
        C.check(lib.fem_rcm(C.ptr(g.rowptr), C.ptr(g.colidx), n_nodes, C.ptr(perm), C.ptr(inv), C.ptr(work),
                            ctypes.byref(lv), C.stream(dev)), "fem_rcm")
        return perm.long(), inv.long()


def renumber(coords: torch.Tensor, elements: torch.Tensor, perm: torch.Tensor, inv: torch.Tensor):
    """The mesh under a node renumbering (rcm_order): coordinates in the new order, connectivity in new ids."""
    return coords[perm], inv[elements]


def pad_connectivity(blocks, npe_max):
    """Concatenate element families into one [sum M, npe_max] block for the pattern (padding repeats node 0
    of the element; duplicates vanish in the unique-neighbour pass)."""
    out = []
    for el in blocks:
        if el.shape[1] < npe_max:
            el = torch.cat([el, el[:, :1].expand(-1, npe_max - el.shape[1])], dim=1)
        out.append(el)
    return torch.cat(out, 0).contiguous()


class SixDofMap:
    """6 dofs per node on the bs = 3 matrices: every node n has a translation block n in [0, N); every node that
    carries a shell also has a rotation block N + rank(n), rank(n) its position among the shell nodes in ascending
    order. Dof (n, c) is scalar row 3 block + c % 3. A shell element with npe nodes is then an ordinary bs = 3 element
    with 2 npe block-nodes [t0 .. t(npe-1), r0 .. r(npe-1)] -- the row order of fem_shell_ke's global-frame matrices
    -- and solid families keep their node ids. Rotation dofs of a node without a shell have no rows."""

    def __init__(self, n_nodes: int, shells):
        shells = [s for s in shells if s is not None]
        if not shells:
            raise ValueError("SixDofMap: no shell connectivity")
        dev = shells[0].device
        self.device = dev
        self.n_nodes = int(n_nodes)
        has = torch.zeros(self.n_nodes, dtype=torch.bool, device=dev)
        for s in shells:
            check_connectivity(s, self.n_nodes)
            has[s.reshape(-1)] = True
        self.has_shell = has
        self.shell_nodes = torch.nonzero(has).view(-1)
        rank = torch.cumsum(has.to(I64), 0) - 1
        self.rot_block = torch.where(has, self.n_nodes + rank, torch.full_like(rank, -1))
        self.n_blocks = self.n_nodes + int(self.shell_nodes.numel())

    def shell_connectivity(self, shell: torch.Tensor) -> torch.Tensor:
        """[M, 2 npe] block-node connectivity of a shell family: its nodes, then their rotation blocks."""
        shell = shell.to(device=self.device, dtype=I64)
        return torch.cat([shell, self.rot_block[shell]], dim=1).contiguous()

    def to_blocks(self, x: torch.Tensor) -> torch.Tensor:
        """x [N, 6] -> [n_blocks, 3] (the rotation columns of nodes without a shell are left out)."""
        x = x.to(device=self.device, dtype=F64)
        if tuple(x.shape) != (self.n_nodes, 6):
            raise ValueError(f"expected [{self.n_nodes}, 6], got {list(x.shape)}")
        return torch.cat([x[:, :3], x[self.shell_nodes, 3:]], dim=0).contiguous()

    def from_blocks(self, xb: torch.Tensor, base: torch.Tensor = None) -> torch.Tensor:
        """[n_blocks, 3] -> [N, 6]; rotation columns of nodes without a shell come from `base` [N, 6] (else 0)."""
        xb = xb.view(self.n_blocks, 3)
        out = (torch.zeros((self.n_nodes, 6), dtype=F64, device=self.device) if base is None
               else base.to(device=self.device, dtype=F64).clone())
        out[:, :3] = xb[: self.n_nodes]
        out[self.shell_nodes, 3:] = xb[self.n_nodes:]
        return out

    def free_mask(self, fixed=None) -> torch.Tensor:
        """1 on free scalar rows, 0 on all six dofs of the `fixed` nodes -> [3 n_blocks] fp64."""
        w = torch.ones((self.n_nodes, 6), dtype=F64, device=self.device)
        if fixed is not None:
            w[torch.as_tensor(fixed).to(device=self.device, dtype=I64)] = 0.0
        return self.to_blocks(w).view(-1)

    def rowless_load(self, force: torch.Tensor) -> bool:
        """True when `force` [N, 6] loads a rotation dof that has no rows (a node without a shell)."""
        f = force.to(device=self.device)
        return bool((f[~self.has_shell, 3:] != 0).any())


def uniform_slices(lib, h, s_begin=0, s_end=-1):
    """fem_pcg_uniform_slices of a solver context handle: (uniform slices, slices, column-index bytes per SpMV)."""
    u, n, ib = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    C.check(lib.fem_pcg_uniform_slices(h, int(s_begin), int(s_end), ctypes.byref(u), ctypes.byref(n),
                                       ctypes.byref(ib)), "fem_pcg_uniform_slices")
    return u.value, n.value, ib.value


# Two-level PCG (csrc/pcg_coarse.hip): free nodes per aggregate of the default aggregation, and the most aggregates
# (m = 6 k <= 3072: Einv is a dense [m, m] tensor that every iteration reads). COARSE_TARGET was chosen from time to
# solution at the n = 55 and n = 119 cubes among 500, 1500 and 4000 (setup included: 96 / 46 / 40 ms at n = 55,
# 275 / 275 / 294 ms at n = 119, where 500 and 1500 both reach the cap; DESIGN §8p, profiles/twolevel_n*.json).
COARSE_TARGET = 1500
COARSE_MAX_AGG = 512
COARSE_DROP = 1e-10   # directions of an aggregate's Gram block below this fraction of its largest eigenvalue go


class CoarseSpace:
    """Rigid-body coarse space of a bs = 3 matrix (SellMatrix.rigid_coarse_space): k aggregates of free nodes, six
    modes each, Z never stored. `E` is Z^T A Z as the Galerkin kernels sum it (not symmetrised), `Einv` the symmetric
    T (T^T E T)^-1 T^T the iteration reads, `dropped` the number of degenerate directions left out, `times` the setup's
    synchronised wall milliseconds {"aggregation", "E", "inverse"}."""

    def __init__(self, A, w, agg, agg_ptr, agg_nodes, centre, radius, rel):
        self.A, self.device = A, A.device
        self.w = w
        self.agg, self.agg_ptr, self.agg_nodes = agg, agg_ptr, agg_nodes
        self.centre, self.radius, self.rel = centre, radius, rel
        self.n_aggregates = int(agg_ptr.numel()) - 1
        self.m = 6 * self.n_aggregates
        self.dropped = 0
        self.E = self.Einv = None
        self.times = {}

    def _restrict(self, rel, w, r):
        c = torch.empty(self.m, dtype=F64, device=self.device)
        C.check(C.lib().fem_coarse_restrict(self.A.n_rows, self.A.bs, self.n_aggregates, C.ptr(self.agg_ptr),
                                            C.ptr(self.agg_nodes), C.ptr(rel), C.ptr(w), C.ptr(r), C.ptr(c),
                                            C.stream(self.device)), "fem_coarse_restrict")
        return c

    def _vec(self, v, what):
        v = v.to(device=self.device, dtype=F64).contiguous().view(-1)
        if v.numel() != self.A.n:
            raise ValueError(f"CoarseSpace: {what} must hold {self.A.n} values, got {v.numel()}")
        return v

    def restrict(self, r):
        """c [m] = Z^T r."""
        with C.device_scope(self.device):
            return self._restrict(self.rel, self.w, self._vec(r, "r"))

    def apply(self, r, w=None):
        """z = w o r + Z Einv Z^T r: the preconditioner as an operator. `w` defaults to the weights the space was built
        with; another `w` must have the same zeros (they mark the rows of Z that are zero)."""
        with C.device_scope(self.device):
            r = self._vec(r, "r")
            w = self.w if w is None else self._vec(w, "w")
            c = self._restrict(self.rel, w, r)
            y = torch.empty(self.m, dtype=F64, device=self.device)
            z = torch.empty_like(r)
            C.check(C.lib().fem_coarse_apply(self.A.n_rows, self.A.bs, self.n_aggregates, C.ptr(self.agg),
                                             C.ptr(self.rel), C.ptr(w), C.ptr(self.Einv), C.ptr(c), C.ptr(r), C.ptr(y),
                                             C.ptr(z), C.stream(self.device)), "fem_coarse_apply")
            return z

    def gram(self):
        """[k, 6, 6] blocks Z_a^T Z_a: column q is the restriction of Z's column q of every aggregate at once (the
        aggregates are disjoint)."""
        N, k = self.A.n_rows, self.n_aggregates
        x, y, z = self.rel[:, 0], self.rel[:, 1], self.rel[:, 2]
        o, l = torch.zeros_like(x), torch.ones_like(x)
        # columns of R_i = [I | -[rel]x]
        colsR = [(l, o, o), (o, l, o), (o, o, l), (o, -z, y), (z, o, -x), (-y, x, o)]
        live = (self.agg >= 0).to(F64)[:, None] * (self.w.view(N, 3) != 0).to(F64)
        G = torch.empty((k, 6, 6), dtype=F64, device=self.device)
        for q, col in enumerate(colsR):
            v = (torch.stack(col, 1) * live).contiguous().view(-1)
            G[:, :, q] = self._restrict(self.rel, self.w, v).view(k, 6)
        return G

    def galerkin(self):
        """E [m, m] = Z^T A Z over the free rows and columns (records per row and neighbour aggregate, a stable sort by
        key, one wave per key summing in record order)."""
        lib, A, dev, k = C.lib(), self.A, self.device, self.n_aggregates
        g, N, st = A.g, A.n_rows, C.stream(self.device)
        cols, dcols = A._multi_cols()
        vals = A.plain_values()
        cnt = torch.empty(N, dtype=I64, device=dev)
        C.check(lib.fem_coarse_galerkin_count(N, A.bs, C.ptr(g.slice_ptr), cols, dcols, C.ptr(self.agg), C.ptr(cnt),
                                              st), "fem_coarse_galerkin_count")
        off = torch.empty(N + 1, dtype=I64, device=dev)
        work = torch.empty(int(lib.fem_scan_work_len(N)) + 1, dtype=I64, device=dev)
        C.check(lib.fem_scan_i64(C.ptr(cnt), N, C.ptr(off), C.ptr(work), st), "fem_scan_i64")
        nrec = int(off[N].item())
        keys = torch.empty(max(nrec, 1), dtype=I64, device=dev)
        rec = torch.empty((max(nrec, 1), 36), dtype=F64, device=dev)
        C.check(lib.fem_coarse_galerkin(N, A.bs, k, C.ptr(g.slice_ptr), cols, dcols, C.ptr(vals), C.ptr(self.agg),
                                        C.ptr(self.rel), C.ptr(self.w), C.ptr(off), C.ptr(keys), C.ptr(rec), st),
                "fem_coarse_galerkin")
        skeys, order = torch.sort(keys[:nrec], stable=True)
        ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
        key_ptr = torch.zeros(ukeys.numel() + 1, dtype=I64, device=dev)
        key_ptr[1:] = torch.cumsum(counts, 0)
        E = torch.zeros((self.m, self.m), dtype=F64, device=dev)
        C.check(lib.fem_coarse_galerkin_sum(int(ukeys.numel()), k, C.ptr(ukeys), C.ptr(key_ptr),
                                            C.ptr(order.contiguous()), C.ptr(rec), C.ptr(E), st),
                "fem_coarse_galerkin_sum")
        self.records = nrec
        return E

    def invert(self, E):
        """(Einv, dropped): the 6 x 6 Gram blocks eigen-decomposed (batched, on the host: k small matrices), directions
        below COARSE_DROP of a block's largest eigenvalue dropped and the rest kept as the orthonormal T; Einv =
        T (T^T E T)^-1 T^T from a Cholesky on the device, symmetrised. ValueError when the Cholesky fails."""
        k, dev = self.n_aggregates, self.device
        lam, V = torch.linalg.eigh(self.gram().cpu())            # ascending per block
        keep = lam > COARSE_DROP * lam[:, -1:]
        keep[:, -1] = True
        a_of, q_of = torch.nonzero(keep, as_tuple=True)          # kept directions, by aggregate then eigenvalue
        mk = int(a_of.numel())
        T = torch.zeros((self.m, mk), dtype=F64)
        rows = (6 * a_of)[:, None] + torch.arange(6)[None, :]
        T[rows, torch.arange(mk)[:, None]] = V[a_of, :, q_of]
        T = T.to(dev)
        Es = 0.5 * (E + E.T)
        Ek = T.T @ Es @ T
        Ek = 0.5 * (Ek + Ek.T)
        L, info = torch.linalg.cholesky_ex(Ek)
        info = int(info)
        if info != 0 or not bool(torch.isfinite(L).all()):
            bad = int(a_of[info - 1]) if info > 0 else -1
            raise ValueError(f"rigid_coarse_space: the coarse matrix Z^T A Z is not positive definite (pivot "
                             f"{info - 1}, aggregate {bad}); is the matrix clamped and w its Jacobi weights?")
        Ik = torch.cholesky_solve(torch.eye(mk, dtype=F64, device=dev), L)
        Einv = T @ (0.5 * (Ik + Ik.T)) @ T.T
        return (0.5 * (Einv + Einv.T)).contiguous(), 6 * k - mk


def check_element_scale(what, scale, M, device):
    """The per-element scale of the scaled assembly: a float64 tensor of M values on `device`, else ValueError (a host
    tensor never reaches C.ptr). Returns it flat and contiguous."""
    if not torch.is_tensor(scale):
        raise ValueError(f"{what}: scale must be a float64 device tensor of {M} values, got {type(scale).__name__}")
    if not scale.is_cuda or scale.device != torch.device(device):
        raise ValueError(f"{what}: scale must live on {device}, got a {scale.device} tensor")
    if scale.dtype != F64:
        raise ValueError(f"{what}: scale must be float64, got {scale.dtype}")
    if scale.numel() != int(M):
        raise ValueError(f"{what}: scale must hold one value per element ({M}), got {scale.numel()}")
    return scale.contiguous().view(-1)


@_scoped
class SellMatrix:
    """Assembled global operator in SELL-64 with bs x bs blocks (bs = dofs per node)."""

    def __init__(self, graph: Graph, bs: int):
        self.g = graph
        self.bs = bs
        self.device = graph.cols.device
        # values are zeroed lazily: the first add_element_matrices of a fresh matrix STORES every value (padding
        # included) instead of adding onto a zeroed buffer -- one memset and one read of the matrix fewer
        self._vals = None            # plain SELL values, allocated on first use
        self._svals = None           # solver layout values (include/fem355.h fem_assemble_tet4_sl)
        self._plain_ok = False       # which of the two holds the current values
        self._sl_ok = False
        self._fresh = True
        self.use16 = graph.dcols is not None   # 16-bit column deltas in every SpMV of this matrix

    def _plain_buf(self):
        if self._vals is None:
            self._vals = torch.empty(max(self.g.sell_entries, 1) * self.bs * self.bs, dtype=F64, device=self.device)
        return self._vals

    @property
    def solver_layout(self):
        """True while the values live in the solver layout (the default of a fresh matrix's assembly: the PCG reads
        them as they are, no per-solve conversion, one resident copy); `vals` then forms the plain copy on demand."""
        return self._sl_ok

    @property
    def vals(self):
        """SELL values [entries * bs * bs] (plane layout); zero until something was added. The caller may edit them in
        place: once handed out, the plain values are the matrix (a solver-layout copy is dropped, so later matvec /
        jacobi / pcg read the edited values; the next solve converts them at its start)."""
        v = self.plain_values()
        self._sl_ok = False
        return v

    def plain_values(self):
        """The plain SELL values for READING (kernels, exports): formed from the solver layout when only it holds the
        values, which stays the matrix -- edits through this tensor are not seen by solves (use `vals` to edit)."""
        if self._fresh:
            self._plain_buf().zero_()
            self._fresh = False
            self._plain_ok = True
        elif not self._plain_ok and self._sl_ok:   # plain copy of a solver-layout matrix
            sl = self.g.solver_layout()
            C.check(C.lib().fem_sell_sl_unpair(self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), C.ptr(self.g.dcols),
                                               C.ptr(sl.uoff), C.ptr(sl.ucol), C.ptr(self.g.rowptr),
                                               C.ptr(self._svals), C.ptr(self._plain_buf()), C.stream(self.device)),
                    "fem_sell_sl_unpair")
            self._plain_ok = True
        return self._vals

    def _sl_target(self):
        """True when the next assembly writes the solver layout: 16-bit deltas, a fresh matrix or one held only there
        (FEM355_SL=0 keeps the plain layout)."""
        return (self.use16 and self.bs in (1, 3) and os.environ.get("FEM355_SL", "1") != "0"
                and (self._fresh or (self._sl_ok and not self._plain_ok)))

    def _svals_buf(self):
        if self._svals is None:
            self._svals = torch.empty(max(self.g.sell_entries, 1) * self.bs * self.bs, dtype=F64, device=self.device)
        return self._svals

    def _modify_plain(self):
        """The plain values about to change: current (or fresh), and the solver layout stale afterwards."""
        if not self._fresh:
            self.plain_values()   # forms the plain copy when only the solver layout holds the values
        self._plain_buf()
        self._sl_ok = False

    def reset(self):
        """Forget the values, keep the buffers: the next assembly call stores every value again (padding included),
        into the layout a fresh matrix would take. For an operator refilled on the same pattern (NewtonStatics)."""
        self._fresh = True
        self._plain_ok = False
        self._sl_ok = False
        return self

    @property
    def n_rows(self):
        return self.g.n_nodes

    @property
    def n(self):
        return self.g.n_nodes * self.bs

    # ---------------------------------------------------------------- assembly
    def add_element_matrices(self, Ke: torch.Tensor, elements: torch.Tensor, inc=None):
        """vals += coalesce(P_e^T K_e P_e) of one element family (deterministic row-gather)."""
        lib = C.lib()
        elements = elements.contiguous()
        Ke = Ke.to(F64).contiguous()
        npe = elements.shape[1]
        if Ke.shape[-1] != npe * self.bs:
            raise ValueError(f"element matrix size {Ke.shape[-1]} != {npe}*{self.bs}")
        inc_ptr, inc_ = inc if inc is not None else (
            (self.g.inc_ptr, self.g.inc) if npe == self.g.npe and elements.shape[0] * npe == self.g.inc.numel()
            else incidence(elements, self.g.n_nodes))
        # bs = 3 with the pattern's widest slice known: the tile form writes the SELL planes directly (csr2sell unused)
        tiled = self.bs == 3 and self.g.max_width > 0 and not os.environ.get("FEM355_KE_ROWS") \
            and not os.environ.get("FEM355_KE_COLS") and not os.environ.get("FEM355_KE_DIRECT")
        if tiled and npe in (4, 6, 8, 10) and self._sl_target():   # straight into the solver layout (layout A)
            store = self._fresh
            self._fresh = False
            C.check(lib.fem_assemble_from_ke_sl(C.ptr(Ke), C.ptr(elements), npe, C.ptr(inc_ptr), C.ptr(inc_),
                                                self.g.n_nodes, C.ptr(self.g.rowptr), C.ptr(self.g.colidx),
                                                C.ptr(self.g.slice_ptr), 1 if store else 0, self.g.max_width,
                                                C.ptr(self._svals_buf()), C.stream(self.device)),
                    "fem_assemble_from_ke_sl")
            self._sl_ok, self._plain_ok = True, False
            return self
        # bs = 1: the tile form as well (k_assemble_ke_tile1: no csr2sell map, no memset)
        tiled = tiled or (self.bs == 1 and self.g.max_width > 0 and npe in (4, 6, 8, 10)
                          and not os.environ.get("FEM355_KE_ROWS"))
        self._modify_plain()
        store = self._fresh
        self._fresh = False
        self._plain_ok = True
        C.check(lib.fem_assemble_from_ke_ex2(C.ptr(Ke), C.ptr(elements), npe, self.bs, C.ptr(inc_ptr), C.ptr(inc_),
                                             self.g.n_nodes, C.ptr(self.g.rowptr), C.ptr(self.g.colidx),
                                             None if tiled else C.ptr(self.g.csr2sell), C.ptr(self.g.slice_ptr),
                                             self.g.nnz, self.g.sell_entries, 1 if store else 0,
                                             self.g.max_width if tiled else 0, C.ptr(self._vals),
                                             C.stream(self.device)), "fem_assemble_from_ke_ex2")
        return self

    def add_shell_matrices(self, Ke_global: torch.Tensor, shell: torch.Tensor, dofmap: "SixDofMap"):
        """vals += one shell family on a 6-dof system: Ke_global [M, 6 npe, 6 npe] in the global frame and block order
        (fem_shell_ke, FEM_SHELL_GLOBAL), shell [M, npe] node ids, on this bs = 3 matrix whose rows are `dofmap`'s
        blocks. The family goes through add_element_matrices as a bs = 3 family of 2 npe block-nodes."""
        if self.bs != 3 or self.g.n_nodes != dofmap.n_blocks:
            raise ValueError(f"add_shell_matrices: a bs = 3 matrix over {dofmap.n_blocks} blocks is needed "
                             f"(bs = {self.bs}, {self.g.n_nodes} rows)")
        conn = dofmap.shell_connectivity(shell)
        return self.add_element_matrices(Ke_global, conn, inc=incidence(conn, dofmap.n_blocks))

    def add_stiffness_and_mass(self, Ke: torch.Tensor, Me: torch.Tensor, elements: torch.Tensor, mass: "SellMatrix"):
        """This bs = 3 matrix += coalesce(P_e^T K_e P_e) and the bs = 1 `mass` (same pattern object) += coalesce(P_e^T
        Me_e P_e) in ONE pass (include/fem355.h fem_assemble_from_ke_mass_sl: one column search and one incidence walk
        for both). Me is the scalar [M, npe, npe] of `compute_M_matrix(..., scalar=True)`. Both results are bit-identical
        to `add_element_matrices(Ke, ...)` and `mass.add_element_matrices(Me, ...)`; where the fused form does not apply
        (plain layout wanted, a non-fresh pair in different states, another pattern) the two separate calls run."""
        lib = C.lib()
        elements = elements.contiguous()
        npe = elements.shape[1]
        Ke = Ke.to(F64).contiguous()
        Me = Me.to(F64).contiguous()
        if Me.shape[-1] != npe or Ke.shape[-1] != 3 * npe:
            raise ValueError(f"element matrix sizes {Ke.shape[-1]} / {Me.shape[-1]} != 3*{npe} / {npe}")
        fused = (self.bs == 3 and mass.bs == 1 and mass.g is self.g and self.g.max_width > 0
                 and npe in (4, 6, 8, 10) and npe == self.g.npe and elements.shape[0] * npe == self.g.inc.numel()
                 and self._sl_target() and self._fresh == mass._fresh
                 and not any(os.environ.get(k) for k in ("FEM355_KE_ROWS", "FEM355_KE_COLS", "FEM355_KE_DIRECT",
                                                         "FEM355_KM_SPLIT")))
        if not fused:
            self.add_element_matrices(Ke, elements)
            mass.add_element_matrices(Me, elements)
            return self
        store = self._fresh
        self._fresh = False
        mass._modify_plain()
        mass._fresh = False
        C.check(lib.fem_assemble_from_ke_mass_sl(C.ptr(Ke), C.ptr(Me), C.ptr(elements), npe, C.ptr(self.g.inc_ptr),
                                                 C.ptr(self.g.inc), self.g.n_nodes, C.ptr(self.g.rowptr),
                                                 C.ptr(self.g.colidx), C.ptr(self.g.slice_ptr), 1 if store else 0,
                                                 self.g.max_width, C.ptr(self._svals_buf()), C.ptr(mass._vals),
                                                 C.stream(self.device)), "fem_assemble_from_ke_mass_sl")
        self._sl_ok, self._plain_ok = True, False
        mass._plain_ok = True
        return self

    def add_element_matrices_sym(self, Kp: torch.Tensor, elements: torch.Tensor, inc=None):
        """vals += coalesce(P_e^T K_e P_e) from the packed symmetric K_e of `element._solid_ke_sym` (bs = 3: upper
        blocks only, the lower ones read as their transposes; include/fem355.h fem_assemble_from_ke_sym) -- the
        configs[4] internal path: about half the element-matrix bytes written and read. Same sums in the same order
        as `add_element_matrices` of the full K_e whose lower blocks mirror its upper ones."""
        lib = C.lib()
        if self.bs != 3 or self.g.max_width <= 0:
            raise ValueError("packed K_e assembly: bs = 3 with the pattern's slice width (tile form)")
        elements = elements.contiguous()
        npe = elements.shape[1]
        if Kp.dtype != F64 or Kp.dim() != 2 or Kp.shape[1] != int(lib.fem_ke_sym_stride(npe)):
            raise ValueError(f"packed K_e must be fp64 [M, {int(lib.fem_ke_sym_stride(npe))}]")
        Kp = Kp.contiguous()
        inc_ptr, inc_ = inc if inc is not None else (
            (self.g.inc_ptr, self.g.inc) if npe == self.g.npe and elements.shape[0] * npe == self.g.inc.numel()
            else incidence(elements, self.g.n_nodes))
        if self._sl_target():
            store = self._fresh
            self._fresh = False
            out, la = self._svals_buf(), 1
            self._sl_ok, self._plain_ok = True, False
        else:
            self._modify_plain()
            store = self._fresh
            self._fresh = False
            self._plain_ok = True
            out, la = self._vals, 0
        C.check(lib.fem_assemble_from_ke_sym(C.ptr(Kp), C.ptr(elements), npe, C.ptr(inc_ptr), C.ptr(inc_),
                                             self.g.n_nodes, C.ptr(self.g.rowptr), C.ptr(self.g.colidx),
                                             C.ptr(self.g.slice_ptr), 1 if store else 0, self.g.max_width, la,
                                             C.ptr(out), C.stream(self.device)), "fem_assemble_from_ke_sym")
        return self

    def add_tet4(self, coords: torch.Tensor, elements: torch.Tensor, E: float, nu: float = 0.0, scale=None):
        """vals += the c3d4 operator computed on the fly (bs=3: elasticity E, nu; bs=1: Poisson, kappa=E).
        scale: a float64 device tensor of one factor per element -- element e then contributes scale[e] K_e (the
        per-element modulus of DESIGN §8t; fem_assemble_tet4_scaled*). None: the unscaled entry points."""
        if scale is not None:
            return self._add_tet4_scaled(coords, elements, E, nu, scale)
        lib = C.lib()
        bad = _dev_scalar(self.device, I64, elements.shape[0])
        self._bad = (bad, elements.shape[0])
        # 16-bit deltas: straight into the solver layout (fresh matrix, or one already held there)
        if self._sl_target() and not os.environ.get("FEM355_ASM_ROWS"):
            sl = self.g.solver_layout() if self.bs == 1 else None
            store = self._fresh
            self._fresh = False
            C.check(lib.fem_assemble_tet4_sl(C.ptr(coords), C.ptr(elements), float(E), float(nu), self.bs,
                                             C.ptr(self.g.inc_ptr), C.ptr(self.g.inc), self.g.n_nodes,
                                             C.ptr(self.g.rowptr), C.ptr(self.g.colidx), C.ptr(self.g.slice_ptr),
                                             C.ptr(sl.uoff) if sl else None, C.ptr(sl.ucol) if sl else None,
                                             1 if store else 0, self.g.max_width, C.ptr(self._svals_buf()), C.ptr(bad),
                                             C.stream(self.device)), "fem_assemble_tet4_sl")
            self._sl_ok, self._plain_ok = True, False
            return self
        self._modify_plain()
        store = self._fresh   # a fresh matrix is stored whole (padding zeroed): no memset, no read of the values
        self._fresh = False
        self._plain_ok = True
        C.check(lib.fem_assemble_tet4_ex2(C.ptr(coords), C.ptr(elements), float(E), float(nu), self.bs,
                                          C.ptr(self.g.inc_ptr), C.ptr(self.g.inc), self.g.n_nodes,
                                          C.ptr(self.g.rowptr), C.ptr(self.g.colidx),
                                          C.ptr(self.g.csr2sell) if os.environ.get("FEM355_ASM_ROWS") else None,
                                          C.ptr(self.g.slice_ptr), 1 if store else 0, self.g.max_width,
                                          C.ptr(self._vals), C.ptr(bad), C.stream(self.device)),
                "fem_assemble_tet4_ex2")
        return self

    def _add_tet4_scaled(self, coords, elements, E, nu, scale):
        """add_tet4 with a per-element scale: the same layout choice, store handling and `bad` bookkeeping, through
        the scaled entry points (which have no row-kernel form: FEM355_ASM_ROWS is not consulted)."""
        scale = check_element_scale("add_tet4", scale, elements.shape[0], self.device)
        lib = C.lib()
        bad = _dev_scalar(self.device, I64, elements.shape[0])
        self._bad = (bad, elements.shape[0])
        if self._sl_target():
            sl = self.g.solver_layout() if self.bs == 1 else None
            store = self._fresh
            self._fresh = False
            C.check(lib.fem_assemble_tet4_scaled_sl(C.ptr(coords), C.ptr(elements), float(E), float(nu), self.bs,
                                                    C.ptr(self.g.inc_ptr), C.ptr(self.g.inc), self.g.n_nodes,
                                                    C.ptr(self.g.rowptr), C.ptr(self.g.colidx),
                                                    C.ptr(self.g.slice_ptr), C.ptr(sl.uoff) if sl else None,
                                                    C.ptr(sl.ucol) if sl else None, 1 if store else 0,
                                                    self.g.max_width, C.ptr(scale), C.ptr(self._svals_buf()),
                                                    C.ptr(bad), C.stream(self.device)), "fem_assemble_tet4_scaled_sl")
            self._sl_ok, self._plain_ok = True, False
            return self
        self._modify_plain()
        store = self._fresh
        self._fresh = False
        self._plain_ok = True
        C.check(lib.fem_assemble_tet4_scaled(C.ptr(coords), C.ptr(elements), float(E), float(nu), self.bs,
                                             C.ptr(self.g.inc_ptr), C.ptr(self.g.inc), self.g.n_nodes,
                                             C.ptr(self.g.rowptr), C.ptr(self.g.colidx), None,
                                             C.ptr(self.g.slice_ptr), 1 if store else 0, self.g.max_width,
                                             C.ptr(scale), C.ptr(self._vals), C.ptr(bad), C.stream(self.device)),
                "fem_assemble_tet4_scaled")
        return self

    def check_singular(self):
        bad = getattr(self, "_bad", None)
        if bad is not None and int(bad[0].item()) < bad[1]:
            raise ValueError("Singular matrix encountered while computing B matrix.")

    # ---------------------------------------------------------------- operators
    def matvec(self, x: torch.Tensor, out: torch.Tensor = None):
        lib = C.lib()
        x = x.to(F64).contiguous()
        y = out if out is not None else torch.empty(self.n, dtype=F64, device=self.device)
        if self._sl_ok:
            if self.bs == 1:
                sl = self.g.solver_layout()
                pc, uo, uc = C.ptr(sl.pcols), C.ptr(sl.uoff), C.ptr(sl.ucol)
            else:   # layout A: plain deltas
                pc, uo, uc = C.ptr(self.g.dcols), None, None
            C.check(lib.fem_spmv_sl(self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), pc, C.ptr(self._svals), uo, uc,
                                    C.ptr(x), C.ptr(y), C.stream(self.device)), "fem_spmv_sl")
        elif self.use16:
            C.check(lib.fem_spmv16(self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), C.ptr(self.g.dcols),
                                   C.ptr(self.plain_values()), C.ptr(x), C.ptr(y), C.stream(self.device)), "fem_spmv16")
        else:
            C.check(lib.fem_spmv(self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), C.ptr(self.g.cols),
                                 C.ptr(self.plain_values()), C.ptr(x), C.ptr(y), C.stream(self.device)), "fem_spmv")
        return y

    def attach_cols16(self, h):
        """Point a (P)CG context at the 16-bit column deltas when this matrix uses them."""
        if self.use16:
            C.check(C.lib().fem_pcg_set_cols16(h, C.ptr(self.g.dcols)), "fem_pcg_set_cols16")

    def solver_vals_ptr(self, fused=False):
        """The values pointer a (P)CG context is created with: the solver layout's when it holds the values (the
        context then reads them through attach_layout), else the plain values."""
        if self._sl_ok and not fused:
            return C.ptr(self._svals)
        return C.ptr(self.plain_values())

    def attach_layout(self, h, fused=False):
        """Hand a context the solver-layout values (+ the bs = 1 pattern, the gather windows) (fem_pcg_set_layout):
        no conversion at start."""
        if self._sl_ok and not fused:
            sl = self.g.solver_layout()
            one = self.bs == 1
            C.check(C.lib().fem_pcg_set_layout(h, C.ptr(self._svals), C.ptr(sl.pcols) if one else None,
                                               C.ptr(sl.uoff) if one else None, C.ptr(sl.ucol) if one else None,
                                               C.ptr(sl.win), sl.G), "fem_pcg_set_layout")

    def jacobi(self, fixed_mask: torch.Tensor = None):
        """w = 1/diag(A) (inf -> 0), zero on fixed DOFs (uint8 mask [n])."""
        lib = C.lib()
        w = torch.empty(self.n, dtype=F64, device=self.device)
        if self._sl_ok:
            sl = self.g.solver_layout() if self.bs == 1 else None
            C.check(lib.fem_jacobi_sl(C.ptr(self._svals), self.bs, C.ptr(self.g.rowptr), C.ptr(self.g.diagpos),
                                      C.ptr(self.g.slice_ptr), C.ptr(sl.uoff) if sl else None,
                                      C.ptr(sl.ucol) if sl else None, self.g.n_nodes,
                                      C.ptr(fixed_mask), C.ptr(w), C.stream(self.device)), "fem_jacobi_sl")
            return w
        C.check(lib.fem_jacobi(C.ptr(self.plain_values()), self.bs, C.ptr(self.g.rowptr), C.ptr(self.g.diagpos),
                               None, C.ptr(self.g.slice_ptr), self.g.n_nodes,
                               C.ptr(fixed_mask), C.ptr(w), C.stream(self.device)), "fem_jacobi")
        return w

    def csr(self):
        """(rowptr, colidx, vals[nnz, bs, bs]) in block-CSR (export / testing)."""
        lib = C.lib()
        out = torch.empty(max(self.g.nnz, 1) * self.bs * self.bs, dtype=F64, device=self.device)
        C.check(lib.fem_sell_to_csr_vals(C.ptr(self.plain_values()), self.bs, C.ptr(self.g.rowptr), self.g.n_nodes,
                                         C.ptr(self.g.csr2sell), C.ptr(self.g.slice_ptr), C.ptr(out),
                                         C.stream(self.device)), "fem_sell_to_csr_vals")
        return self.g.rowptr, self.g.colidx, out[: self.g.nnz * self.bs * self.bs].view(-1, self.bs, self.bs)

    def algorithmic_bytes_spmv(self, index_bytes=None, index_total=None):
        """HBM bytes one SpMV must move: (8 bs^2 + idx) nnzb + 4 (nb+1) + 16 n, fp64 values;
        idx = 4 for int32 columns (the survey's 12 nnz + 4(n+1) + 16 n for bs=1), 2 for 16-bit deltas.
        index_total: the column-index bytes of the stored format instead of idx nnzb (slice-uniform deltas:
        PcgRunner.uniform_slices())."""
        idx = index_bytes if index_bytes is not None else (2 if self.use16 else 4)
        nnzb, nb = self.g.nnz, self.g.n_nodes
        ib = idx * nnzb if index_total is None else int(index_total)
        return 8 * self.bs * self.bs * nnzb + ib + 4 * (nb + 1) + 16 * nb * self.bs

    # ---------------------------------------------------------------- solver
    def pcg(self, b, x0=None, w=None, mode=C.MODE_PCG, tol=1e-8, max_iter=1000, eps=1e-30, history=False,
            chunk=32, fused=False, schedule=None, constraints=None, tune=None):
        """Run the device (P)CG; returns a PcgResult. `constraints` (a constraints.ConstraintSet, mode
        CG_CONSTRAINED, 3-kernel schedule) is projected onto x at start and after every x update. `tune`: the
        context's FEM_TUNE_* flags instead of the library default (A/B checks)."""
        lib = C.lib()
        b = b.to(device=self.device, dtype=F64).contiguous().view(-1)
        x = (torch.zeros(self.n, dtype=F64, device=self.device) if x0 is None
             else x0.to(device=self.device, dtype=F64).clone().contiguous().view(-1))
        w = w.to(device=self.device, dtype=F64).contiguous().view(-1)
        hist = torch.full((max(max_iter, 1),), float("nan"), dtype=F64, device=self.device) if history else None
        h = ctypes.c_void_p()
        sched = _schedule(fused, schedule, self.bs)
        # the solver layout is read by the paired schedules (FEM_TUNE_PAIR = 2); fused / constrained contexts: plain
        plain = sched == SCHED_FUSED or constraints is not None or (tune is not None and not (int(tune) & 2))
        args = (self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), C.ptr(self.g.cols), self.solver_vals_ptr(plain),
                C.ptr(b),
                C.ptr(x), C.ptr(w), mode, float(tol), float(eps), C.ptr(hist), hist.numel() if hist is not None else 0,
                C.stream(self.device), ctypes.byref(h))
        rc = lib.fem_pcg_create(*args)
        if rc == C.FEM_EHIP:   # out of memory: hand the library's recycled buffers and torch's cache back, retry once
            C.release_cache()
            torch.cuda.empty_cache()
            rc = lib.fem_pcg_create(*args)
        C.check(rc, "fem_pcg_create")
        try:
            C.check(lib.fem_pcg_set_schedule(h, sched), "fem_pcg_set_schedule")
            if tune is not None:
                C.check(lib.fem_pcg_set_tuning(h, int(tune)), "fem_pcg_set_tuning")
            C.check(lib.fem_pcg_set_entries(h, self.g.sell_entries), "fem_pcg_set_entries")
            self.attach_cols16(h)
            self.attach_layout(h, plain)
            if constraints is not None:
                C.check(lib.fem_pcg_set_constraints(h, *constraints.args()), "fem_pcg_set_constraints")
            it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
            C.check(lib.fem_pcg_solve(h, int(max_iter), int(chunk), ctypes.byref(it), ctypes.byref(stt),
                                      ctypes.byref(rz)), "fem_pcg_solve")
            sc = (ctypes.c_double * 6)()
            C.check(lib.fem_pcg_scalars(h, sc), "fem_pcg_scalars")
            ran = int(lib.fem_pcg_get_schedule(h))
            _check_sync(stt.value)
        finally:
            lib.fem_pcg_destroy(h)
        if hist is not None:
            hist = hist[: min(it.value, hist.numel())]
        return PcgResult(x, it.value, stt.value, rz.value, sc[1], hist, ran)

    # ---------------------------------------------------------------- several right-hand sides
    def _multi_cols(self):
        """(cols, dcols) arguments of the multi-vector kernels: the 16-bit deltas when the graph has them."""
        return C.ptr(self.g.cols), (C.ptr(self.g.dcols) if self.use16 else None)

    def matvec_multi(self, X: torch.Tensor, max_cols: int = None):
        """Y = A X for X [n, L], any L >= 1: the matrix is streamed once per pass (multi_passes: up to 8 columns for
        bs = 1, 4 for bs = 3; `max_cols` overrides) (include/fem355.h fem_spmm) instead of once per column. Column j
        equals matvec(X[:, j]) up to FMA contraction.
        Reads the plain SELL values: for a matrix held in the solver layout `plain_values()` forms a plain copy once,
        so one extra resident copy of the values."""
        if X.dim() != 2 or X.shape[0] != self.n or X.shape[1] < 1:
            raise ValueError(f"matvec_multi: X must be [{self.n}, L] with L >= 1, got {tuple(X.shape)}")
        lib = C.lib()
        X = X.to(device=self.device, dtype=F64)
        L = X.shape[1]
        Y = torch.empty((self.n, L), dtype=F64, device=self.device)
        cols, dcols = self._multi_cols()
        vals = C.ptr(self.plain_values())
        for j, k, nv in multi_passes(L, self.bs, max_cols):
            if k == nv == L and X.is_contiguous() and X.data_ptr() % 16 == 0:
                Xp, Yp = X, Y
            else:
                Xp = torch.zeros((self.n, nv), dtype=F64, device=self.device)
                Xp[:, :k] = X[:, j:j + k]
                Yp = torch.empty((self.n, nv), dtype=F64, device=self.device)
            C.check(lib.fem_spmm(self.g.n_nodes, self.bs, nv, C.ptr(self.g.slice_ptr), cols, dcols, vals, C.ptr(Xp),
                                 C.ptr(Yp), C.stream(self.device)), "fem_spmm")
            if Yp is not Y:
                Y[:, j:j + k] = Yp[:, :k]
        return Y

    def pcg_multi(self, B, x0=None, w=None, mode=C.MODE_PCG, tol=1e-8, max_iter=1000, eps=1e-30, history=False,
                  chunk=32, max_cols=None):
        """The device (P)CG for L right-hand sides B [n, L] in lock-step (include/fem355.h fem_mpcg_*): every column
        is the CG / Jacobi-PCG of `pcg` with its own alpha, beta, iteration count and status, and the matrix is read
        once per iteration for all columns of a pass; more columns than a pass takes (multi_passes: 8 for bs = 1, 4
        for bs = 3; `max_cols` overrides, at most 8) run in several passes. `w` [n] is shared by all columns,
        `tol` is a float or a length-L sequence. A column that has stopped is frozen; the others go on. Modes
        MODE_PCG and MODE_CG_STABLE. Returns a MultiPcgResult. Plain launches only, so no status needs the
        synchronisation check of `pcg`.
        Reads the plain SELL values: for a matrix held in the solver layout `plain_values()` forms a plain copy once,
        so one extra resident copy of the values."""
        if B.dim() != 2 or B.shape[0] != self.n or B.shape[1] < 1:
            raise ValueError(f"pcg_multi: B must be [{self.n}, L] with L >= 1, got {tuple(B.shape)}")
        L = B.shape[1]
        if x0 is not None and tuple(x0.shape) != (self.n, L):
            raise ValueError(f"pcg_multi: x0 must be [{self.n}, {L}], got {tuple(x0.shape)}")
        if w is None or w.numel() != self.n:
            raise ValueError(f"pcg_multi: w must hold {self.n} values (shared by all columns)")
        tols = [float(tol)] * L if not hasattr(tol, "__len__") else [float(t) for t in tol]
        if len(tols) != L:
            raise ValueError(f"pcg_multi: {len(tols)} tolerances for {L} columns")
        lib = C.lib()
        B = B.to(device=self.device, dtype=F64)
        w = w.to(device=self.device, dtype=F64).contiguous().view(-1)
        x = torch.zeros((self.n, L), dtype=F64, device=self.device)
        cols, dcols = self._multi_cols()
        vals = C.ptr(self.plain_values())
        its, stts, rzs, pqs, hists = [], [], [], [], []
        for j, k, nv in multi_passes(L, self.bs, max_cols):
            Bp = torch.zeros((self.n, nv), dtype=F64, device=self.device)
            Bp[:, :k] = B[:, j:j + k]
            Xp = torch.zeros((self.n, nv), dtype=F64, device=self.device)
            if x0 is not None:
                Xp[:, :k] = x0[:, j:j + k].to(device=self.device, dtype=F64)
            hist = (torch.full((max(max_iter, 1), nv), float("nan"), dtype=F64, device=self.device)
                    if history else None)
            tl = (ctypes.c_double * nv)(*tols[j:j + k])
            h = ctypes.c_void_p()
            C.check(lib.fem_mpcg_create(self.g.n_nodes, self.bs, nv, k, C.ptr(self.g.slice_ptr), cols, dcols, vals,
                                        C.ptr(Bp), C.ptr(Xp), C.ptr(w), int(mode), tl, float(eps), C.ptr(hist),
                                        hist.shape[0] if hist is not None else 0, C.stream(self.device),
                                        ctypes.byref(h)), "fem_mpcg_create")
            try:
                it, stt, rz = (ctypes.c_int * nv)(), (ctypes.c_int * nv)(), (ctypes.c_double * nv)()
                C.check(lib.fem_mpcg_solve(h, int(max_iter), int(chunk), it, stt, rz), "fem_mpcg_solve")
                sc = (ctypes.c_double * (6 * nv))()
                C.check(lib.fem_mpcg_scalars(h, sc), "fem_mpcg_scalars")
            finally:
                lib.fem_mpcg_destroy(h)
            x[:, j:j + k] = Xp[:, :k]
            its += list(it[:k])
            stts += list(stt[:k])
            rzs += list(rz[:k])
            pqs += [sc[6 * v + 1] for v in range(k)]
            if hist is not None:
                hists.append(hist[:, :k])
        hist = None
        if history:
            hist = torch.cat(hists, dim=1)[: min(max(its), max(max_iter, 1))]
        return MultiPcgResult(x, its, stts, rzs, pqs, hist)

    # ---------------------------------------------------------------- two-level PCG
    def rigid_coarse_space(self, coords, w, n_aggregates=None, aggregates=None) -> "CoarseSpace":
        """The rigid-body coarse space of this bs = 3 matrix for M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T (pcg_two_level).
        coords [n_rows, 3]; `w` [n] the masked Jacobi weights: dofs with w != 0 are free, a node is free if any of its
        dofs is, rows of Z at the other dofs are zero. The aggregates are `dist.rcb_partition` of the free nodes into
        `n_aggregates` parts (default ceil(free nodes / COARSE_TARGET), clamped to [1, COARSE_MAX_AGG]), or the
        caller's ids `aggregates` [n_rows] (-1: none; any labels, numbered here in ascending order). Per aggregate:
        centre and RMS radius rho of its free nodes, both rounded to fp32 (so that rel = (x - c) / rho carries the
        same bits whatever order the sums ran in); directions a degenerate aggregate cannot carry (a 2-node aggregate
        has no rotation about its axis) are dropped. ValueError for bs != 3, a 6-dof shell system (more rows than
        nodes) and a coarse matrix that is not positive definite."""
        import time
        try:
            from . import dist as _dist
        except ImportError:  # pragma: no cover - flat import
            import dist as _dist  # type: ignore
        N, dev = self.g.n_nodes, self.device
        if self.bs != 3:
            raise ValueError(f"rigid_coarse_space: a bs = 3 matrix with 3 translational dofs per node is needed "
                             f"(bs = {self.bs})")
        coords = coords.to(device=dev, dtype=F64).contiguous()
        if coords.dim() != 2 or tuple(coords.shape) != (N, 3):
            raise ValueError(f"rigid_coarse_space: coords must be [{N}, 3] (one node per block row; 6-dof shell "
                             f"systems are out of scope), got {list(coords.shape)}")
        if w is None or w.numel() != self.n:
            raise ValueError(f"rigid_coarse_space: w must hold {self.n} values (Jacobi weights, zero on the fixed dofs)")
        w = w.to(device=dev, dtype=F64).contiguous().view(-1)

        def tick():
            torch.cuda.synchronize(dev)
            return time.perf_counter()

        t0 = tick()
        free = (w.view(N, 3) != 0).any(1)
        if aggregates is None:
            ids = torch.nonzero(free).view(-1)
            nfree = int(ids.numel())
            if nfree == 0:
                raise ValueError("rigid_coarse_space: no free dof (w is zero everywhere)")
            k = -(-nfree // COARSE_TARGET) if n_aggregates is None else int(n_aggregates)
            if n_aggregates is not None and not 1 <= k <= COARSE_MAX_AGG:
                raise ValueError(f"rigid_coarse_space: 1 to {COARSE_MAX_AGG} aggregates, got {n_aggregates}")
            k = max(1, min(k, COARSE_MAX_AGG, nfree))
            label = torch.full((N,), -1, dtype=I64, device=dev)
            label[ids] = _dist.rcb_partition(coords[ids], k)
        else:
            label = aggregates.to(device=dev, dtype=I64).view(-1).clone()
            if label.numel() != N:
                raise ValueError(f"rigid_coarse_space: aggregates must hold {N} ids, got {label.numel()}")
            label[~free] = -1
        sel = torch.nonzero(label >= 0).view(-1)
        if sel.numel() == 0:
            raise ValueError("rigid_coarse_space: no free node lies in an aggregate")
        uniq, inv = torch.unique(label[sel], return_inverse=True)   # ascending labels -> 0 .. k - 1
        k = int(uniq.numel())
        if k > COARSE_MAX_AGG:
            raise ValueError(f"rigid_coarse_space: {k} aggregates exceed {COARSE_MAX_AGG} (m = 6 k <= "
                             f"{6 * COARSE_MAX_AGG})")
        agg = torch.full((N,), -1, dtype=I32, device=dev)
        agg[sel] = inv.to(I32)
        order = torch.sort(inv, stable=True).indices              # grouped by aggregate, ascending inside each
        agg_nodes = sel[order].to(I32).contiguous()
        agg_ptr = torch.zeros(k + 1, dtype=I32, device=dev)
        agg_ptr[1:] = torch.cumsum(torch.bincount(inv, minlength=k), 0).to(I32)
        cs = CoarseSpace(self, w, agg, agg_ptr, agg_nodes, None, None, None)
        # centre and radius from the restriction kernel (translation rows of Z^T with rel = 0, all dofs counted): the
        # node list in order, a fixed tree
        ones, zero = torch.ones(self.n, dtype=F64, device=dev), torch.zeros((N, 3), dtype=F64, device=dev)
        cnt = (agg_ptr[1:] - agg_ptr[:-1]).to(F64)[:, None]
        centre = (cs._restrict(zero, ones, coords.view(-1)).view(k, 6)[:, :3] / cnt).float().double()
        live = (agg >= 0)[:, None]
        ai = agg.long().clamp(min=0)
        d = torch.where(live, coords - centre[ai], zero)
        radius = (cs._restrict(zero, ones, (d * d).contiguous().view(-1)).view(k, 6)[:, :3].sum(1, keepdim=True)
                  / cnt).sqrt().float().double()
        radius = torch.where(radius > 0, radius, torch.ones_like(radius))   # a one-node aggregate
        cs.centre, cs.radius = centre, radius.view(-1)
        cs.rel = torch.where(live, d / radius[ai], zero).contiguous()
        t1 = tick()
        cs.E = cs.galerkin()
        t2 = tick()
        cs.Einv, cs.dropped = cs.invert(cs.E)
        t3 = tick()
        cs.times = {"aggregation": (t1 - t0) * 1e3, "E": (t2 - t1) * 1e3, "inverse": (t3 - t2) * 1e3}
        return cs

    def pcg_two_level(self, b, x0=None, w=None, coarse=None, tol=1e-8, max_iter=1000, history=False, chunk=32):
        """PCG with the two-level preconditioner of `coarse` (rigid_coarse_space; required): z = w o r + Z Einv Z^T r,
        MODE_PCG's semantics with this z (stop on sqrt(r.z) < tol, history of sqrt(r.z)) plus one guard, p.Ap <= 0 or
        non-finite -> PCG_BREAKDOWN at that iteration (Einv is only numerically positive definite). `w` defaults to
        the weights the space was built with. Plain launches (include/fem355.h fem_pcg2_*); reads the plain SELL
        values like pcg_multi. Returns a PcgResult."""
        if self.bs != 3:
            raise ValueError(f"pcg_two_level: a bs = 3 matrix is needed (bs = {self.bs})")
        if coarse is None or coarse.A is not self:
            raise ValueError("pcg_two_level: `coarse` must be this matrix's CoarseSpace (rigid_coarse_space)")
        lib = C.lib()
        b = b.to(device=self.device, dtype=F64).contiguous().view(-1)
        if b.numel() != self.n:
            raise ValueError(f"pcg_two_level: b must hold {self.n} values, got {b.numel()}")
        x = (torch.zeros(self.n, dtype=F64, device=self.device) if x0 is None
             else x0.to(device=self.device, dtype=F64).clone().contiguous().view(-1))
        w = coarse.w if w is None else w.to(device=self.device, dtype=F64).contiguous().view(-1)
        if x.numel() != self.n or w.numel() != self.n:
            raise ValueError(f"pcg_two_level: x0 and w must hold {self.n} values")
        hist = torch.full((max(max_iter, 1),), float("nan"), dtype=F64, device=self.device) if history else None
        cols, dcols = self._multi_cols()
        h = ctypes.c_void_p()
        C.check(lib.fem_pcg2_create(self.g.n_nodes, self.bs, C.ptr(self.g.slice_ptr), cols, dcols,
                                    C.ptr(self.plain_values()), C.ptr(b), C.ptr(x), C.ptr(w), coarse.n_aggregates,
                                    C.ptr(coarse.agg), C.ptr(coarse.agg_ptr), C.ptr(coarse.agg_nodes),
                                    C.ptr(coarse.rel), C.ptr(coarse.Einv), float(tol), C.ptr(hist),
                                    hist.numel() if hist is not None else 0, C.stream(self.device), ctypes.byref(h)),
                "fem_pcg2_create")
        try:
            it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
            C.check(lib.fem_pcg2_solve(h, int(max_iter), int(chunk), ctypes.byref(it), ctypes.byref(stt),
                                       ctypes.byref(rz)), "fem_pcg2_solve")
            sc = (ctypes.c_double * 6)()
            C.check(lib.fem_pcg2_scalars(h, sc), "fem_pcg2_scalars")
        finally:
            lib.fem_pcg2_destroy(h)
        if hist is not None:
            hist = hist[: min(it.value, hist.numel())]
        return PcgResult(x, it.value, stt.value, rz.value, sc[1], hist)

    # ---------------------------------------------------------------- stiffness and mass together
    def _mass_form(self, what, mass):
        """(FEM_MASS_* form, mass) of a `mass` argument, ValueError for one that does not fit -- no device call."""
        if isinstance(mass, SellMatrix):
            if mass.g is not self.g:
                raise ValueError(f"{what}: the mass matrix must be assembled on the same Graph object as this matrix")
            if mass.bs != 1:
                raise ValueError(f"{what}: the mass matrix is the scalar factor M_s (bs = 1), got bs = {mass.bs}")
            return C.MASS_SELL, mass
        if not torch.is_tensor(mass) or mass.dim() != 1 or mass.numel() != self.n:
            shape = tuple(mass.shape) if torch.is_tensor(mass) else type(mass).__name__
            raise ValueError(f"{what}: mass must be a bs = 1 SellMatrix or a diagonal of length {self.n}, got {shape}")
        return C.MASS_DIAG, mass

    def _mass_values(self, form, mass):
        if form == C.MASS_SELL:
            return mass.plain_values()
        return mass.to(device=self.device, dtype=F64).contiguous()

    def matvec_km_multi(self, mass, X: torch.Tensor, max_cols: int = None):
        """(K X, M X) for X [n, L] in one sweep of the pattern per pass (include/fem355.h fem_spmm_km): every gathered
        block column of X is loaded once for both products. `mass` is a bs = 1 SellMatrix on the same Graph object
        (M = M_s (x) I_bs: what add_stiffness_and_mass / compute_M_matrix(..., scalar=True) produce) or a tensor [n]
        (M = diag(mass)). Passes and padding as matvec_multi; column j of K X equals matvec_multi's bit for bit."""
        form, mass = self._mass_form("matvec_km_multi", mass)
        if X.dim() != 2 or X.shape[0] != self.n or X.shape[1] < 1:
            raise ValueError(f"matvec_km_multi: X must be [{self.n}, L] with L >= 1, got {tuple(X.shape)}")
        passes = multi_passes(X.shape[1], self.bs, max_cols)
        lib = C.lib()
        X = X.to(device=self.device, dtype=F64)
        L = X.shape[1]
        Y = torch.empty((self.n, L), dtype=F64, device=self.device)
        Z = torch.empty((self.n, L), dtype=F64, device=self.device)
        cols, dcols = self._multi_cols()
        vals, mv = self.plain_values(), self._mass_values(form, mass)
        for j, k, nv in passes:
            if k == nv == L and X.is_contiguous() and X.data_ptr() % 16 == 0:
                Xp, Yp, Zp = X, Y, Z
            else:
                Xp = torch.zeros((self.n, nv), dtype=F64, device=self.device)
                Xp[:, :k] = X[:, j:j + k]
                Yp = torch.empty((self.n, nv), dtype=F64, device=self.device)
                Zp = torch.empty((self.n, nv), dtype=F64, device=self.device)
            C.check(lib.fem_spmm_km(self.g.n_nodes, self.bs, nv, C.ptr(self.g.slice_ptr), cols, dcols, C.ptr(vals),
                                    C.ptr(mv), form, C.ptr(Xp), C.ptr(Yp), C.ptr(Zp), C.stream(self.device)),
                    "fem_spmm_km")
            if Yp is not Y:
                Y[:, j:j + k] = Yp[:, :k]
                Z[:, j:j + k] = Zp[:, :k]
        return Y, Z

    def eig_lowest(self, mass, k, w, block=None, tol=1e-8, max_iter=2000, seed=0, X0=None, history=False):
        """The k lowest eigenpairs of K u = lambda M u by block LOBPCG with the Jacobi preconditioner (csrc/modal.hip;
        what the docstring of the reference's `vectorized_modal_solver`, `solver/solver.py:1084-1313`, promises).
        `mass` as in matvec_km_multi. `w` [n] holds the Jacobi weights with zeros on the fixed dofs (SellMatrix.jacobi):
        X, W and P hold zeros on those rows from the start, so the pencil is the one of the free dofs and no row is
        eliminated. Block width m = modal_block(k, block). Per iteration: the residual R = KX - MX diag(theta) with
        W = w o R, ONE pass over the matrix for KW and MW, the Gram matrices of [X W P], one device-to-host read of
        them, Rayleigh-Ritz on the host (rayleigh_ritz; P is dropped for the iteration when the basis is too
        ill-conditioned: a restart), and the rotation of the basis and its products in place. Column j has converged
        when ||R_j|| <= tol theta_j ||MX_j|| (norms over the free dofs); the solve stops when the first k have.
        The start block comes from torch.Generator().manual_seed(seed) on the host (X0 [n, <= m] replaces its first
        columns) and is followed by a Rayleigh-Ritz on X alone. Same input, same bits.
        The clamped K must be positive definite: a Ritz value that is not finite, <= 0 or below MODAL_THETA_FLOOR of
        the start block's largest stops the solve with PCG_BREAKDOWN (the last good values are returned). Free-free
        structures and spectral shifts are out of scope. No column locking. Returns a ModalResult."""
        form, mass = self._mass_form("eig_lowest", mass)
        m = modal_block(k, block)
        k = int(k)
        if w is None or w.numel() != self.n:
            raise ValueError(f"eig_lowest: w must hold {self.n} values (Jacobi weights, zero on the fixed dofs)")
        if X0 is not None and (X0.dim() != 2 or X0.shape[0] != self.n or not 1 <= X0.shape[1] <= m):
            raise ValueError(f"eig_lowest: X0 must be [{self.n}, 1..{m}], got {tuple(X0.shape)}")
        if max_iter < 0:
            raise ValueError(f"eig_lowest: max_iter must be >= 0, got {max_iter}")
        lib = C.lib()
        dev, n = self.device, self.n
        w = w.to(device=dev, dtype=F64).contiguous().view(-1)
        start = torch.randn((n, m), dtype=F64, generator=torch.Generator().manual_seed(int(seed)))
        V = [torch.zeros((n, m), dtype=F64, device=dev) for _ in range(9)]   # X W P KX KW KP MX MW MP
        X, W, _, KX, KW, _, MX, MW, _ = V
        X.copy_(start)
        if X0 is not None:
            X[:, :X0.shape[1]] = X0.to(device=dev, dtype=F64)
        X.mul_((w != 0).to(F64)[:, None])
        ptrs = (ctypes.c_void_p * 9)(*[v.data_ptr() for v in V])
        work = torch.empty(int(lib.fem_modal_work_len()), dtype=F64, device=dev)
        out = torch.zeros(C.MODAL_OUT_LEN, dtype=F64, device=dev)
        coef = torch.zeros(3 * 64 + 8, dtype=F64, device=dev)     # C [a m, m], then theta at 192
        coef_host = torch.zeros(3 * 64 + 8, dtype=F64)
        cols, dcols = self._multi_cols()
        vals, mv = self.plain_values(), self._mass_values(form, mass)
        st = C.stream(dev)

        def product(Vin, KV, MV):
            C.check(lib.fem_spmm_km(self.g.n_nodes, self.bs, m, C.ptr(self.g.slice_ptr), cols, dcols, C.ptr(vals),
                                    C.ptr(mv), form, C.ptr(Vin), C.ptr(KV), C.ptr(MV), st), "fem_spmm_km")

        def gram(a):
            C.check(lib.fem_modal_gram(n, m, a, ptrs, C.ptr(work), C.ptr(out), st), "fem_modal_gram")

        def grams(host, a, sub):
            """(G_K, G_M) of the leading `sub` blocks out of a Gram launch with `a` blocks."""
            am = a * m
            GK = host[: am * am].view(am, am)[: sub * m, : sub * m]
            GM = host[C.MODAL_OUT_GM: C.MODAL_OUT_GM + am * am].view(am, am)[: sub * m, : sub * m]
            return GK, GM

        def rotate(a, theta, Cm):
            coef_host.zero_()
            coef_host[: a * m * m] = Cm.reshape(-1)
            coef_host[192: 192 + m] = theta
            coef.copy_(coef_host)
            C.check(lib.fem_modal_rotate(n, m, a, ptrs, C.ptr(coef), st), "fem_modal_rotate")

        def bad(theta, ref):
            return not bool(torch.isfinite(theta).all()) or bool((theta <= MODAL_THETA_FLOOR * ref).any())

        def result(theta, status, it, rel, restarts, hist):
            h = torch.stack(hist[1:]) if len(hist) > 1 else torch.zeros((0, k), dtype=F64)
            return ModalResult(theta[:k].clone(), X[:, :k].clone(), it, status, rel, restarts, h if history else None)

        nan = torch.full((k,), float("nan"), dtype=F64)
        # Rayleigh-Ritz on the start block alone
        product(X, KX, MX)
        gram(1)
        rr = rayleigh_ritz(*grams(out.cpu(), 1, 1), m)
        if rr is None or bad(rr[0], float(rr[0].abs().max())):
            return result(torch.zeros(m, dtype=F64), C.PCG_BREAKDOWN, 0, nan, 0, [])
        theta, Cm = rr
        theta_ref = float(theta.max())
        rotate(1, theta, Cm)
        has_p, restarts, hist, status, it = False, 0, [], C.PCG_MAXITER, 0
        rel = nan
        for it in range(int(max_iter) + 1):
            C.check(lib.fem_modal_residual(n, m, C.ptr(KX), C.ptr(MX), C.ptr(w), C.ptr(coef[192:]), C.ptr(W),
                                           C.ptr(work), C.ptr(out), st), "fem_modal_residual")
            a = 3 if has_p else 2
            if it < max_iter:      # the one pass over the matrices, and the Gram matrices: read with the norms
                product(W, KW, MW)
                gram(a)
            host = out.cpu()       # the iteration's one device-to-host read
            rn = host[C.MODAL_OUT_NORMS: C.MODAL_OUT_NORMS + m]
            mn = host[C.MODAL_OUT_NORMS + m: C.MODAL_OUT_NORMS + 2 * m]
            rel = (rn / (theta * mn))[:k].clone()
            hist.append(rel)
            if not bool(torch.isfinite(rel).all()):
                status = C.PCG_BREAKDOWN
                break
            if bool((rel <= tol).all()):
                status = C.PCG_CONVERGED
                break
            if it == max_iter:
                break
            rr = rayleigh_ritz(*grams(host, a, a), m)
            if rr is None and a == 3:       # restart: this iteration without P
                restarts += 1
                a = 2
                rr = rayleigh_ritz(*grams(host, 3, 2), m)
            if rr is None or bad(rr[0], theta_ref):
                status = C.PCG_BREAKDOWN
                break
            theta, Cm = rr
            rotate(a, theta, Cm)
            has_p = True
        return result(theta, status, it, rel, restarts, hist)

    def buckling_lowest(self, G, k, w, block=None, tol=1e-8, max_iter=200, linear_tol=1e-10, linear_max_iter=10000,
                        seed=0, history=False, timers=None):
        """The k load factors of smallest magnitude of linear buckling, (K + lambda K_g) phi = 0, with this matrix the
        bs = 3 stiffness K and `G` the bs = 1 SellMatrix of the geometric stiffness' scalar factor on the same Graph
        object (K_g = G (x) I3: compute_geometric_stiffness assembled like a scalar mass). `w` [n]: the Jacobi weights
        with zeros on the fixed dofs. K is positive definite on the free dofs, K_g is indefinite, so the pencil is
        turned round: G phi = theta K phi, lambda = -1 / theta, and the pairs of largest |theta| are found by block
        subspace iteration with K-solves (eig_lowest refuses shifts and indefinite pencils). The start
        block is eig_lowest's (host generator, `seed`, masked by w != 0, width m = modal_block(k, block)), followed by a
        Rayleigh-Ritz on it. Per outer iteration: the right-hand sides -G X with the fixed rows zeroed; pcg_multi on K
        from the warm start X diag(-theta) (exact for a converged column), every column to
        sqrt(r.z) <= linear_tol sqrt(b.w b); one fem_spmm_km sweep for (K X, G X); fem_modal_gram; one device-to-host
        read; rayleigh_ritz(X^T G X, X^T K X) on the host with its pairs reordered by |theta| descending;
        fem_modal_rotate; fem_modal_residual with G X in the place of K X and K X in the place of M X. Column j has
        converged when ||G x_j - theta_j K x_j|| <= tol |theta_j| ||K x_j|| over the free dofs; the solve stops when
        the first k have. Same input, same bits.
        PCG_BREAKDOWN: a Ritz value that is not finite, a Rayleigh-Ritz that fails, or every |theta| at or below
        MODAL_THETA_FLOOR of the start block's largest (G = 0: no prestress). PCG_MAXITER: the outer cap, or an inner
        solve that did not converge (inner_failed). No column locking. `timers` (a dict, for tools/bench_buckling.py):
        the seconds of the inner solves, the sweeps and the rest are added to its "solve", "sweep" and "host" entries,
        with a device synchronisation around each. Returns a BucklingResult."""
        form, G = self._mass_form("buckling_lowest", G)
        if form != C.MASS_SELL:
            raise ValueError("buckling_lowest: G must be a bs = 1 SellMatrix (the scalar factor of K_g)")
        if self.bs != 3:
            raise ValueError(f"buckling_lowest: the stiffness must be a bs = 3 matrix, got bs = {self.bs}")
        m = modal_block(k, block)
        k = int(k)
        if w is None or w.numel() != self.n:
            raise ValueError(f"buckling_lowest: w must hold {self.n} values (Jacobi weights, zero on the fixed dofs)")
        if max_iter < 0 or linear_max_iter < 1:
            raise ValueError(f"buckling_lowest: max_iter >= 0 and linear_max_iter >= 1 needed, got {max_iter} and "
                             f"{linear_max_iter}")
        lib = C.lib()
        dev, n = self.device, self.n
        w = w.to(device=dev, dtype=F64).contiguous().view(-1)
        free = (w != 0).to(F64)[:, None]
        start = torch.randn((n, m), dtype=F64, generator=torch.Generator().manual_seed(int(seed)))
        X, W, GX, KX = (torch.zeros((n, m), dtype=F64, device=dev) for _ in range(4))
        X.copy_(start)
        X.mul_(free)
        # the modal kernels' nine slots X W P KX KW KP MX MW MP: G X takes KX's, K X takes MX's; P and the W products
        # are never touched with one block (a = 1)
        ptrs = (ctypes.c_void_p * 9)(*[v.data_ptr() for v in (X, W, W, GX, W, W, KX, W, W)])
        work = torch.empty(int(lib.fem_modal_work_len()), dtype=F64, device=dev)
        out = torch.zeros(C.MODAL_OUT_LEN, dtype=F64, device=dev)
        coef = torch.zeros(3 * 64 + 8, dtype=F64, device=dev)     # C [m, m], then theta at 192
        coef_host = torch.zeros(3 * 64 + 8, dtype=F64)
        cols, dcols = self._multi_cols()
        vals, gv = self.plain_values(), G.plain_values()
        st = C.stream(dev)

        def timed(name, fn, *args):
            """fn(*args), its seconds added to timers[name] (with device synchronisations) when timers are kept."""
            if timers is None:
                return fn(*args)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = fn(*args)
            torch.cuda.synchronize(dev)
            own[name] = own.get(name, 0.0) + time.perf_counter() - t0
            return r

        own = {}

        def sweep():
            C.check(lib.fem_spmm_km(self.g.n_nodes, self.bs, m, C.ptr(self.g.slice_ptr), cols, dcols, C.ptr(vals),
                                    C.ptr(gv), form, C.ptr(X), C.ptr(KX), C.ptr(GX), st), "fem_spmm_km")

        def ritz():
            """Gram matrices of X, one read, Rayleigh-Ritz, |theta| descending -> (theta, C) or None."""
            C.check(lib.fem_modal_gram(n, m, 1, ptrs, C.ptr(work), C.ptr(out), st), "fem_modal_gram")
            host = out.cpu()
            GG = host[: m * m].view(m, m)
            GK = host[C.MODAL_OUT_GM: C.MODAL_OUT_GM + m * m].view(m, m)
            rr = rayleigh_ritz(GG, GK, m)
            if rr is None or not bool(torch.isfinite(rr[0]).all()):
                return None
            order = torch.argsort(rr[0].abs(), descending=True, stable=True)
            return rr[0][order].clone(), rr[1][:, order].contiguous()

        def rotate(theta, Cm):
            coef_host.zero_()
            coef_host[: m * m] = Cm.reshape(-1)
            coef_host[192: 192 + m] = theta
            coef.copy_(coef_host)
            C.check(lib.fem_modal_rotate(n, m, 1, ptrs, C.ptr(coef), st), "fem_modal_rotate")

        def result(theta, status, it, lin, rel, hist, inner=False):
            th = theta[:k].clone()
            h = torch.stack(hist) if hist else torch.zeros((0, k), dtype=F64)
            return BucklingResult(-1.0 / th, th, X[:, :k].clone(), it, lin, status, rel, h if history else None, inner)

        nan = torch.full((k,), float("nan"), dtype=F64)
        t_all = time.perf_counter()
        sweep()
        rr = ritz()
        if rr is None or not float(rr[0].abs().max()) > 0.0:
            return result(torch.zeros(m, dtype=F64), C.PCG_BREAKDOWN, 0, 0, nan, [])
        theta, Cm = rr
        theta_ref = float(theta.abs().max())
        rotate(theta, Cm)
        hist, status, it, lin, rel = [], C.PCG_MAXITER, 0, 0, nan
        for it in range(int(max_iter) + 1):
            C.check(lib.fem_modal_residual(n, m, C.ptr(GX), C.ptr(KX), C.ptr(w), C.ptr(coef[192:]), C.ptr(W),
                                           C.ptr(work), C.ptr(out), st), "fem_modal_residual")
            host = out.cpu()
            rn = host[C.MODAL_OUT_NORMS: C.MODAL_OUT_NORMS + m]
            kn = host[C.MODAL_OUT_NORMS + m: C.MODAL_OUT_NORMS + 2 * m]
            rel = (rn / (theta.abs() * kn))[:k].clone()
            hist.append(rel)
            if not bool(torch.isfinite(rel).all()):
                status = C.PCG_BREAKDOWN
                break
            if bool((rel <= tol).all()):
                status = C.PCG_CONVERGED
                break
            if it == max_iter:
                break
            B = GX.mul(free).neg_()
            scale = torch.sqrt((w[:, None] * B * B).sum(dim=0)).cpu()
            tols = [max(float(linear_tol) * float(s), 1e-300) for s in scale]
            sol = timed("solve", lambda: self.pcg_multi(B, x0=X * (-theta).to(dev)[None, :], w=w, mode=C.MODE_PCG,
                                                        tol=tols, max_iter=int(linear_max_iter)))
            lin += max(sol.iterations)
            if any(s != C.PCG_CONVERGED for s in sol.status):
                return result(theta, C.PCG_MAXITER, it, lin, rel, hist, inner=True)
            X.copy_(sol.x)
            timed("sweep", sweep)
            rr = ritz()
            if rr is None or float(rr[0].abs().max()) <= MODAL_THETA_FLOOR * theta_ref:
                status = C.PCG_BREAKDOWN
                break
            theta, Cm = rr
            rotate(theta, Cm)
        if timers is not None:   # everything that is neither an inner solve nor a sweep: Gram, Ritz, rotation, residual
            torch.cuda.synchronize(dev)
            own["host"] = time.perf_counter() - t_all - own.get("solve", 0.0) - own.get("sweep", 0.0)
            for name, secs in own.items():
                timers[name] = timers.get(name, 0.0) + secs
        return result(theta, status, it, lin, rel, hist)

    # ---------------------------------------------------------------- combinations with the mass (csrc/transient.hip)
    def _held_values(self):
        """(values, layout_a) as the transient kernels read this matrix: the bs = 3 layout A when it holds the values,
        else the plain planes (a bs = 1 matrix in the solver layout goes through plain_values())."""
        if self._sl_ok and self.bs == 3:
            return self._svals, 1
        return self.plain_values(), 0

    def scaled_add_mass(self, mass, cK, cM):
        """A new SellMatrix cK K + cM M on the same graph (include/fem355.h fem_sell_axpby_mass), `mass` as in
        matvec_km_multi: the effective matrix of an implicit time step, or a shifted K - sigma M. It is held in the
        solver layout exactly when this matrix is bs = 3 in the solver layout -- the PCG then reads it as it is --
        and in the plain planes otherwise. matvec, jacobi, pcg and csr work on the result unchanged."""
        form, mass = self._mass_form("scaled_add_mass", mass)
        mv = self._mass_values(form, mass)
        src, la = self._held_values()
        out = SellMatrix(self.g, self.bs)
        out.use16 = self.use16
        dst = out._svals_buf() if la else out._plain_buf()
        C.check(C.lib().fem_sell_axpby_mass(self.g.n_nodes, self.bs, la, self.g.sell_entries, C.ptr(self.g.slice_ptr),
                                            C.ptr(self.g.rowptr), C.ptr(self.g.diagpos), C.ptr(src), C.ptr(mv), form,
                                            float(cK), float(cM), C.ptr(dst), C.stream(self.device)),
                "fem_sell_axpby_mass")
        out._fresh = False
        out._sl_ok, out._plain_ok = bool(la), not la
        return out

    def quadforms(self, mass, x, y):
        """Device tensor [2] = (x^T K x, y^T M y) in one sweep of the pattern (include/fem355.h fem_quadform_km);
        bit-reproducible. `mass` as in matvec_km_multi."""
        form, mass = self._mass_form("quadforms", mass)
        if x.numel() != self.n or y.numel() != self.n:
            raise ValueError(f"quadforms: x and y must hold {self.n} values, got {x.numel()} and {y.numel()}")
        lib = C.lib()
        X = torch.stack((x.to(device=self.device, dtype=F64).reshape(-1),
                         y.to(device=self.device, dtype=F64).reshape(-1)), dim=1).contiguous()
        mv = self._mass_values(form, mass)
        kv, la = self._held_values()
        work = torch.empty(int(lib.fem_transient_work_len()), dtype=F64, device=self.device)
        out = torch.empty(2, dtype=F64, device=self.device)
        cols, dcols = self._multi_cols()
        C.check(lib.fem_quadform_km(self.g.n_nodes, self.bs, la, C.ptr(self.g.slice_ptr), cols, dcols, C.ptr(kv),
                                    C.ptr(mv), form, C.ptr(X), C.ptr(work), C.ptr(out), C.stream(self.device)),
                "fem_quadform_km")
        return out

    def energy(self, mass, u, v):
        """E = u^T K u / 2 + v^T M v / 2 (one device-to-host read)."""
        return 0.5 * float(self.quadforms(mass, u, v).sum())


@_scoped
class MatFreeOperator:
    """Element-chunk c3d4 operator (include/fem355.h fem_mf_*, csrc/matfree.hip): y = K x formed from the vertex
    coordinates in every application -- the reference's element-by-element product (`compute_nodal_forces`,
    `solver/element.py:429-464`) of the c3d4 stiffness (`compute_c3d4_K_matrix`, `:883-903`; kind "elastic", 3 dofs
    per node) or the P1 Laplacian (kind "poisson", kappa = E), no matrix in memory. Same interface as SellMatrix for
    what the solvers use (n, bs, matvec, diag, jacobi, pcg, PcgRunner)."""

    is_matfree = True

    def __init__(self, coords: torch.Tensor, elements: torch.Tensor, kind="elastic", E=1.0, nu=0.0):
        lib = C.lib()
        self.device = coords.device
        self.coords = coords.to(F64).contiguous()
        self.elements = elements.to(torch.int64).contiguous()
        self.kind = kind
        self.bs = 1 if kind == "poisson" else 3
        self.n_nodes = self.coords.shape[0]
        self.n = self.n_nodes * self.bs
        self.M = self.elements.shape[0]
        self.h = ctypes.c_void_p()
        bad = ctypes.c_int64(-1)
        k = C.KIND_POISSON if kind == "poisson" else C.KIND_ELASTIC
        C.check(lib.fem_mf_create(C.ptr(self.coords), C.ptr(self.elements), self.M, self.n_nodes, k, float(E),
                                  float(nu), ctypes.byref(bad), C.stream(self.device), ctypes.byref(self.h)),
                "fem_mf_create")

    def info(self):
        """{chunks, slots, bs, static bytes one application streams, M, N}"""
        out = (ctypes.c_int64 * 6)()
        C.check(C.lib().fem_mf_info(self.h, out), "fem_mf_info")
        keys = ("chunks", "slots", "bs", "static_bytes", "elements", "nodes")
        return dict(zip(keys, list(out)))

    def layout(self):
        """(Morton element order [M], chunk element offsets, chunk slot offsets, slot nodes) as device int32."""
        i = self.info()
        z = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=self.device)
        eo, cp, sb, cn = z(self.M), z(i["chunks"] + 1), z(i["chunks"] + 1), z(i["slots"])
        C.check(C.lib().fem_mf_order(self.h, C.ptr(eo), C.ptr(cp), C.ptr(sb), C.ptr(cn), C.stream(self.device)),
                "fem_mf_order")
        return eo[: self.M], cp[: i["chunks"] + 1], sb[: i["chunks"] + 1], cn[: i["slots"]]

    def algorithmic_bytes(self):
        """HBM bytes one application must move at least: the static layout streams + the coordinates, x and y once."""
        return self.info()["static_bytes"] + 24 * self.n_nodes + 16 * self.n

    def matvec(self, x: torch.Tensor, out: torch.Tensor = None):
        x = x.to(device=self.device, dtype=F64).contiguous().view(-1)
        y = out if out is not None else torch.empty(self.n, dtype=F64, device=self.device)
        C.check(C.lib().fem_mf_apply(self.h, C.ptr(x), C.ptr(y), C.stream(self.device)), "fem_mf_apply")
        return y

    def diag(self):
        d = torch.empty(self.n, dtype=F64, device=self.device)
        C.check(C.lib().fem_mf_diag(self.h, C.ptr(d), C.stream(self.device)), "fem_mf_diag")
        return d

    def jacobi(self, fixed_mask: torch.Tensor = None):
        """w = 1/diag(K) (inf -> 0), zero on fixed DOFs (uint8 mask [n])."""
        d = self.diag()
        w = torch.empty_like(d)
        C.check(C.lib().fem_jacobi_from_diag(C.ptr(d), self.n, C.ptr(fixed_mask), C.ptr(w), C.stream(self.device)),
                "fem_jacobi_from_diag")
        return w

    def check_singular(self):
        return None   # fem_mf_create already raised for a singular element

    def create_context(self, b, x, w, mode, tol, eps, hist, hist_len, stream, h):
        lib = C.lib()
        if mode == C.MODE_CG_CONSTRAINED:
            raise ValueError("the element-chunk operator has no constrained CG (SPC / RBE2 / RBE3 projections need "
                             "the assembled matrix: SellMatrix.pcg(..., constraints=...))")
        C.check(lib.fem_pcg_create(self.n_nodes, self.bs, None, None, None, C.ptr(b), C.ptr(x), C.ptr(w), mode,
                                   float(tol), float(eps), C.ptr(hist), hist_len, stream, ctypes.byref(h)),
                "fem_pcg_create")
        rc = lib.fem_pcg_set_operator_mf(h, self.h)
        if rc != C.FEM_OK:
            lib.fem_pcg_destroy(h)
            C.check(rc, "fem_pcg_set_operator_mf")

    def pcg(self, b, x0=None, w=None, mode=C.MODE_PCG, tol=1e-8, max_iter=1000, eps=1e-30, history=False, chunk=32):
        """Device (P)CG on this operator (3-kernel schedule with the merged update); returns a PcgResult."""
        lib = C.lib()
        b = b.to(device=self.device, dtype=F64).contiguous().view(-1)
        x = (torch.zeros(self.n, dtype=F64, device=self.device) if x0 is None
             else x0.to(device=self.device, dtype=F64).clone().contiguous().view(-1))
        w = w.to(device=self.device, dtype=F64).contiguous().view(-1)
        hist = torch.full((max(max_iter, 1),), float("nan"), dtype=F64, device=self.device) if history else None
        h = ctypes.c_void_p()
        self.create_context(b, x, w, mode, tol, eps, hist, hist.numel() if hist is not None else 0,
                            C.stream(self.device), h)
        try:
            it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
            C.check(lib.fem_pcg_solve(h, int(max_iter), int(chunk), ctypes.byref(it), ctypes.byref(stt),
                                      ctypes.byref(rz)), "fem_pcg_solve")
            sc = (ctypes.c_double * 6)()
            C.check(lib.fem_pcg_scalars(h, sc), "fem_pcg_scalars")
            ran = int(lib.fem_pcg_get_schedule(h))
            _check_sync(stt.value)
        finally:
            lib.fem_pcg_destroy(h)
        if hist is not None:
            hist = hist[: min(it.value, hist.numel())]
        return PcgResult(x, it.value, stt.value, rz.value, sc[1], hist, ran)

    def close(self):
        if getattr(self, "h", None):
            C.lib().fem_mf_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_sync(status):
    if status == C.PCG_SYNC_TIMEOUT:
        raise RuntimeError("persistent PCG: an in-launch wait gave up (grid synchronisation timed out); "
                           "the iterate is not meaningful")


class _DistMarker:
    """Mixin marking distributed runners (they run the 3-kernel schedule)."""


@_scoped
class PcgRunner:
    """Persistent (P)CG context for fixed-iteration timing (bench.py): start once, iterate k, poll."""

    def __init__(self, A: SellMatrix, b, w, x0=None, mode=C.MODE_PCG, tol=0.0, eps=1e-30, fused=False,
                 schedule=None, constraints=None, tune=None):
        """tune: the context's FEM_TUNE_* flags instead of the library default (e.g. TUNE_DEFAULT | TUNE_PK_GV)."""
        self.lib = C.lib()
        self.A = A
        self.device = A.device
        self.b = b.to(device=A.device, dtype=F64).contiguous().view(-1)
        self.w = w.to(device=A.device, dtype=F64).contiguous().view(-1)
        self.x = (torch.zeros(A.n, dtype=F64, device=A.device) if x0 is None
                  else x0.to(device=A.device, dtype=F64).clone().contiguous().view(-1))
        # a dedicated stream: hipGraph capture is not allowed on the legacy default stream
        self.stream = torch.cuda.Stream(device=A.device)
        self.stream.wait_stream(torch.cuda.current_stream(A.device))
        self.h = ctypes.c_void_p()
        if getattr(A, "is_matfree", False):   # one form only: refuse what it would otherwise ignore
            if constraints is not None:
                raise ValueError("the element-chunk operator has no constrained CG (constraints= needs a SellMatrix)")
            if fused or (schedule is not None and int(schedule) not in (SCHED_THREE, SCHED_AUTO)):
                raise ValueError("the element-chunk operator runs the three-kernel schedule (no fused / deferred / "
                                 "persistent form)")
        self.schedule = (0 if isinstance(self, _DistMarker) or getattr(A, "is_matfree", False)
                         else _schedule(fused, schedule, A.bs))
        self.constraints = constraints   # keeps the device arrays alive with the context
        self._mode, self._tol, self._eps = mode, float(tol), float(eps)
        # solver-layout values (bs = 1) unless the context must read the plain ones (distributed, fused, constrained)
        self._create(isinstance(self, _DistMarker) or self.schedule == SCHED_FUSED or constraints is not None)
        if tune is not None:
            self.set_tuning(tune)

    def _create(self, plain):
        A = self.A
        if getattr(A, "is_matfree", False):
            A.create_context(self.b, self.x, self.w, self._mode, self._tol, self._eps, None, 0,
                             ctypes.c_void_p(self.stream.cuda_stream), self.h)
            self._sl = False
            self.stream.wait_stream(torch.cuda.current_stream(A.device))
            return
        C.check(self.lib.fem_pcg_create(A.g.n_nodes, A.bs, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols),
                                        A.solver_vals_ptr(plain), C.ptr(self.b), C.ptr(self.x), C.ptr(self.w),
                                        self._mode, self._tol, self._eps, None, 0,
                                        ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(self.h)),
                "fem_pcg_create")
        C.check(self.lib.fem_pcg_set_schedule(self.h, self.schedule), "fem_pcg_set_schedule")
        C.check(self.lib.fem_pcg_set_entries(self.h, A.g.sell_entries), "fem_pcg_set_entries")
        A.attach_cols16(self.h)
        A.attach_layout(self.h, plain)
        self._sl = A.solver_layout and not plain
        if self.constraints is not None:
            C.check(self.lib.fem_pcg_set_constraints(self.h, *self.constraints.args()), "fem_pcg_set_constraints")
        # the setup above may enqueue work on the current stream that this context's stream reads: the solver
        # layout formed on first use (paired deltas, uniform lists, gather windows), the plain values formed back
        self.stream.wait_stream(torch.cuda.current_stream(A.device))

    def set_tuning(self, flags):
        if self._sl and not (int(flags) & 2):   # no FEM_TUNE_PAIR: a context over the plain values instead
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()
            self._create(True)
        C.check(self.lib.fem_pcg_set_tuning(self.h, int(flags)), "fem_pcg_set_tuning")

    def finish(self):
        C.check(self.lib.fem_pcg_finish(self.h), "fem_pcg_finish")

    def start(self):
        C.check(self.lib.fem_pcg_start(self.h), "fem_pcg_start")

    def use_graph(self, k):
        C.check(self.lib.fem_pcg_use_graph(self.h, int(k)), "fem_pcg_use_graph")

    def iterate(self, k):
        C.check(self.lib.fem_pcg_iterate(self.h, int(k)), "fem_pcg_iterate")

    def poll(self):
        it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        C.check(self.lib.fem_pcg_poll(self.h, ctypes.byref(it), ctypes.byref(stt), ctypes.byref(rz)), "fem_pcg_poll")
        _check_sync(stt.value)
        return it.value, stt.value, rz.value

    def debug_window(self, L, lo, hi):
        """Test-only fault injection: overwrite logical workgroup L's gather window (after start())."""
        C.check(self.lib.fem_pcg_debug_window(self.h, int(L), int(lo), int(hi)), "fem_pcg_debug_window")

    def effective_schedule(self):
        """The schedule the context runs (after start(): SCHED_PERSIST may have fallen back to SCHED_DEFERRED)."""
        return int(self.lib.fem_pcg_get_schedule(self.h))

    def uniform_slices(self, s_begin=0, s_end=-1):
        """(slices stored with slice-uniform deltas, slices, column-index bytes per SpMV) over the slices
        [s_begin, s_end) of the context's matrix copy (after start())."""
        return uniform_slices(self.lib, self.h, s_begin, s_end)

    def offdiag_slices(self):
        """(slices whose diagonal the persistent launches keep on chip, slices, value bytes left out per iteration)
        of the started context (include/fem355.h FEM_TUNE_PK_OFFDIAG); zeros when it reads the full values."""
        c, n, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        C.check(self.lib.fem_pcg_offdiag_slices(self.h, ctypes.byref(c), ctypes.byref(n), ctypes.byref(nb)),
                "fem_pcg_offdiag_slices")
        return c.value, n.value, nb.value

    def debug_offdiag_values(self):
        """Test-only: the plain SELL values rebuilt from the started context's diagonal-free stream and diagonal."""
        A = self.A
        out = torch.empty(max(A.g.sell_entries, 1), dtype=F64, device=A.device)
        C.check(self.lib.fem_pcg_debug_offdiag(self.h, C.ptr(A.g.rowptr), C.ptr(out)), "fem_pcg_debug_offdiag")
        return out

    def desc_slices(self):
        """(slices the persistent launches read from descriptor records, slices) of the started context
        (include/fem355.h FEM_TUNE_PK_DESC); (0, slices) when its build reads no records."""
        c, n = ctypes.c_int64(), ctypes.c_int64()
        C.check(self.lib.fem_pcg_desc_slices(self.h, ctypes.byref(c), ctypes.byref(n)), "fem_pcg_desc_slices")
        return c.value, n.value

    def debug_desc_records(self):
        """Test-only: the started context's descriptor records, an int32 tensor [slices, 16] on the host (word layout:
        csrc/sell_pair.hpp PkDesc)."""
        out = torch.empty((max(self.A.g.slice_ptr.numel() - 1, 0), 16), dtype=torch.int32)
        C.check(self.lib.fem_pcg_debug_desc(self.h, ctypes.c_void_p(out.data_ptr())), "fem_pcg_debug_desc")
        return out

    def pipelined(self):
        """True when the started context runs the pipelined persistent iteration (tune |= TUNE_PK_GV; bs = 1, single
        GPU, PCG mode, at most 2 slices per wave -- include/fem355.h FEM_TUNE_PK_GV)."""
        on = ctypes.c_int()
        C.check(self.lib.fem_pcg_pipelined(self.h, ctypes.byref(on)), "fem_pcg_pipelined")
        return bool(on.value)

    def persist_granules(self):
        """True when the started context's persistent launches reduce d and g through tagged granules
        (include/fem355.h FEM_TUNE_PK_GRAN), False on the counter barrier."""
        on = ctypes.c_int()
        C.check(self.lib.fem_pcg_persist_granules(self.h, ctypes.byref(on)), "fem_pcg_persist_granules")
        return bool(on.value)

    def persist_build(self):
        """(register slots per wave, overflow build, packed slices per wave) of the persistent launches (after
        start(); zeros when the context does not run schedule 3)."""
        sl, ov, pk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        C.check(self.lib.fem_pcg_persist_build(self.h, ctypes.byref(sl), ctypes.byref(ov), ctypes.byref(pk)),
                "fem_pcg_persist_build")
        return sl.value, ov.value, pk.value

    def profile(self, k, every=1):
        """k iterations with hip events around the kernels of every `every`-th one -> (ms sums, counts)."""
        ms = (ctypes.c_double * 3)()
        n = (ctypes.c_int * 3)()
        C.check(self.lib.fem_pcg_profile(self.h, int(k), int(every), ms, n), "fem_pcg_profile")
        return list(ms), list(n)

    def close(self):
        if self.h:
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ============================================================================ transient dynamics (csrc/transient.hip)
def newmark_constants(dt, beta=0.25, gamma=0.5, damping=(0.0, 0.0)):
    """The constants of a Newmark-beta step of M a + C v + K u = f with C = alpha M + beta_R K, damping = (alpha,
    beta_R): a0..a5, the factors of K_eff = cK K + cM M, and `coef`, the 12 values fem_newmark_update takes
    (include/fem355.h). ValueError unless dt > 0, beta > 0, gamma >= 1/2 and both damping factors are >= 0 -- no device
    call. A conditionally stable pair (2 beta < gamma) is accepted: dt is then the caller's business."""
    dt, beta, gamma = float(dt), float(beta), float(gamma)
    if not dt > 0.0:
        raise ValueError(f"Newmark: dt must be > 0, got {dt}")
    if not beta > 0.0 or not gamma >= 0.5:
        raise ValueError(f"Newmark: needs beta > 0 and gamma >= 1/2 (the explicit beta = 0 scheme is out of scope), "
                         f"got beta = {beta}, gamma = {gamma}")
    try:
        alpha, beta_r = (float(d) for d in damping)
    except (TypeError, ValueError):
        raise ValueError(f"Newmark: damping must be the pair (alpha, beta_R), got {damping!r}") from None
    if not alpha >= 0.0 or not beta_r >= 0.0:
        raise ValueError(f"Newmark: the Rayleigh factors must be >= 0, got alpha = {alpha}, beta_R = {beta_r}")
    a0, a1, a2 = 1.0 / (beta * dt * dt), gamma / (beta * dt), 1.0 / (beta * dt)
    a3, a4, a5 = 1.0 / (2.0 * beta) - 1.0, gamma / beta - 1.0, 0.5 * dt * (gamma / beta - 2.0)
    c = dict(dt=dt, beta=beta, gamma=gamma, alpha=alpha, beta_r=beta_r, a0=a0, a1=a1, a2=a2, a3=a3, a4=a4, a5=a5,
             cK=1.0 + a1 * beta_r, cM=a0 + a1 * alpha)
    c["coef"] = [a0, a2, a3, dt * (1.0 - gamma), dt * gamma,
                 a0 + alpha * a1, a2 + alpha * a4, a3 + alpha * a5,
                 beta_r * a1, beta_r * a4, beta_r * a5, dt]
    return c


@dataclass
class TransientResult:
    """NewmarkIntegrator.run: what happened step by step. Entry 0 of the recorded rows and of `times` is the start."""
    times: torch.Tensor            # [steps done + 1] (host)
    iterations: list               # PCG iterations of every step tried (the stopped one included)
    status: list                   # _capi.PCG_* of every step tried
    steps_done: int                # steps whose solve converged
    rec_u: torch.Tensor = None     # [steps done + 1, len(record)] (device): the recorded dofs
    rec_v: torch.Tensor = None
    rec_a: torch.Tensor = None
    energy_steps: list = None      # the steps whose energy was taken (0, energy_every, ...)
    energies: torch.Tensor = None  # [len(energy_steps)] (host): u^T K u / 2 + v^T M v / 2

    @property
    def converged(self):
        return all(s == C.PCG_CONVERGED for s in self.status)


@_scoped
class NewmarkIntegrator:
    """Implicit Newmark-beta integration of M a + C v + K u = f(t), C = alpha M + beta_R K, on an assembled K (`A`) and
    a mass as in SellMatrix.matvec_km_multi (M_s (x) I_bs on the same Graph, or a lumped diagonal).
    Set-up forms K_eff = cK K + cM M once, in the layout the solver reads (scaled_add_mass), its Jacobi weights with
    zeros on the dofs of `fixed_mask` (uint8 [n]; u, v, a stay zero there, no row is eliminated), and ONE PCG context
    over fixed b and x buffers. A step is one pattern sweep for the right-hand side (fem_newmark_rhs), one
    fem_pcg_solve on that context warm-started from u_n (`predictor`: from u_n + dt v_n) and one fused vector kernel
    (fem_newmark_update). With K_eff in layout A the context converts nothing per step; with plain values (bs = 1,
    FEM355_SL=0, int32 columns) its paired copy is rebuilt at every start.
    `tol` is absolute on sqrt(r.z); `rtol`, when given, sets every step's tolerance to rtol sqrt(b.(w o b)) of that
    step's right-hand side (one extra device-to-host read per step). A step whose solve does not end converged leaves
    the state at the step before."""

    def __init__(self, A: SellMatrix, mass, fixed_mask, dt, beta=0.25, gamma=0.5, damping=(0.0, 0.0), tol=1e-8,
                 rtol=None, max_iter=1000, schedule=None, predictor=False, chunk=32):
        self.c = newmark_constants(dt, beta, gamma, damping)
        self.form, mass = A._mass_form("NewmarkIntegrator", mass)
        if rtol is not None and not float(rtol) > 0.0:
            raise ValueError(f"NewmarkIntegrator: rtol must be > 0, got {rtol}")
        self.lib = C.lib()
        self.A, self.mass, self.device = A, mass, A.device
        self.tol, self.rtol, self.max_iter, self.chunk = float(tol), rtol, int(max_iter), int(chunk)
        self.predictor = bool(predictor)
        self.events = None               # a list: step() appends its four torch events (rhs | solve | update)
        dev, n = A.device, A.n
        self._mv = A._mass_values(self.form, mass)
        self._kv, self._la = A._held_values()
        self.Keff = A.scaled_add_mass(mass, self.c["cK"], self.c["cM"])
        fixed_mask = fixed_mask.to(device=dev, dtype=torch.uint8).contiguous().view(-1)
        if fixed_mask.numel() != n:
            raise ValueError(f"NewmarkIntegrator: fixed_mask must hold {n} values, got {fixed_mask.numel()}")
        self.fixed_mask = fixed_mask
        self.w = self.Keff.jacobi(fixed_mask)
        self.free = self.w != 0
        z = lambda *s: torch.zeros(s, dtype=F64, device=dev)
        self.b, self.x, self.u, self.v, self.a, self.Y = z(n), z(n), z(n), z(n), z(n), z(n, 2)
        self._coef = (ctypes.c_double * 12)(*self.c["coef"])
        self.t, self.step_no = 0.0, 0
        self.h = ctypes.c_void_p()
        K = self.Keff
        self.schedule = _schedule(False, schedule, K.bs)
        plain = self.schedule == SCHED_FUSED
        self._stream = C.stream(dev)
        C.check(self.lib.fem_pcg_create(K.g.n_nodes, K.bs, C.ptr(K.g.slice_ptr), C.ptr(K.g.cols),
                                        K.solver_vals_ptr(plain), C.ptr(self.b), C.ptr(self.x), C.ptr(self.w),
                                        C.MODE_PCG, self.tol, 1e-30, None, 0, self._stream, ctypes.byref(self.h)),
                "fem_pcg_create")
        C.check(self.lib.fem_pcg_set_schedule(self.h, self.schedule), "fem_pcg_set_schedule")
        C.check(self.lib.fem_pcg_set_entries(self.h, K.g.sell_entries), "fem_pcg_set_entries")
        K.attach_cols16(self.h)
        K.attach_layout(self.h, plain)

    # -------------------------------------------------------------- start
    def _vec(self, x, what):
        if x is None:
            return torch.zeros(self.A.n, dtype=F64, device=self.device)
        x = x.to(device=self.device, dtype=F64).reshape(-1)
        if x.numel() != self.A.n:
            raise ValueError(f"NewmarkIntegrator: {what} must hold {self.A.n} values, got {x.numel()}")
        return x

    def _mass_times(self, x):
        if self.form == C.MASS_DIAG:
            return self._mv * x
        bs, N = self.A.bs, self.A.g.n_nodes
        return self.mass.matvec_multi(x.view(N, bs).contiguous()).reshape(-1)

    def start(self, u0=None, v0=None, f0=None):
        """Set the state at t = 0: u0, v0 (zeroed on the fixed dofs) and a_0 = M^-1 (f0 - C v0 - K u0) on the free
        dofs -- a division for the diagonal mass, Mg.pcg_multi over the bs components (rtol 1e-12 of each column's own
        sqrt(r0.z0)) for the SELL mass, whose fixed dofs must then be whole nodes."""
        A, c, free = self.A, self.c, self.free
        u0, v0, f0 = self._vec(u0, "u0") * free, self._vec(v0, "v0") * free, self._vec(f0, "f0")
        r = f0 - A.matvec(u0 + c["beta_r"] * v0)
        if c["alpha"] != 0.0:
            r = r - c["alpha"] * self._mass_times(v0)
        r = r * free
        if self.form == C.MASS_DIAG:
            a0 = torch.where(free, r / self._mv, torch.zeros_like(r))
        else:
            bs, N = A.bs, A.g.n_nodes
            fm = self.fixed_mask.view(N, bs)
            if bs > 1 and bool((fm != fm[:, :1]).any()):
                raise ValueError("NewmarkIntegrator: with the SELL mass a node is fixed in all its components or none")
            wm = self.mass.jacobi(fm[:, 0].contiguous())
            R = r.view(N, bs).contiguous()
            nrm = torch.sqrt((R * (wm[:, None] * R)).sum(0)).cpu()
            a0 = torch.zeros_like(R)
            nz = [j for j in range(bs) if float(nrm[j]) > 0.0]   # a zero column has a_0 = 0 (and no search direction)
            if nz:
                res = self.mass.pcg_multi(R[:, nz].contiguous(), None, w=wm, mode=C.MODE_PCG,
                                          tol=[1e-12 * float(nrm[j]) for j in nz], max_iter=10000)
                if any(s != C.PCG_CONVERGED for s in res.status):
                    raise C.FemError(f"NewmarkIntegrator: the mass solve for a_0 stopped with status {res.status}")
                a0[:, nz] = res.x
            a0 = a0.reshape(-1) * free
        self.u.copy_(u0)
        self.v.copy_(v0)
        self.a.copy_(a0)
        k = c["coef"]
        self.Y[:, 1] = k[5] * self.u + k[6] * self.v + k[7] * self.a
        self.Y[:, 0] = k[8] * self.u + k[9] * self.v + k[10] * self.a
        self.x.copy_(self.u + c["dt"] * self.v if self.predictor else self.u)
        self.t, self.step_no = 0.0, 0
        return self

    # -------------------------------------------------------------- one step
    def rhs(self, F=None, amp=1.0):
        """b <- amp F + M yM + K yK (the K stream is read only with stiffness damping)."""
        A = self.A
        if F is not None and (not F.is_cuda or F.dtype != F64 or F.numel() != A.n or not F.is_contiguous()):
            raise ValueError(f"NewmarkIntegrator: F must be a contiguous fp64 device tensor of {A.n} values")
        cols, dcols = A._multi_cols()
        kv = C.ptr(self._kv) if self.c["beta_r"] != 0.0 else None
        C.check(self.lib.fem_newmark_rhs(A.g.n_nodes, A.bs, self._la, C.ptr(A.g.slice_ptr), cols, dcols, kv,
                                         C.ptr(self._mv), self.form, float(amp), C.ptr(F), C.ptr(self.Y),
                                         C.ptr(self.b), self._stream), "fem_newmark_rhs")

    def update(self):
        C.check(self.lib.fem_newmark_update(self.A.n, self._coef, 1 if self.predictor else 0, C.ptr(self.x),
                                            C.ptr(self.u), C.ptr(self.v), C.ptr(self.a), C.ptr(self.w), C.ptr(self.Y),
                                            self._stream), "fem_newmark_update")

    def step(self, F=None, amp=1.0):
        """Advance to t + dt under the load amp F at the NEW time -> (PCG iterations, status). A solve that does not end
        converged leaves u, v, a and t at the step before."""
        ev = None
        if self.events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        self.rhs(F, amp)
        if ev:
            ev[1].record()
        zero = False
        if self.rtol is not None:
            bn = float(torch.sqrt(torch.dot(self.b, self.w * self.b)))
            zero = bn == 0.0   # nothing moves and nothing pushes: u_new = 0
            if not zero:
                C.check(self.lib.fem_pcg_set_tol(self.h, float(self.rtol) * bn), "fem_pcg_set_tol")
        it, stt, rz = ctypes.c_int(0), ctypes.c_int(C.PCG_CONVERGED), ctypes.c_double()
        if zero:
            self.x.zero_()
        else:
            C.check(self.lib.fem_pcg_solve(self.h, self.max_iter, self.chunk, ctypes.byref(it), ctypes.byref(stt),
                                           ctypes.byref(rz)), "fem_pcg_solve")
            _check_sync(stt.value)
        if ev:
            ev[2].record()
        if stt.value != C.PCG_CONVERGED:
            self.x.copy_(self.u + self.c["dt"] * self.v if self.predictor else self.u)
            return it.value, stt.value
        self.update()
        if ev:
            ev[3].record()
            self.events.append(ev)
        self.step_no += 1
        self.t = self.step_no * self.c["dt"]
        return it.value, stt.value

    # -------------------------------------------------------------- a whole run
    def run(self, steps, load=None, record=None, energy_every=0, callback=None):
        """`steps` steps from the started state. load(k) -> (F or None, amp) gives the load at step k = 1..steps (F a
        contiguous fp64 device tensor [n]). record: dof indices (device int64) whose u, v, a are kept per step.
        energy_every = m > 0: the energy at steps 0, m, 2m, ... (read back once, at the end). callback(step, t, u, v,
        a) gets the device state itself (views, not copies). A step that does not converge stops the run and prints
        `Transient solver: step k stopped with status S after N iterations`. Returns a TransientResult."""
        its, stts, recs, en, en_steps = [], [], [], [], []

        def keep(k):
            if record is not None:
                recs.append(torch.stack((self.u[record], self.v[record], self.a[record])))
            if energy_every and k % energy_every == 0:
                en.append(self.A.quadforms(self.mass, self.u, self.v))
                en_steps.append(k)

        keep(0)
        done = 0
        for k in range(1, int(steps) + 1):
            F, amp = load(k) if load is not None else (None, 0.0)
            it, stt = self.step(F, amp)
            its.append(it)
            stts.append(stt)
            if stt != C.PCG_CONVERGED:
                print(f"Transient solver: step {k} stopped with status {stt} after {it} iterations")
                break
            done = k
            keep(k)
            if callback is not None:
                callback(k, self.t, self.u, self.v, self.a)
        res = TransientResult(torch.arange(done + 1, dtype=F64) * self.c["dt"], its, stts, done)
        if record is not None:
            R = torch.stack(recs)   # [steps + 1, 3, len]
            res.rec_u, res.rec_v, res.rec_a = R[:, 0], R[:, 1], R[:, 2]
        if energy_every:
            res.energy_steps = en_steps
            res.energies = 0.5 * torch.stack(en).sum(1).cpu()
        return res

    def close(self):
        if getattr(self, "h", None):
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ============================================================================ explicit dynamics (csrc/explicit.hip)
XD_OK, XD_INVERTED, XD_DIVERGED = "OK", "INVERTED", "DIVERGED"


def check_explicit_mesh(what, coords, elements, rho, E, nu):
    """The ValueErrors shared by everything explicit -- no device call: c3d4 mesh shapes, rho > 0, E > 0 and nu in
    (-1, 0.5). Returns (N, M)."""
    if not torch.is_tensor(coords) or coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"{what}: coords must be [N, 3], got {tuple(getattr(coords, 'shape', ()))}")
    if not torch.is_tensor(elements) or elements.dim() != 2 or elements.shape[1] != 4:
        raise ValueError(f"{what}: c3d4 connectivity [M, 4] expected, got {tuple(getattr(elements, 'shape', ()))}")
    if not float(rho) > 0.0:
        raise ValueError(f"{what}: rho must be > 0, got {rho}")
    if not float(E) > 0.0:
        raise ValueError(f"{what}: E must be > 0, got {E}")
    if not -1.0 < float(nu) < 0.5:
        raise ValueError(f"{what}: nu must lie in (-1, 0.5), got {nu}")
    return coords.shape[0], elements.shape[0]


def check_explicit_run(what, steps, dt):
    if int(steps) != steps or int(steps) < 0:
        raise ValueError(f"{what}: steps must be an integer >= 0, got {steps}")
    if dt is not None and not float(dt) > 0.0:
        raise ValueError(f"{what}: dt must be > 0, got {dt}")


@dataclass
class ExplicitResult:
    """ExplicitDynamics.run: the run's steps n0 .. n0 + steps - 1 (counted from the start). The recorded rows hold the
    state at the beginning of each step, t = n dt; the state at the end of the run is the integrator's u, v, a."""
    steps_done: int                # steps taken by this run
    status: str                    # XD_OK, XD_INVERTED (an element with det F <= 0) or XD_DIVERGED (a non-finite value)
    stop_step: int                 # the first step (from the start) at which that happened, -1 for XD_OK
    dt: float
    first_step: int = 0            # n0
    rec_u: torch.Tensor = None     # [steps, len(record)] (device)
    rec_v: torch.Tensor = None
    rec_a: torch.Tensor = None
    t_energy: torch.Tensor = None  # [rows] (host): the times of the energy rows (steps n with n % energy_every == 0)
    kinetic: torch.Tensor = None   # sum m v_n^2 / 2
    strain: torch.Tensor = None    # sum V W (u_n)
    ext_power: torch.Tensor = None  # amp_n F . v_n
    ext_work: torch.Tensor = None   # amp_n F . u_n: the work of the load held at its current value (the potential of a
                                    # constant load; kinetic + strain - ext_work is then conserved without damping)
    # with a contact set (ExplicitDynamics.set_contact): rows at the steps n with n % contact_every == 0 ...
    t_contact: torch.Tensor = None       # [rows] (host): their times
    reaction: torch.Tensor = None        # [rows, S, 3] (host): the force on each surface, -sum of what its nodes received
    in_contact: torch.Tensor = None      # [rows, S] int64: nodes with a positive penetration
    penetration: torch.Tensor = None     # [rows, S]: the largest penetration
    # ... and on the energy steps
    contact_energy: torch.Tensor = None  # sum k p^2 / 2, the potential of the normal forces
    friction_power: torch.Tensor = None  # sum f_t . (v_n - w), the rate at which friction dissipates
    surface_power: torch.Tensor = None   # sum f_c . w, the power the moving surfaces put in


class RigidSurface:
    """A rigid analytic surface for ExplicitDynamics.set_contact. kind "plane": `point` on it and `normal`
    pointing into the side the body may occupy; "sphere": centre `point`, `radius`; "cylinder": infinite, `axis` through
    `point`, `radius`. inside=True makes a sphere or cylinder a cavity that holds the body. friction: Coulomb mu >= 0.
    The surface translates by `velocity` (a constant 3-vector: d(t) = velocity t) or by `displacement` (a callable of t
    giving a 3-vector; its velocity during a step is the difference quotient over that step); its orientation is fixed.
    nodes: the ids of the nodes that may touch it (default: all). Every ValueError is raised here or in check_contact,
    before any device call."""

    def __init__(self, kind, point, normal=None, axis=None, radius=None, inside=False, friction=0.0, velocity=None,
                 displacement=None, nodes=None):
        what = "RigidSurface"
        if kind not in C.SURFACE_KINDS:
            raise ValueError(f"{what}: unknown kind {kind!r} (supported: {', '.join(sorted(C.SURFACE_KINDS))})")
        self.kind = kind
        self.point = self._vec3(point, "point")
        direction = {"plane": normal, "cylinder": axis, "sphere": None}[kind]
        self.direction = (0.0, 0.0, 0.0)
        if kind != "sphere":
            name = "normal" if kind == "plane" else "axis"
            if direction is None:
                raise ValueError(f"{what}: a {kind} needs its {name}")
            d = self._vec3(direction, name)
            length = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if not length > 0.0:
                raise ValueError(f"{what}: the {name} must not be zero")
            self.direction = tuple(x / length for x in d)
        self.radius = 0.0
        if kind != "plane":
            if radius is None or not float(radius) > 0.0:
                raise ValueError(f"{what}: a {kind} needs a radius > 0, got {radius}")
            self.radius = float(radius)
        self.inside = bool(inside) and kind != "plane"
        if not float(friction) >= 0.0:
            raise ValueError(f"{what}: friction must be >= 0, got {friction}")
        self.friction = float(friction)
        if velocity is not None and displacement is not None:
            raise ValueError(f"{what}: give velocity or displacement, not both")
        if displacement is not None and not callable(displacement):
            raise ValueError(f"{what}: displacement must be a callable of t")
        self.velocity = None if velocity is None else self._vec3(velocity, "velocity")
        self.displacement = displacement
        self.nodes = None if nodes is None else torch.as_tensor(nodes).to(torch.int64).reshape(-1).cpu()

    @staticmethod
    def _vec3(x, name):
        v = [float(t) for t in (x.reshape(-1).tolist() if torch.is_tensor(x) else x)]
        if len(v) != 3 or not all(math.isfinite(t) for t in v):
            raise ValueError(f"RigidSurface: {name} must hold 3 finite values")
        return tuple(v)

    def offset(self, t):
        """d(t) as 3 floats."""
        if self.displacement is not None:
            return self._vec3(self.displacement(t), "displacement(t)")
        if self.velocity is not None:
            return tuple(w * t for w in self.velocity)
        return (0.0, 0.0, 0.0)

    def step_velocity(self, t0, t1):
        """The velocity of the step t0 -> t1: the constant one, else the difference quotient of d."""
        if self.displacement is None:
            return self.velocity or (0.0, 0.0, 0.0)
        a, b = self.offset(t0), self.offset(t1)
        return tuple((y - x) / (t1 - t0) for x, y in zip(a, b))


def check_contact(what, surfaces, penalty, N, safety=None):
    """The ValueErrors of a contact set -- no device call: at most 8 RigidSurface, node ids in [0, N), 0 < penalty < 4
    and, where the caller takes dt = safety x the guaranteed stable step, penalty <= 4 (1 - safety^2), which keeps
    omega dt <= 2. Returns the list of surfaces."""
    surfaces = list(surfaces)
    if len(surfaces) > C.XD_MAX_SURFACES:
        raise ValueError(f"{what}: at most {C.XD_MAX_SURFACES} surfaces, got {len(surfaces)}")
    for k, s in enumerate(surfaces):
        if not isinstance(s, RigidSurface):
            raise ValueError(f"{what}: surface {k} is not a RigidSurface")
        if s.nodes is not None and s.nodes.numel() and (int(s.nodes.min()) < 0 or int(s.nodes.max()) >= N):
            raise ValueError(f"{what}: surface {k} names a node outside [0, {N})")
    if not 0.0 < float(penalty) < 4.0:
        raise ValueError(f"{what}: penalty must lie in (0, 4), got {penalty}")
    if safety is not None and float(penalty) > 4.0 * (1.0 - float(safety) ** 2) * (1.0 + 1e-12):   # 0.76 at 0.9 passes
        raise ValueError(f"{what}: penalty {penalty} exceeds 4 (1 - safety^2) = {4.0 * (1.0 - float(safety) ** 2):.4g}, "
                         f"the bound that keeps the step safety x the stable one within omega dt <= 2")
    return surfaces


@_scoped
class ExplicitDynamics:
    """Explicit central-difference dynamics of a c3d4 mesh (include/fem355.h fem_xd_*, csrc/explicit.hip):
    M a + alpha M v + f_int(u) = amp(t) F with the lumped mass m_i = sum rho V_e / 4, `damping` = alpha, integrated in
    leapfrog form. A step is one chunk kernel (the internal force of `material` on the MatFreeOperator layout this
    object owns: "linear", "svk" or "neo_hookean") and one vector kernel; nothing is assembled and nothing is solved.
    fixed_mask: uint8 / bool [3N] or [N,3], the dofs held at u = v = a = 0. Uniform rho, E, nu. The step size is the
    caller's: stable_dt() returns a guaranteed bound."""

    def __init__(self, coords, elements, rho, E, nu, material="linear", fixed_mask=None, damping=0.0):
        what = "ExplicitDynamics"
        N, M = check_explicit_mesh(what, coords, elements, rho, E, nu)
        if material not in C.EXPLICIT_MATERIALS:
            raise ValueError(f"{what}: unknown material {material!r} (supported: "
                             f"{', '.join(sorted(C.EXPLICIT_MATERIALS))})")
        if not float(damping) >= 0.0:
            raise ValueError(f"{what}: damping must be >= 0, got {damping}")
        if fixed_mask is not None and (not torch.is_tensor(fixed_mask) or fixed_mask.numel() != 3 * N):
            raise ValueError(f"{what}: fixed_mask must hold {3 * N} values")
        self.lib = C.lib()
        self.material, self.rho, self.E, self.nu, self.damping = material, float(rho), float(E), float(nu), float(damping)
        self.op = MatFreeOperator(coords, elements, "elastic", E, nu)
        self.device, self.N, self.M, self.n = self.op.device, N, M, 3 * N
        dev = self.device
        self.h = ctypes.c_void_p()
        self.mass = torch.zeros(max(N, 1), dtype=F64, device=dev)[:N]
        C.check(self.lib.fem_xd_lumped_mass(self.op.h, self.rho, C.ptr(self.mass), C.stream(dev)), "fem_xd_lumped_mass")
        self.fixed_mask = None if fixed_mask is None else \
            (fixed_mask.to(dev) != 0).to(torch.uint8).contiguous().view(-1)
        z = lambda: torch.zeros(self.n, dtype=F64, device=dev)
        self.u, self.v, self.a = z(), z(), z()
        C.check(self.lib.fem_xd_create(self.op.h, C.EXPLICIT_MATERIALS[material], self.rho, C.ptr(self.mass),
                                       C.ptr(self.fixed_mask), self.damping, C.ptr(self.u), C.ptr(self.v),
                                       C.ptr(self.a), C.stream(dev), ctypes.byref(self.h)), "fem_xd_create")
        self.started = False
        self._surfaces, self._word = [], None
        self._t_base, self._n_base, self._t_dt = 0.0, 0, None   # the time reached is _t_base + _n_base * _t_dt

    def time(self, k=0):
        """The time k steps of the current dt after the state reached (kept on the host: surface motion continues
        across runs and across changes of dt)."""
        return self._t_base + (self._n_base + k) * self._t_dt if self._t_dt else self._t_base

    def set_contact(self, surfaces, penalty=0.5, dt=None):
        """Attach frictional penalty contact with up to 8 rigid surfaces (RigidSurface), or clear it with
        None / []. penalty = kappa: the normal stiffness of node i is kappa m_i / dt^2 with the run's dt; 0 < kappa < 4,
        and kappa <= 4 (1 - s^2) keeps a step of s x stable_dt() stable. Attach before start(): its a_0 then includes
        the contact force at the surfaces' positions at the time reached, with the stiffness of `dt` (default 0.9 x
        stable_dt(); the runs use their own dt)."""
        what = "ExplicitDynamics.set_contact"
        surfaces = check_contact(what, surfaces or [], penalty, self.N)
        if dt is not None and not float(dt) > 0.0:
            raise ValueError(f"{what}: dt must be > 0, got {dt}")
        dev = self.device
        if not surfaces:
            C.check(self.lib.fem_xd_contact(self.h, 0, None, 0.0, 0.0, None, C.stream(dev)), "fem_xd_contact")
            self._surfaces, self._word = [], None
            return self
        if dt is None:
            dt = 0.9 * self.stable_dt()[0]
            if not dt < float("inf"):
                dt = 1.0
        dt, t = float(dt), self.time()
        rows = []
        for s in surfaces:
            d0 = s.offset(t)
            rows += [float(C.SURFACE_KINDS[s.kind]), float(s.inside)] + [c + d for c, d in zip(s.point, d0)] + \
                list(s.direction) + [s.radius, s.friction] + list(s.step_velocity(t, t + dt))
        word = None
        if any(s.nodes is not None for s in surfaces):
            w = torch.zeros(max(self.N, 1), dtype=torch.uint8)
            for k, s in enumerate(surfaces):
                if s.nodes is None:
                    w |= 1 << k
                else:
                    w[s.nodes] |= 1 << k
            word = w.to(dev)
        table = (ctypes.c_double * len(rows))(*rows)
        C.check(self.lib.fem_xd_contact(self.h, len(surfaces), table, float(penalty), dt, C.ptr(word), C.stream(dev)),
                "fem_xd_contact")
        self._surfaces, self._word, self._contact_t0 = surfaces, word, t   # the word array lives as long as the set
        return self

    def _vec(self, x, what, null=True):
        if x is None:
            return None if null else torch.zeros(self.n, dtype=F64, device=self.device)
        x = x.to(device=self.device, dtype=F64).reshape(-1).contiguous()
        if x.numel() != self.n:
            raise ValueError(f"ExplicitDynamics: {what} must hold {self.n} values, got {x.numel()}")
        return x

    def stable_dt(self):
        """(dt, per-element dt [M] on the device): dt = min_e 1 / (c_d sqrt(sum_a |g_a|^2)), c_d^2 = (max(lam, 0) + 2 mu) / rho,
        which is <= 2 / omega_max of the lumped-mass pencil (inf for a mesh of no element)."""
        dev = self.device
        dte = torch.empty(max(self.M, 1), dtype=F64, device=dev)
        out = torch.empty(1, dtype=F64, device=dev)
        C.check(self.lib.fem_xd_stable_dt(C.ptr(self.op.coords), C.ptr(self.op.elements), self.M, self.E, self.nu,
                                          self.rho, C.ptr(dte), C.ptr(out), C.stream(dev)), "fem_xd_stable_dt")
        return float(out.item()), dte[: self.M]

    def internal_force(self, u):
        """f_int(u) [3N] of the material (one chunk kernel and the slot sums); the state is untouched."""
        u = self._vec(u, "u", null=False)
        f = torch.empty(self.n, dtype=F64, device=self.device)
        C.check(self.lib.fem_xd_force(self.h, C.ptr(u), C.ptr(f), C.stream(self.device)), "fem_xd_force")
        return f

    def start(self, u0=None, v0=None, F=None, amp=1.0):
        """Set the state at t = 0: u0, v0 (zero on the fixed dofs) and a_0 = (amp F - f_int(u0)) / m - alpha v0."""
        u0, v0, F = self._vec(u0, "u0"), self._vec(v0, "v0"), self._vec(F, "F")
        C.check(self.lib.fem_xd_start(self.h, C.ptr(u0), C.ptr(v0), C.ptr(F), float(amp), C.stream(self.device)),
                "fem_xd_start")
        self.started = True
        self._t_base, self._n_base, self._t_dt = 0.0, 0, None
        return self

    def status(self):
        """(status, stop_step) since the start; synchronises."""
        w = (ctypes.c_int64 * 2)()
        C.check(self.lib.fem_xd_status(self.h, w, C.stream(self.device)), "fem_xd_status")
        inv, nf = int(w[0]), int(w[1])
        if nf >= 0 and (inv < 0 or nf < inv):
            return XD_DIVERGED, nf
        if inv >= 0:
            return XD_INVERTED, inv
        return XD_OK, -1

    def steps_taken(self):
        w = (ctypes.c_int64 * 4)()
        C.check(self.lib.fem_xd_info(self.h, w), "fem_xd_info")
        return int(w[0])

    def run(self, steps, dt, F=None, amps=1.0, record=None, energy_every=0, contact_every=0):
        """`steps` steps of `dt` from the state reached, all enqueued at once (two launches per step). F [3N]: the load
        pattern (None: no load); amps: a number, or the load factors at the run's times -- steps + 1 values (t_n0 ..
        t_n0+steps; with `steps` values the last is held). record: dof indices whose u, v, a are kept per step;
        energy_every = m > 0: the energies at the steps n with n % m == 0 counted from the start. Consecutive runs
        with the same dt continue the same trajectory bit for bit. With a contact set, contact_every = m > 0 keeps the
        per-surface reaction, contact count and largest penetration at the steps n with n % m == 0, and the energy
        steps also keep the penalty energy, the friction power and the surface power. Returns an ExplicitResult (reads
        the status words back: one synchronisation at the end)."""
        what = "ExplicitDynamics.run"
        check_explicit_run(what, steps, dt)
        steps, dt, every = int(steps), float(dt), int(energy_every)
        if every < 0:
            raise ValueError(f"{what}: energy_every must be >= 0, got {energy_every}")
        cevery = int(contact_every)
        if cevery < 0 or (cevery > 0 and not self._surfaces):
            raise ValueError(f"{what}: contact_every must be >= 0 and needs a contact set, got {contact_every}")
        if not self.started:
            self.start()
        if dt != self._t_dt:   # the time so far is kept; steps are counted anew with this dt
            self._t_base, self._n_base, self._t_dt = self.time(), 0, dt
        dev = self.device
        F = self._vec(F, "F")
        if isinstance(amps, (int, float)):
            al = [float(amps)] * (steps + 1)
        else:
            al = [float(x) for x in (amps.cpu() if torch.is_tensor(amps) else amps)]
            if len(al) == steps and steps > 0:
                al.append(al[-1])
            if len(al) != steps + 1:
                raise ValueError(f"{what}: amps must hold steps + 1 = {steps + 1} values (or steps), got {len(al)}")
        n0 = self.steps_taken()
        res = ExplicitResult(steps, XD_OK, -1, dt, n0)
        nrec, rdofs, inv, ru, rv, ra = 0, None, None, None, None, None
        if record is not None:
            rec = torch.as_tensor(record).to(device=dev, dtype=torch.int64).reshape(-1)
            if rec.numel() and (int(rec.min()) < 0 or int(rec.max()) >= self.n):
                raise ValueError(f"{what}: a recorded dof lies outside [0, {self.n})")
            rdofs, inv = torch.unique(rec, return_inverse=True)   # the kernel takes distinct dofs
            nrec = rdofs.numel()
            ru, rv, ra = (torch.zeros((steps, max(nrec, 1)), dtype=F64, device=dev)[:, :nrec].contiguous()
                          for _ in range(3))
        rows = [n for n in range(n0, n0 + steps) if every and n % every == 0]
        en = torch.zeros((max(len(rows), 1), 4), dtype=F64, device=dev) if every else None
        amp_c = (ctypes.c_double * (steps + 1))(*al)
        S = len(self._surfaces)
        crows = [n for n in range(n0, n0 + steps) if cevery and n % cevery == 0]
        if S and self.n and steps:
            times = [self.time(k) for k in range(steps + 2)]
            t0 = self._contact_t0
            base = [s.offset(t0) for s in self._surfaces]
            off, vel = [], []
            for k in range(steps + 1):
                kv = min(k, steps - 1)   # the closing evaluation takes the last step's velocity
                for s, b in zip(self._surfaces, base):
                    off += [d - c for d, c in zip(s.offset(times[k]), b)]
                    vel += list(s.step_velocity(times[kv], times[kv + 1]))
            off_c, vel_c = (ctypes.c_double * len(off))(*off), (ctypes.c_double * len(vel))(*vel)
            hist = torch.zeros((max(len(crows), 1), S, 5), dtype=F64, device=dev) if cevery else None
            cen = torch.zeros((max(len(rows), 1), 3), dtype=F64, device=dev) if every else None
            C.check(self.lib.fem_xd_run_contact(self.h, steps, dt, amp_c, C.ptr(F), nrec,
                                                C.ptr(rdofs) if nrec else None, C.ptr(ru) if nrec else None,
                                                C.ptr(rv) if nrec else None, C.ptr(ra) if nrec else None, every,
                                                C.ptr(en), off_c, vel_c, cevery, C.ptr(hist), C.ptr(cen),
                                                C.stream(dev)), "fem_xd_run_contact")
            if cevery:
                hc = hist[: len(crows)].cpu()
                res.t_contact = torch.tensor([self.time(n - n0) for n in crows], dtype=F64)
                res.reaction, res.penetration = hc[:, :, :3].clone(), hc[:, :, 4].clone()
                res.in_contact = hc[:, :, 3].round().to(torch.int64)
            if every:
                ce = cen[: len(rows)].cpu()
                res.contact_energy, res.friction_power, res.surface_power = ce[:, 0], ce[:, 1], ce[:, 2]
        elif self.n and steps:
            C.check(self.lib.fem_xd_run(self.h, steps, dt, amp_c, C.ptr(F), nrec, C.ptr(rdofs) if nrec else None,
                                        C.ptr(ru) if nrec else None, C.ptr(rv) if nrec else None,
                                        C.ptr(ra) if nrec else None, every, C.ptr(en), C.stream(dev)), "fem_xd_run")
        elif steps:
            C.check(self.lib.fem_xd_run(self.h, steps, dt, amp_c, None, 0, None, None, None, None, 0, None,
                                        C.stream(dev)), "fem_xd_run")
        if record is not None:
            res.rec_u, res.rec_v, res.rec_a = ru[:, inv], rv[:, inv], ra[:, inv]
        if every:
            e = en[: len(rows)].cpu()
            res.t_energy = torch.tensor(rows, dtype=F64) * dt
            res.kinetic, res.strain, res.ext_power, res.ext_work = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
        res.status, res.stop_step = self.status()
        self._n_base += steps
        return res

    def close(self):
        if getattr(self, "h", None):
            self.lib.fem_xd_destroy(self.h)
            self.h = ctypes.c_void_p()
        if getattr(self, "op", None) is not None:
            self.op.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ============================================================================ nonlinear statics (csrc/nonlinear.hip)
NL_OK,NL_MAX_ITER, NL_LINE_SEARCH_FAILED, NL_LINEAR_SOLVE_FAILED = "OK", "MAX_ITER", "LINE_SEARCH_FAILED", \
    "LINEAR_SOLVE_FAILED"


@dataclass
class NonlinearResult:
    """Outcome of solver.nonlinear_static_solver. The per-step lists have one entry per load step started: the Newton
    iterations taken, and per iteration the residual norm it started from (plus the final one of a converged step),
    the PCG iterations of its linear solve and the accepted step length."""
    u: torch.Tensor
    converged: bool
    status: str                      # NL_OK / NL_MAX_ITER / NL_LINE_SEARCH_FAILED / NL_LINEAR_SOLVE_FAILED
    message: str = ""
    newton_iterations: list = None
    residual_norms: list = None
    pcg_iterations: list = None
    step_lengths: list = None
    # solver.elastoplastic_static_solver only (None elsewhere)
    state: "PlasticState" = None     # committed state after the last converged step
    stress: torch.Tensor = None      # [M,6] at the returned u (xx, yy, zz, xy, yz, xz)
    plastic_fraction: list = None    # per converged step: the share of elements that yielded in it
    failed_step: int = None          # 1-based index in the load path of the step that did not converge


@_scoped
class NewtonStatics:
    """Device state of a geometrically nonlinear c3d4 statics solve: the graph, one bs = 3 SellMatrix that
    every Newton iteration refills in place, the element buffers (forces, energies, packed tangent) and ONE PCG context
    over fixed b / x / w buffers, all allocated once. With the matrix in layout A the context reads the matrix's own
    values (fem_pcg_set_layout) and a refill needs nothing from it; with plain values its paired copy is rebuilt by every
    fem_pcg_start, as for any solve. fixed_mask: uint8 [3 N], 1 on the dofs held at zero."""

    def __init__(self, coords, elements, E, nu, material, fixed_mask, graph: Graph = None):
        if material not in C.MATERIALS:
            raise ValueError(f"Unknown material {material!r} (supported: {', '.join(sorted(C.MATERIALS))}).")
        self._setup(coords, elements, E, nu, fixed_mask, graph)
        self.mat = C.MATERIALS[material]

    def _setup(self, coords, elements, E, nu, fixed_mask, graph):
        """Everything but the material: the graph, the matrix and the buffers (shared with PlasticStatics)."""
        self.lib = C.lib()
        self.device = dev = coords.device
        self.coords = coords.to(F64).contiguous()
        self.elements = elements.to(I64).contiguous()
        if self.elements.dim() != 2 or self.elements.shape[1] != 4:
            raise ValueError(f"NewtonStatics: c3d4 connectivity [M, 4] expected, got {tuple(self.elements.shape)}")
        self.E, self.nu = float(E), float(nu)
        self.N, self.M = self.coords.shape[0], self.elements.shape[0]
        self.g = graph if graph is not None else build_graph(self.elements, self.N)
        self.A = SellMatrix(self.g, 3)
        n = 3 * self.N
        self.mask = fixed_mask.to(device=dev, dtype=torch.uint8).contiguous().view(-1)
        if self.mask.numel() != n:
            raise ValueError(f"NewtonStatics: fixed_mask must hold {n} values, got {self.mask.numel()}")
        e = lambda *s: torch.empty(s, dtype=F64, device=dev)
        self.fe, self.we = e(max(self.M, 1), 4, 3), e(max(self.M, 1))
        self.Kp = e(max(self.M, 1), int(self.lib.fem_ke_sym_stride(4)))
        self.r, self.b, self.x, self.w = e(n), e(n), e(n), e(n)
        self.idx = torch.empty(2, dtype=I64, device=dev)   # (degenerate, inverted) element words of a launch
        self.work = 0.0        # fext . u of the last evaluate (the load's part of the potential)
        self.launches = 0      # fem_tet4_nl launches so far
        self.h = ctypes.c_void_p()
        self._stream = C.stream(dev)
        self._kp_ok = False

    def _vec(self, x, what):
        x = x.to(device=self.device, dtype=F64).contiguous().view(-1)
        if x.numel() != 3 * self.N:
            raise ValueError(f"NewtonStatics: {what} must hold {3 * self.N} values, got {x.numel()}")
        return x

    def _element(self, u, tangent, forces):
        """One element-kernel launch at u: the packed tangent into Kp (tangent) and / or fe, we (forces)."""
        self.idx.fill_(self.M)
        C.check(self.lib.fem_tet4_nl(C.ptr(self.coords), C.ptr(self.elements), self.M, C.ptr(u), self.E, self.nu,
                                     self.mat, 1, C.ptr(self.Kp) if tangent else None,
                                     C.ptr(self.fe) if forces else None, C.ptr(self.we) if forces else None,
                                     None, None, C.ptr(self.idx[0:1]), C.ptr(self.idx[1:2]), self._stream),
                "fem_tet4_nl")
        self.launches += 1

    def evaluate(self, u, load_factor, fext, tangent=False):
        """r = load_factor fext - f_int(u) (0 on the fixed dofs) -> (r, internal energy, ||r||_2, inverted): one
        fem_tet4_nl launch (tangent: also the packed tangent, kept for `tangent()`), one gather, and ONE small
        device-to-host copy for the scalars. r is this object's buffer, overwritten by the next call. inverted: the
        lowest element with det F <= 0, or None (the energy is then +inf). The energies are summed in a fixed order."""
        u, fext = self._vec(u, "u"), self._vec(fext, "fext")
        self._element(u, tangent, True)
        self._kp_ok = bool(tangent)
        C.check(self.lib.fem_tet4_nl_gather(C.ptr(self.fe), C.ptr(self.g.inc_ptr), C.ptr(self.g.inc), self.N,
                                            C.ptr(fext), float(load_factor), C.ptr(self.mask), None, C.ptr(self.r),
                                            self._stream), "fem_tet4_nl_gather")
        s = torch.stack((self.we[: self.M].sum(), torch.dot(self.r, self.r), torch.dot(fext, u),
                         self.idx[0].to(F64), self.idx[1].to(F64))).cpu()
        if int(s[3]) < self.M:
            raise ValueError("Singular matrix encountered while computing B matrix.")
        self.work = float(s[2])
        inv = int(s[4])
        return self.r, float(s[0]), float(s[1]) ** 0.5, (inv if inv < self.M else None)

    def tangent(self, u=None):
        """Refill the matrix with the tangent at u (None: the packed tangent of the last evaluate(..., tangent=True)):
        reset() + add_element_matrices_sym. Returns the SellMatrix."""
        if u is not None or not self._kp_ok:
            if u is None:
                raise ValueError("NewtonStatics.tangent: no tangent evaluated yet; pass u")
            self._element(self._vec(u, "u"), True, False)
        return self._refill()

    def _refill(self):
        """The matrix from the packed tangent in Kp: reset() + add_element_matrices_sym."""
        self._kp_ok = False
        self.A.reset()
        if self.M:
            self.A.add_element_matrices_sym(self.Kp[: self.M], self.elements)
        else:
            self.A.plain_values()
        return self.A

    def jacobi(self):
        """Jacobi weights of the current tangent, zero on the fixed dofs."""
        return self.A.jacobi(self.mask)

    def solve_increment(self, r, w, linear_rtol=1e-6, linear_max_iter=10000, chunk=32):
        """K_T delta = r by MODE_PCG from zero on the kept context, stopped at sqrt(r.z) <= linear_rtol sqrt(r0.z0)
        (solve_tet4's rtol rule) -> (delta, PCG iterations, status). delta is this object's buffer."""
        A = self.A
        self.b.copy_(self._vec(r, "r"))
        self.w.copy_(self._vec(w, "w"))
        self.x.zero_()
        bn = float(torch.sqrt(torch.dot(self.b, self.w * self.b)))
        if not bn > 0.0:
            return self.x, 0, C.PCG_CONVERGED
        if not self.h:
            plain = _schedule(False, None, 3) == SCHED_FUSED
            C.check(self.lib.fem_pcg_create(A.g.n_nodes, 3, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols),
                                            A.solver_vals_ptr(plain), C.ptr(self.b), C.ptr(self.x), C.ptr(self.w),
                                            C.MODE_PCG, 0.0, 1e-30, None, 0, self._stream, ctypes.byref(self.h)),
                    "fem_pcg_create")
            C.check(self.lib.fem_pcg_set_schedule(self.h, _schedule(False, None, 3)), "fem_pcg_set_schedule")
            C.check(self.lib.fem_pcg_set_entries(self.h, A.g.sell_entries), "fem_pcg_set_entries")
            A.attach_cols16(self.h)
            A.attach_layout(self.h, plain)
            self._ctx_sl = A.solver_layout
        elif self._ctx_sl != A.solver_layout:   # the refill must land where the context reads
            raise C.FemError("NewtonStatics: the matrix changed layout under its solver context")
        elif not self._ctx_sl:
            A.plain_values()
        C.check(self.lib.fem_pcg_set_tol(self.h, float(linear_rtol) * bn), "fem_pcg_set_tol")
        it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        C.check(self.lib.fem_pcg_solve(self.h, int(linear_max_iter), int(chunk), ctypes.byref(it), ctypes.byref(stt),
                                       ctypes.byref(rz)), "fem_pcg_solve")
        _check_sync(stt.value)
        return self.x, it.value, stt.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class PlasticState:
    """Material state of an elastoplastic c3d4 mesh, one integration point per element: the plastic strain [M,6]
    (deviatoric; tensor components in the order xx, yy, zz, xy, yz, xz) and the accumulated (equivalent) plastic
    strain [M] >= 0."""
    plastic_strain: torch.Tensor
    equivalent_plastic_strain: torch.Tensor

    @classmethod
    def virgin(cls, M, device="cuda:0"):
        return cls(torch.zeros((int(M), 6), dtype=F64, device=device), torch.zeros(int(M), dtype=F64, device=device))


def check_plastic_material(what, E, nu, yield_stress, hardening):
    """The ValueErrors of the elastoplastic entry points (fem_tet4_j2's FEM_EARG conditions), before any device call."""
    if not float(E) > 0.0:
        raise ValueError(f"{what}: E must be > 0, got {E}")
    if not -1.0 < float(nu) < 0.5:
        raise ValueError(f"{what}: nu must lie in (-1, 0.5), got {nu}")
    if not float(yield_stress) > 0.0:
        raise ValueError(f"{what}: yield_stress must be > 0, got {yield_stress}")
    if not float(hardening) >= 0.0:
        raise ValueError(f"{what}: hardening must be >= 0, got {hardening}")


def check_plastic_state(what, state, M):
    if state is None:
        return
    ep, al = getattr(state, "plastic_strain", None), getattr(state, "equivalent_plastic_strain", None)
    if not torch.is_tensor(ep) or not torch.is_tensor(al) or tuple(ep.shape) != (M, 6) or tuple(al.shape) != (M,):
        raise ValueError(f"{what}: state must be a PlasticState with plastic_strain [{M}, 6] and "
                         f"equivalent_plastic_strain [{M}]")


_UNREACHABLE_YIELD = 1e300


@_scoped
class PlasticStatics(NewtonStatics):
    """Device state of an elastoplastic c3d4 statics solve: NewtonStatics with the J2 return-mapping kernel
    of csrc/plasticity.hip in place of the hyperelastic one, plus two sets of state buffers allocated once. evaluate()
    reads the committed set and writes the trial set, so the trial points of a line search leave no trace; commit()
    swaps the two after a converged load step. The energy evaluate() returns is the incremental potential of the step."""

    def __init__(self, coords, elements, E, nu, yield_stress, hardening, fixed_mask, graph: Graph = None, state=None):
        check_plastic_material("PlasticStatics", E, nu, yield_stress, hardening)
        self._setup(coords, elements, E, nu, fixed_mask, graph)
        check_plastic_state("PlasticStatics", state, self.M)
        self.sigma_y, self.hardening = float(yield_stress), float(hardening)
        m = max(self.M, 1)
        z = lambda *s: torch.zeros(s, dtype=F64, device=self.device)
        self._st = [(z(m, 6), z(m)), (z(m, 6), z(m))]
        self._c = 0               # index of the committed set; the other one takes the trial states
        self._trial_ok = False    # the trial set holds the state of the last evaluate
        self.plastic = torch.zeros(m, dtype=torch.uint8, device=self.device)   # 1 where the last evaluate yielded
        if state is not None and self.M:
            self._st[0][0][: self.M].copy_(state.plastic_strain)
            self._st[0][1][: self.M].copy_(state.equivalent_plastic_strain)

    def _j2(self, u, Kp, fe, we, sigma, trial, plastic, sigma_y=None):
        ep, al = self._st[self._c]
        ep_t, al_t = self._st[1 - self._c] if trial else (None, None)
        self.idx.fill_(self.M)
        C.check(self.lib.fem_tet4_j2(C.ptr(self.coords), C.ptr(self.elements), self.M, C.ptr(u), self.E, self.nu,
                                     self.sigma_y if sigma_y is None else sigma_y, self.hardening, C.ptr(ep),
                                     C.ptr(al), 1, C.ptr(Kp), C.ptr(fe),
                                     C.ptr(we), C.ptr(sigma), C.ptr(ep_t), C.ptr(al_t), C.ptr(plastic),
                                     C.ptr(self.idx[0:1]), self._stream), "fem_tet4_j2")
        self.launches += 1

    def _element(self, u, tangent, forces):
        self._j2(u, self.Kp if tangent else None, self.fe if forces else None, self.we if forces else None, None,
                 forces, self.plastic if forces else None)
        self._trial_ok = self._trial_ok or bool(forces)

    def elastic_tangent(self):
        """Refill the matrix with the elastic tangent (the kernel's tangent under an unreachable yield stress; it does
        not depend on u). The Newton loop takes it in the first iteration of a load step: at the u just committed every
        yielded element has f_tr = 0 up to rounding, so which branch its consistent tangent takes there is noise, and a
        plastic tangent on elements that unload overshoots. Returns the SellMatrix."""
        self._j2(self.x.zero_(), self.Kp, None, None, None, False, None, sigma_y=_UNREACHABLE_YIELD)
        return self._refill()

    def commit(self):
        """The trial state of the last evaluate() becomes the committed state (a swap of the two buffer sets)."""
        if not self._trial_ok:
            raise ValueError("PlasticStatics.commit: no evaluate() since the last commit")
        self._c = 1 - self._c
        self._trial_ok = False

    def state(self):
        """The committed state -> PlasticState (copies)."""
        ep, al = self._st[self._c]
        return PlasticState(ep[: self.M].clone(), al[: self.M].clone())

    def trial_state(self):
        """The state the last evaluate() would commit -> PlasticState (copies)."""
        if not self._trial_ok:
            raise ValueError("PlasticStatics.trial_state: no evaluate() since the last commit")
        ep, al = self._st[1 - self._c]
        return PlasticState(ep[: self.M].clone(), al[: self.M].clone())

    def plastic_fraction(self):
        """Share of the elements that yielded in the last evaluate()."""
        return float(self.plastic[: self.M].to(F64).mean()) if self.M else 0.0

    def stress(self, u):
        """sigma [M,6] at u from the committed state; neither state set is written."""
        out = torch.empty((max(self.M, 1), 6), dtype=F64, device=self.device)
        self._j2(self._vec(u, "u"), None, None, None, out, False, None)
        return out[: self.M]


def assemble_tet4_system(coords, elements, kind="poisson", E=1.0, nu=0.0, graph=None, scale=None):
    """Mesh -> assembled device operator in one pass (pattern + values; element matrices never stored).
    kind: "poisson" (bs=1, kappa=E) or "elastic" (bs=3). scale: per-element factors on K_e (SellMatrix.add_tet4)."""
    n_nodes = coords.shape[0]
    bs = 1 if kind == "poisson" else 3
    if scale is not None:
        scale = check_element_scale("assemble_tet4_system", scale, elements.shape[0], coords.device)
    # bs = 1: the solver layout formed in the pattern's fill pass (the value kernel writes it straight away)
    g = graph if graph is not None else build_graph(elements, n_nodes, solver_layout=bs == 1)
    A = SellMatrix(g, bs).add_tet4(coords.to(F64).contiguous(), elements.contiguous(), E, nu, scale=scale)
    return A


# ============================================================================ geometric multigrid (csrc/multigrid.hip)
MG_COARSE_CAP = 3072   # free dofs of the coarsest level's dense inverse (the m the two-level PCG allows)


def chebyshev_scalars(lmax, degree, boost=1.1, ratio=30.0):
    """(c1 [degree], c2 [degree]) of the Chebyshev smoother on [lmax boost / ratio, lmax boost] in the residual-update
    form d_k = c1[k] d_{k-1} + c2[k] w o r_k: theta, delta the interval's centre and half width, sigma = theta /
    delta, rho_0 = 1 / sigma, rho_k = 1 / (2 sigma - rho_{k-1}); c1[0] = 0, c2[0] = 1 / theta, c1[k] = rho_k rho_{k-1},
    c2[k] = 2 rho_k / delta. Host floats."""
    hi = float(lmax) * float(boost)
    lo = hi / float(ratio)
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    c1, c2 = [0.0], [1.0 / theta]
    for _ in range(1, int(degree)):
        rho_new = 1.0 / (2.0 * sigma - rho)
        c1.append(rho_new * rho)
        c2.append(2.0 * rho_new / delta)
        rho = rho_new
    return c1, c2


def power_start(n, device="cpu"):
    """The power iteration's start vector: a fixed hash of the dof index in (-0.5, 0.5) -- no generator state."""
    i = torch.arange(n, dtype=I64, device=device)
    return ((i * 2654435761) % 4294967296).to(F64) / 4294967296.0 - 0.5


class Multigrid:
    """Geometric multigrid preconditioner on a topology.MeshHierarchy: one assembled SellMatrix per level (for nested
    P1 spaces and a constant material the rediscretised coarse matrix is the Galerkin product), masked Jacobi weights,
    lmax of diag(w) A per level from `eig_iters` power iterations (power_start, the existing SpMV, torch's
    fixed-order sums), the Chebyshev scalars, the child lists of the restriction and the dense inverse of the coarsest
    level's free block. `fixed_mask` [N_fine] bool marks the fixed nodes of the finest level; a node of a lower level
    is fixed iff the finest node it is carried over to is. z = apply(r) is one V(degree, degree) cycle; pcg() is
    MODE_PCG's iteration with that z. `times`: the setup's synchronised wall milliseconds {"assemble", "eig",
    "coarse"}. `assemble(level, coords, elements) -> SellMatrix` replaces assemble_tet4_system (a caller's own element
    matrices or column format). ValueError for a kind other than "poisson" / "elastic", more than MG_COARSE_CAP free dofs on level 0
    and a coarsest matrix that is not positive definite."""

    def __init__(self, hierarchy, kind="elastic", E=1.0, nu=0.0, fixed_mask=None, degree=2, eig_iters=10, boost=1.1,
                 ratio=30.0, assemble=None):
        import time
        if kind not in ("poisson", "elastic"):
            raise ValueError(f"Multigrid: kind must be 'poisson' (bs = 1) or 'elastic' (bs = 3), got {kind!r}")
        if len(hierarchy.levels) < 2:
            raise ValueError("Multigrid: the hierarchy needs at least one refined level")
        if not 1 <= int(degree) <= 8:
            raise ValueError(f"Multigrid: degree 1 to 8, got {degree}")
        self.h = ctypes.c_void_p()
        self.hierarchy, self.kind, self.degree = hierarchy, kind, int(degree)
        self.eig_iters, self.boost, self.ratio = int(eig_iters), float(boost), float(ratio)
        self.bs = bs = 1 if kind == "poisson" else 3
        lv = hierarchy.levels
        self.device = dev = lv[-1].coords.device
        L = len(lv)
        with C.device_scope(dev):
            lib = C.lib()
            Nf = lv[-1].n_nodes
            fixed = (torch.zeros(Nf, dtype=torch.bool, device=dev) if fixed_mask is None
                     else fixed_mask.to(device=dev, dtype=torch.bool).view(-1))
            if fixed.numel() != Nf:
                raise ValueError(f"Multigrid: fixed_mask must hold {Nf} values, got {fixed.numel()}")
            masks = [None] * L
            masks[-1] = fixed
            for l in range(L - 1, 0, -1):   # a carried-over node hands its state down
                p = lv[l].parents.long()
                carried = p[:, 0] == p[:, 1]
                m = torch.zeros(lv[l - 1].n_nodes, dtype=torch.bool, device=dev)
                m[p[carried, 0]] = masks[l][carried]
                masks[l - 1] = m
            free0 = bs * int((~masks[0]).sum())
            if free0 > MG_COARSE_CAP:
                raise ValueError(f"Multigrid: level 0 has {free0} free dofs, the dense coarse solve is capped at "
                                 f"{MG_COARSE_CAP}: start from a coarser mesh or add a level")
            if free0 == 0:
                raise ValueError("Multigrid: level 0 has no free dof")

            def tick():
                torch.cuda.synchronize(dev)
                return time.perf_counter()

            t0 = tick()
            self.A, self.w, self.masks = [], [], masks
            for l in range(L):
                A = (assemble_tet4_system(lv[l].coords, lv[l].elements, kind, E, nu) if assemble is None
                     else assemble(l, lv[l].coords, lv[l].elements))
                if A.bs != bs or A.n_rows != lv[l].n_nodes:
                    raise ValueError(f"Multigrid: level {l} needs a bs = {bs} matrix of {lv[l].n_nodes} block rows")
                A.check_singular()
                A.plain_values()
                mask = torch.zeros((lv[l].n_nodes, bs), dtype=torch.uint8, device=dev)
                mask[masks[l]] = 1
                self.A.append(A)
                self.w.append(A.jacobi(mask.view(-1)))
            t1 = tick()
            self.lmax = [None] + [self._lmax(self.A[l], self.w[l]) for l in range(1, L)]
            c1, c2 = [0.0] * self.degree, [0.0] * self.degree
            for l in range(1, L):
                a, b = chebyshev_scalars(self.lmax[l], self.degree, self.boost, self.ratio)
                c1 += a
                c2 += b
            t2 = tick()
            self.Einv = self._coarse_inverse(self.A[0], masks[0])
            self.child_ptr, self.child = [None], [None]
            for l in range(1, L):
                flat = lv[l].parents.long().view(-1)
                order = torch.sort(flat, stable=True).indices   # by coarse node, the fine ids ascending inside
                self.child.append((order // 2).to(I32).contiguous())
                ptr = torch.zeros(lv[l - 1].n_nodes + 1, dtype=I32, device=dev)
                ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=lv[l - 1].n_nodes), 0).to(I32)
                self.child_ptr.append(ptr)
            t3 = tick()
            self.times = {"assemble": (t1 - t0) * 1e3, "eig": (t2 - t1) * 1e3, "coarse": (t3 - t2) * 1e3}

            def arr(ts):
                return (ctypes.c_void_p * L)(*[None if t is None else t.data_ptr() for t in ts])

            nrows = (ctypes.c_int64 * L)(*[x.n_nodes for x in lv])
            self._c1 = (ctypes.c_double * (L * self.degree))(*c1)
            self._c2 = (ctypes.c_double * (L * self.degree))(*c2)
            self._keep = [A.plain_values() for A in self.A]
            C.check(lib.fem_mg_create(
                L, bs, nrows, arr([A.g.slice_ptr for A in self.A]), arr([A.g.cols for A in self.A]),
                arr([A.g.dcols if A.use16 else None for A in self.A]), arr(self._keep), arr(self.w),
                arr([x.parents for x in lv]), arr(self.child_ptr), arr(self.child), self.degree, self._c1, self._c2,
                bs * lv[0].n_nodes, C.ptr(self.Einv), C.stream(dev), ctypes.byref(self.h)), "fem_mg_create")

    @property
    def fine(self):
        return self.A[-1]

    def _lmax(self, A, w):
        x = power_start(A.n, self.device) * (w != 0).to(F64)
        x = x / torch.sqrt((x * x).sum())
        lam = 0.0
        for _ in range(self.eig_iters):
            y = w * A.matvec(x)
            lam = float((x * y).sum())
            x = y / torch.sqrt((y * y).sum())
        if not lam > 0.0:
            raise ValueError(f"Multigrid: the power iteration gave lmax = {lam} (is the matrix positive definite?)")
        return lam

    def _coarse_inverse(self, A, fixed):
        """[m0, m0]: the inverse of the coarsest matrix on its free dofs (Cholesky on the device, symmetrised), zero
        rows and columns at the fixed ones."""
        dev, bs, N = self.device, self.bs, A.n_rows
        rowptr, colidx, vals = A.csr()
        rows = torch.repeat_interleave(torch.arange(N, device=dev), (rowptr[1:] - rowptr[:-1]).long())
        D = torch.zeros((N, N, bs, bs), dtype=F64, device=dev)
        D[rows, colidx.long()[: rows.numel()]] = vals
        D = D.permute(0, 2, 1, 3).reshape(N * bs, N * bs)
        f = torch.nonzero((~fixed)[:, None].expand(N, bs).reshape(-1)).view(-1)
        Aff = D[f][:, f]
        Aff = 0.5 * (Aff + Aff.T)
        Lc, info = torch.linalg.cholesky_ex(Aff)
        if int(info) != 0 or not bool(torch.isfinite(Lc).all()):
            raise ValueError(f"Multigrid: the coarsest level's matrix is not positive definite on its free dofs "
                             f"(pivot {int(info) - 1}); is the mesh clamped?")
        I = torch.cholesky_solve(torch.eye(f.numel(), dtype=F64, device=dev), Lc)
        Einv = torch.zeros((N * bs, N * bs), dtype=F64, device=dev)
        Einv[f[:, None], f[None, :]] = 0.5 * (I + I.T)
        return Einv.contiguous()

    def _vec(self, v, what):
        v = v.to(device=self.device, dtype=F64).contiguous().view(-1)
        if v.numel() != self.fine.n:
            raise ValueError(f"Multigrid: {what} must hold {self.fine.n} values, got {v.numel()}")
        return v

    def levels_info(self):
        """One dict per level: nodes, elements, dofs, free dofs, lmax of diag(w) A (None on level 0), the column
        format."""
        return [{"level": l, "nodes": A.n_rows, "elements": int(self.hierarchy.levels[l].elements.shape[0]),
                 "dofs": A.n, "free_dofs": int((self.w[l] != 0).sum()), "lmax": self.lmax[l],
                 "columns": "delta16" if A.use16 else "int32"} for l, A in enumerate(self.A)]

    def restrict(self, level, r):
        """P^T (mask o r) from `level` to level - 1 (the restriction kernel alone)."""
        with C.device_scope(self.device):
            A, Ac = self.A[level], self.A[level - 1]
            r = r.to(device=self.device, dtype=F64).contiguous().view(-1)
            if r.numel() != A.n:
                raise ValueError(f"Multigrid.restrict: r must hold {A.n} values, got {r.numel()}")
            rc = torch.empty(Ac.n, dtype=F64, device=self.device)
            C.check(C.lib().fem_mg_restrict(Ac.n_rows, A.n_rows, self.bs, C.ptr(self.child_ptr[level]),
                                            C.ptr(self.child[level]), C.ptr(self.w[level]), C.ptr(r), C.ptr(rc),
                                            C.stream(self.device)), "fem_mg_restrict")
            return rc

    def prolong(self, level, xc, xf=None):
        """xf + mask o P xc from level - 1 to `level` (the prolongation kernel alone; xf defaults to zero)."""
        with C.device_scope(self.device):
            A, Ac = self.A[level], self.A[level - 1]
            xc = xc.to(device=self.device, dtype=F64).contiguous().view(-1)
            if xc.numel() != Ac.n:
                raise ValueError(f"Multigrid.prolong: xc must hold {Ac.n} values, got {xc.numel()}")
            out = (torch.zeros(A.n, dtype=F64, device=self.device) if xf is None
                   else xf.to(device=self.device, dtype=F64).clone().contiguous().view(-1))
            C.check(C.lib().fem_mg_prolong(A.n_rows, Ac.n_rows, self.bs, C.ptr(self.hierarchy.levels[level].parents),
                                           C.ptr(self.w[level]), C.ptr(xc), C.ptr(out), C.stream(self.device)),
                    "fem_mg_prolong")
            return out

    def sweep(self, level=None):
        """One fused Chebyshev sweep on the context's work vectors of `level` (default: the finest) -- for timing the
        kernel; the vectors are scratch that every cycle rewrites."""
        level = len(self.A) - 1 if level is None else int(level)
        with C.device_scope(self.device):
            C.check(C.lib().fem_mg_sweep(self.h, level), "fem_mg_sweep")

    def algorithmic_bytes_sweep(self, level=None):
        """HBM bytes one fused sweep must move: the matrix once (values, column indices, slice pointers, as
        SellMatrix.algorithmic_bytes_spmv counts them) plus seven vectors of the level -- d_old, r, w, x read and r,
        d_new, x written."""
        A = self.A[len(self.A) - 1 if level is None else int(level)]
        return A.algorithmic_bytes_spmv() - 16 * A.n + 7 * 8 * A.n

    def apply(self, r):
        """z = one V-cycle on r."""
        with C.device_scope(self.device):
            r = self._vec(r, "r")
            z = torch.empty_like(r)
            C.check(C.lib().fem_mg_apply(self.h, C.ptr(r), C.ptr(z)), "fem_mg_apply")
            return z

    def pcg(self, b, x0=None, tol=1e-8, max_iter=1000, history=False, chunk=8):
        """PCG on the finest matrix with z = V-cycle(r): MODE_PCG's semantics (stop on sqrt(r.z) < tol, history of
        sqrt(r.z)), PCG_BREAKDOWN on p.Ap <= 0 or non-finite (x untouched by that iteration) and on r.z <= 0 or
        non-finite. Returns a PcgResult."""
        with C.device_scope(self.device):
            lib = C.lib()
            b = self._vec(b, "b")
            x = (torch.zeros_like(b) if x0 is None else self._vec(x0, "x0").clone())
            hist = torch.full((max(max_iter, 1),), float("nan"), dtype=F64, device=self.device) if history else None
            it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
            C.check(lib.fem_mg_solve(self.h, C.ptr(b), C.ptr(x), float(tol), int(max_iter), int(chunk), C.ptr(hist),
                                     hist.numel() if hist is not None else 0, ctypes.byref(it), ctypes.byref(stt),
                                     ctypes.byref(rz)), "fem_mg_solve")
            sc = (ctypes.c_double * 6)()
            C.check(lib.fem_mg_scalars(self.h, sc), "fem_mg_scalars")
            if hist is not None:
                hist = hist[: min(it.value, hist.numel())]
            return PcgResult(x, it.value, stt.value, rz.value, sc[1], hist)

    def close(self):
        if self.h:
            C.lib().fem_mg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ============================================================================ topology optimisation (csrc/topopt.hip)
TOPOPT_OK, TOPOPT_MAX_ITER, TOPOPT_LINEAR_SOLVE_FAILED = "OK", "MAX_ITER", "LINEAR_SOLVE_FAILED"
OC_BISECTIONS = 60


@dataclass
class TopOptResult:
    """Outcome of solver.topology_optimization_solver. density is the last accepted design (the optimiser's variable),
    filtered_density / modulus_scale / u belong to the last design that was solved; the lists have one entry per design
    iteration that finished its linear solve (volume_fraction and change: per update)."""
    density: torch.Tensor
    filtered_density: torch.Tensor
    modulus_scale: torch.Tensor
    u: torch.Tensor
    converged: bool
    status: str                      # TOPOPT_OK / TOPOPT_MAX_ITER / TOPOPT_LINEAR_SOLVE_FAILED
    message: str = ""
    compliance: list = None          # sum_e s_e E ce_e = u^T K(s) u
    load_work: list = None           # F.u (equals the compliance up to the linear solve's error)
    volume_fraction: list = None
    change: list = None              # max |rho_new - rho|
    pcg_iterations: list = None


def check_topopt_parameters(what, volume_fraction, penal, s_min, rho_min, move, filter_passes):
    """The parameter ValueErrors of the topology-optimisation entry points, before any device call."""
    if not 0.0 < float(volume_fraction) <= 1.0:
        raise ValueError(f"{what}: volume_fraction must lie in (0, 1], got {volume_fraction}")
    if not float(penal) >= 1.0:
        raise ValueError(f"{what}: penal must be >= 1, got {penal}")
    if not 0.0 < float(s_min) < 1.0:
        raise ValueError(f"{what}: s_min must lie in (0, 1), got {s_min}")
    if not 0.0 < float(rho_min) < 1.0:
        raise ValueError(f"{what}: rho_min must lie in (0, 1), got {rho_min}")
    if not float(move) > 0.0:
        raise ValueError(f"{what}: move must be > 0, got {move}")
    if int(filter_passes) != filter_passes or int(filter_passes) < 0:
        raise ValueError(f"{what}: filter_passes must be an integer >= 0, got {filter_passes}")


@_scoped
class TopOpt:
    """Device state of a SIMP compliance minimisation on a c3d4 mesh, allocated once: the graph, one bs = 3
    SellMatrix refilled every design iteration by reset() + add_tet4(..., scale=s), the element volumes V and node
    volumes Vn, every element / node work buffer, b / x / w and ONE PCG context over them (the create / attach_cols16 /
    attach_layout / set_tol sequence of NewtonStatics.solve_increment). x is not zeroed between design iterations: each
    solve starts from the previous displacement. fixed_mask: uint8 [3 N], 1 on the dofs held at zero. F: the load
    [N,3]. passive: int8 [M] (0 free, 1 solid, -1 void) or None."""

    def __init__(self, coords, elements, F, fixed_mask, E, nu, volume_fraction, penal=3.0, s_min=1e-3, rho_min=1e-3,
                 filter_passes=1, move=0.2, passive=None, graph: Graph = None):
        check_topopt_parameters("TopOpt", volume_fraction, penal, s_min, rho_min, move, filter_passes)
        self.lib = C.lib()
        self.device = dev = coords.device
        self.coords = coords.to(F64).contiguous()
        self.elements = elements.to(I64).contiguous()
        if self.elements.dim() != 2 or self.elements.shape[1] != 4:
            raise ValueError(f"TopOpt: c3d4 connectivity [M, 4] expected, got {tuple(self.elements.shape)}")
        self.E, self.nu = float(E), float(nu)
        self.volfrac, self.penal, self.s_min, self.rho_min = float(volume_fraction), float(penal), float(s_min), \
            float(rho_min)
        self.passes, self.move = int(filter_passes), float(move)
        self.N, self.M = self.coords.shape[0], self.elements.shape[0]
        n, m = 3 * self.N, max(self.M, 1)
        self.mask = fixed_mask.to(device=dev, dtype=torch.uint8).contiguous().view(-1)
        if self.mask.numel() != n:
            raise ValueError(f"TopOpt: fixed_mask must hold {n} values, got {self.mask.numel()}")
        self.passive = None
        if passive is not None:
            if not torch.is_tensor(passive) or passive.numel() != self.M:
                raise ValueError(f"TopOpt: passive must hold {self.M} values")
            self.passive = passive.to(device=dev, dtype=torch.int8).contiguous().view(-1)
        self.g = graph if graph is not None else build_graph(self.elements, self.N)
        self.A = SellMatrix(self.g, 3)
        e = lambda *s: torch.empty(s, dtype=F64, device=dev)
        self.V, self.Vn = e(m), e(max(self.N, 1))
        self.node_tmp, self.elem_tmp = e(max(self.N, 1)), e(m)
        self.rho_t, self.s, self.ce, self.dct, self.dc, self.rho_new = e(m), e(m), e(m), e(m), e(m), e(m)
        self.work = e(max(int(self.lib.fem_topopt_work_len(self.M)), 1))
        self.out = e(4)                                    # compliance | change, volume fraction | spare
        self.idx = torch.empty(1, dtype=I64, device=dev)   # lowest degenerate element of a launch
        self.b, self.x, self.w = e(n), torch.zeros(n, dtype=F64, device=dev), e(n)
        self.b.copy_(F.to(device=dev, dtype=F64).reshape(-1))
        self.h = ctypes.c_void_p()
        self._stream = C.stream(dev)
        self.idx.fill_(self.M)
        C.check(self.lib.fem_tet4_volumes(C.ptr(self.coords), C.ptr(self.elements), self.M, C.ptr(self.g.inc_ptr),
                                          C.ptr(self.g.inc), self.N, C.ptr(self.V), C.ptr(self.Vn), C.ptr(self.idx),
                                          self._stream), "fem_tet4_volumes")
        if int(self.idx.item()) < self.M:
            raise ValueError("Singular matrix encountered while computing B matrix.")

    def _elem(self, x, what):
        x = x.to(device=self.device, dtype=F64).contiguous().view(-1)
        if x.numel() != self.M:
            raise ValueError(f"TopOpt: {what} must hold {self.M} values, got {x.numel()}")
        return x

    def _filter(self, x, out, adjoint, scale=None):
        C.check(self.lib.fem_density_filter(C.ptr(self.elements), self.M, C.ptr(self.g.inc_ptr), C.ptr(self.g.inc),
                                            self.N, C.ptr(self.V), C.ptr(self.Vn), C.ptr(x), self.passes,
                                            1 if adjoint else 0, self.penal, self.s_min, C.ptr(self.node_tmp),
                                            C.ptr(self.elem_tmp), C.ptr(out), C.ptr(scale), self._stream),
                "fem_density_filter")
        return out

    def filter(self, rho):
        """rho_t = the density filter applied filter_passes times (this object's buffer)."""
        return self._filter(self._elem(rho, "rho"), self.rho_t, False)[: self.M]

    def filter_adjoint(self, g):
        """The transposed filter of an element vector (this object's dc buffer)."""
        return self._filter(self._elem(g, "g"), self.dc, True)[: self.M]

    def scale(self, rho):
        """(rho_t, s): the filtered density and the modulus scale s = s_min + (1 - s_min) rho_t^penal, in one call
        (the scale is fused into the filter's last element kernel). Both are this object's buffers."""
        self._filter(self._elem(rho, "rho"), self.rho_t, False, scale=self.s)
        return self.rho_t[: self.M], self.s[: self.M]

    def solve(self, s, linear_rtol=1e-8, linear_max_iter=10000, chunk=32):
        """K(s) u = F on the free dofs by Jacobi-PCG from the previous u (this object's x, zero at first), stopped at
        sqrt(r.z) <= linear_rtol sqrt(F.w F) -> (u, PCG iterations, status). u is this object's buffer."""
        A = self.A
        A.reset()
        if self.M:
            A.add_tet4(self.coords, self.elements, self.E, self.nu, scale=self._elem(s, "s"))
        else:
            A.plain_values()
        self.w.copy_(A.jacobi(self.mask))   # (a degenerate element was refused when the volumes were formed)
        bn = float(torch.sqrt(torch.dot(self.b, self.w * self.b)))
        if not bn > 0.0:
            raise ValueError("TopOpt: the load is zero on the free dofs")
        if not self.h:
            plain = _schedule(False, None, 3) == SCHED_FUSED
            C.check(self.lib.fem_pcg_create(A.g.n_nodes, 3, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols),
                                            A.solver_vals_ptr(plain), C.ptr(self.b), C.ptr(self.x), C.ptr(self.w),
                                            C.MODE_PCG, 0.0, 1e-30, None, 0, self._stream, ctypes.byref(self.h)),
                    "fem_pcg_create")
            C.check(self.lib.fem_pcg_set_schedule(self.h, _schedule(False, None, 3)), "fem_pcg_set_schedule")
            C.check(self.lib.fem_pcg_set_entries(self.h, A.g.sell_entries), "fem_pcg_set_entries")
            A.attach_cols16(self.h)
            A.attach_layout(self.h, plain)
            self._ctx_sl = A.solver_layout
        elif self._ctx_sl != A.solver_layout:   # the refill must land where the context reads
            raise C.FemError("TopOpt: the matrix changed layout under its solver context")
        elif not self._ctx_sl:
            A.plain_values()
        C.check(self.lib.fem_pcg_set_tol(self.h, float(linear_rtol) * bn), "fem_pcg_set_tol")
        it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        C.check(self.lib.fem_pcg_solve(self.h, int(linear_max_iter), int(chunk), ctypes.byref(it), ctypes.byref(stt),
                                       ctypes.byref(rz)), "fem_pcg_solve")
        _check_sync(stt.value)
        return self.x, it.value, stt.value

    def _energy(self, u, rho_t):
        self.idx.fill_(self.M)
        C.check(self.lib.fem_tet4_unit_energy(C.ptr(self.coords), C.ptr(self.elements), self.M, C.ptr(u), self.nu,
                                              C.ptr(rho_t), self.penal, self.s_min, self.E, C.ptr(self.ce),
                                              C.ptr(self.dct), C.ptr(self.work), C.ptr(self.out[0:1]),
                                              C.ptr(self.idx), self._stream), "fem_tet4_unit_energy")
        self._filter(self.dct, self.dc, True)

    def sensitivities(self, u, rho_t):
        """(dc, compliance): dc = F^T dct with dct[e] = -penal (1 - s_min) rho_t[e]^(penal - 1) E ce[e], the derivative
        of the compliance u^T K(s) u in the design rho at fixed load; dc is this object's buffer."""
        u = u.to(device=self.device, dtype=F64).contiguous().view(-1)
        if u.numel() != 3 * self.N:
            raise ValueError(f"TopOpt: u must hold {3 * self.N} values, got {u.numel()}")
        self._energy(u, self._elem(rho_t, "rho_t"))
        return self.dc[: self.M], float(self.out[0].item())

    def _update(self, rho, dc):
        C.check(self.lib.fem_oc_update(C.ptr(rho), C.ptr(dc), C.ptr(self.V), C.ptr(self.passive), self.M, self.volfrac,
                                       self.move, self.rho_min, OC_BISECTIONS, C.ptr(self.work), C.ptr(self.rho_new),
                                       C.ptr(self.out[1:3]), self._stream), "fem_oc_update")

    def update(self, rho, dc):
        """The optimality-criteria step -> (rho_new, max |rho_new - rho|, reached volume fraction); rho_new is this
        object's buffer."""
        self._update(self._elem(rho, "rho"), self._elem(dc, "dc"))
        o = self.out[1:3].cpu()
        return self.rho_new[: self.M], float(o[0]), float(o[1])

    def step(self, rho, linear_rtol=1e-8, linear_max_iter=10000):
        """One design iteration from rho: filter + scale, refill, solve, sensitivities, OC update, with ONE small
        device-to-host copy after the solve's own -> dict(rho_new, rho_t, s, u, compliance, load_work, change,
        volume_fraction, pcg_iterations, status). After a linear solve that did not converge nothing else is run and
        rho_new is None."""
        rho = self._elem(rho, "rho")
        rho_t, s = self.scale(rho)
        u, it, stt = self.solve(s, linear_rtol, linear_max_iter)
        rec = {"rho_new": None, "rho_t": rho_t, "s": s, "u": u, "pcg_iterations": it, "status": stt}
        if stt != C.PCG_CONVERGED:
            return rec
        self._energy(u, self.rho_t)
        self._update(rho, self.dc)
        self.out[3] = torch.dot(self.b, u)
        o = torch.cat((self.out, self.idx.to(F64))).cpu()
        if int(o[4]) < self.M:
            raise ValueError("Singular matrix encountered while computing B matrix.")
        rec.update(rho_new=self.rho_new[: self.M], compliance=float(o[0]), change=float(o[1]),
                   volume_fraction=float(o[2]), load_work=float(o[3]))
        return rec

    def close(self):
        if getattr(self, "h", None):
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_ceiling(dev, gib=2.0, reps=5):
    """Measured HBM ceilings on this box (report the fraction of the measured STREAM ceiling too):
    16-byte-per-lane read-only sweep and copy over buffers far larger than the 256 MB memory-side cache, best of
    `reps`, timed with hip events on the stream the probes run on."""
    lib = C.lib()
    n = int(gib * (1 << 30) / 8)
    src = torch.ones(n, dtype=torch.float64, device=dev)
    dst = torch.empty(n // 2, dtype=torch.float64, device=dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    res = {}
    for name, fn, nbytes in (("read", lambda: lib.fem_stream_read(C.ptr(src), C.ptr(out), n, 4096, C.stream(dev)), n * 8),
                             ("copy", lambda: lib.fem_stream_copy(C.ptr(src), C.ptr(dst), n // 2, 4096, C.stream(dev)), n * 8)):
        best = None
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            C.check(fn(), "stream probe")
            e1.record(st)
            e1.synchronize()
            t = e0.elapsed_time(e1) * 1e-3
            best = t if best is None else min(best, t)
        res[name] = nbytes / best / 1e9
    del src, dst
    torch.cuda.empty_cache()
    return res
