"""GPU: the dof-level CSR C-ABI named in SURVEY §8(b) (fem_solid_ke, fem_csr_pattern, fem_csr_fill,
fem_spmv_csr, fem_pcg_csr), called through ctypes exactly as a foreign caller would.

Oracle: `oracle.ref_cpu.coo_to_csr` (the reference's COO assembly of `subdivision.ipynb:118-139`, coalesced) and the
golden fixtures of the reference itself. Pattern (rowptr, colidx, diagpos) bit-exact; values 1e-13 relative
(summation order); SpMV 1e-13; solutions 1e-10 relative with iteration counts within ±2; solid K 1e-12.

The second half runs every element family and dpn, seeded non-symmetric K_e, rows of 0 to 64 entries, an exhausted
iteration budget and a matrix too wide for 16-bit column deltas, against `tests/pattern_ref.py`; values there are
held to the rounding bound of two summation orders (`pattern_ref.sum_bound`), not to a relative figure.
"""
import ctypes

import pytest
import torch

import pattern_ref as PR
from conftest import load_golden, rel
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
E, NU = 113.8e9, 0.342
F64, I32 = torch.float64, torch.int32
# Stop of the 36,501-dof PCG case (sqrt(r.z) below it). Chosen from the oracle alone: its own PCG run with two
# summation orders of the operator (element by element, and `R.csr_matvec` on `R.coo_to_csr`) stops at the same
# iteration (511) and the two solutions differ by 2e-13 relative -- 5e-11 at 1e-6, 1e-11 at 1e-8 -- so that the
# 1e-10 solution bound measures the library and not the stopping point.
PCG_TOL_22 = 1e-10


def _lib():
    import fem355  # noqa: F401
    from fem355 import _capi as C
    return C, C.lib()


def _csr(C, lib, tets, N, dpn, dev):
    st = C.stream(dev)
    el = tets.to(dev).long().contiguous()
    rowptr = torch.empty(N * dpn + 1, dtype=I32, device=dev)
    nnz = ctypes.c_int64()
    C.check(lib.fem_csr_pattern(C.ptr(el), el.shape[0], el.shape[1], dpn, N, C.ptr(rowptr), None, None,
                                ctypes.byref(nnz), st), "fem_csr_pattern")
    colidx = torch.empty(nnz.value, dtype=I32, device=dev)
    diag = torch.empty(N * dpn, dtype=I32, device=dev)
    C.check(lib.fem_csr_pattern(C.ptr(el), el.shape[0], el.shape[1], dpn, N, C.ptr(rowptr), C.ptr(colidx),
                                C.ptr(diag), ctypes.byref(nnz), st), "fem_csr_pattern")
    return el, rowptr, colidx, diag


def test_csr_pattern_fill_spmv_vs_reference_coo(gpu):
    C, lib = _lib()
    g = load_golden("tet4_cube_n4_jit")
    N = g["coords"].shape[0]
    el, rowptr, colidx, diag = _csr(C, lib, g["tets"], N, 3, gpu)
    rp_ref, col_ref, val_ref = R.coo_to_csr(g["K"], g["tets"], 3)
    assert torch.equal(rowptr.cpu().long(), rp_ref) and torch.equal(colidx.cpu().long(), col_ref)
    for r in (0, 7, 3 * N - 1):
        assert int(colidx[diag[r]]) == r
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    K = g["K"].to(gpu).contiguous()
    C.check(lib.fem_csr_fill(C.ptr(K), C.ptr(el), el.shape[0], 4, 3, N, C.ptr(rowptr), C.ptr(colidx), C.ptr(vals),
                             C.stream(gpu)), "fem_csr_fill")
    assert rel(vals, val_ref) < 1e-13
    p = g["p"].to(gpu).reshape(-1).contiguous()
    y = torch.empty_like(p)
    C.check(lib.fem_spmv_csr(C.ptr(rowptr), C.ptr(colidx), C.ptr(vals), C.ptr(p), C.ptr(y), 3 * N, C.stream(gpu)),
            "fem_spmv_csr")
    assert rel(y.view(N, 3), g["y"]) < 1e-13


def test_csr_poisson_pattern_dpn1(gpu):
    C, lib = _lib()
    g = load_golden("poisson_tet4_n4_jit")
    N = g["coords"].shape[0]
    _, rowptr, colidx, _ = _csr(C, lib, g["tets"], N, 1, gpu)
    rp_ref, col_ref = R.node_pattern(g["tets"], N)
    assert torch.equal(rowptr.cpu().long(), rp_ref) and torch.equal(colidx.cpu().long(), col_ref)


@pytest.mark.parametrize("mode", ["cg", "pcg"])
def test_pcg_csr_vs_reference(gpu, mode):
    C, lib = _lib()
    g = load_golden("tet4_cube_n4_jit")
    N = g["coords"].shape[0]
    el, rowptr, colidx, _ = _csr(C, lib, g["tets"], N, 3, gpu)
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    K = g["K"].to(gpu).contiguous()
    C.check(lib.fem_csr_fill(C.ptr(K), C.ptr(el), el.shape[0], 4, 3, N, C.ptr(rowptr), C.ptr(colidx), C.ptr(vals),
                             C.stream(gpu)), "fem_csr_fill")
    b = g["F"].to(gpu).reshape(-1).contiguous()
    x = torch.zeros_like(b)
    fixed = torch.zeros((N, 3), dtype=torch.uint8)
    fixed[g["fixed"]] = 1
    fixed = fixed.view(-1).to(gpu)
    it, st = ctypes.c_int(), ctypes.c_int()
    hist = torch.zeros(3000, dtype=F64, device=gpu)
    if mode == "cg":
        C.check(lib.fem_pcg_csr(C.ptr(rowptr), C.ptr(colidx), C.ptr(vals), 3 * N, C.ptr(b), C.ptr(x), None,
                                C.ptr(fixed), float(g["tol"]), 3000, 1e-30, C.MODE_CG_STABLE, ctypes.byref(it),
                                ctypes.byref(st), C.ptr(hist), C.stream(gpu)), "fem_pcg_csr")
        assert st.value == C.PCG_CONVERGED and abs(it.value - int(g["n_cg"])) <= 2
        assert rel(x.view(N, 3), g["u_cg"]) < 1e-10
    else:
        dinv = g["Minv"].to(gpu).reshape(-1).contiguous()
        C.check(lib.fem_pcg_csr(C.ptr(rowptr), C.ptr(colidx), C.ptr(vals), 3 * N, C.ptr(b), C.ptr(x), C.ptr(dinv),
                                None, 1e-6, 3000, 0.0, C.MODE_PCG, ctypes.byref(it), ctypes.byref(st), None,
                                C.stream(gpu)), "fem_pcg_csr")
        assert st.value == C.PCG_CONVERGED and abs(it.value - int(g["n_pcg"])) <= 2
        assert rel(x.view(N, 3), g["u_pcg"]) < 1e-10


@pytest.mark.parametrize("etype,npe", [("c3d8", 8), ("c3d6", 6), ("c3d10", 10)])
def test_solid_ke_vs_reference(gpu, etype, npe):
    C, lib = _lib()
    g = load_golden(f"{etype}_cells")
    X = g["coords"].to(gpu).contiguous()
    el = g["elements"].to(gpu).long().contiguous()
    M = el.shape[0]
    ip = g["points"].to(gpu).contiguous()
    w = g["weights"].to(gpu).contiguous()
    d = 3 * npe
    K1 = torch.empty((M, d, d), dtype=F64, device=gpu)
    C.check(lib.fem_solid_ke(npe, C.ptr(X), C.ptr(el), M, E, NU, C.ptr(ip), C.ptr(w), ip.shape[0], 1, C.ptr(K1),
                             C.stream(gpu)), "fem_solid_ke")
    assert rel(K1, g["K_single"]) < 1e-12
    K0 = torch.empty(g["K_multi"].shape, dtype=F64, device=gpu)
    C.check(lib.fem_solid_ke(npe, C.ptr(X), C.ptr(el), M, E, NU, C.ptr(ip), C.ptr(w), ip.shape[0], 0, C.ptr(K0),
                             C.stream(gpu)), "fem_solid_ke")
    assert rel(K0, g["K_multi"]) < 1e-12
    with pytest.raises(ValueError):
        C.check(lib.fem_solid_ke(20, C.ptr(X), C.ptr(el), M, E, NU, C.ptr(ip), C.ptr(w), ip.shape[0], 1, C.ptr(K1),
                                 C.stream(gpu)), "fem_solid_ke")


def test_scratch_memory_returns_to_baseline(gpu):
    """the library's stream-ordered scratch (graph build temporaries of fem_csr_pattern, the 9 nnz
    staging of fem_csr_fill) comes from a private pool that keeps at most 256 MB across synchronisations, so the
    device's free memory returns to within that of its baseline after a large pattern + fill (a 1.2M-tet elastic
    cube: ~1 GB of temporaries), and fem_release_scratch trims the rest."""
    C, lib = _lib()
    from fem355 import mesh
    c, t = mesh.kuhn_cube(59)
    N = c.shape[0]
    K = torch.randn(t.shape[0], 12, 12, dtype=F64, generator=torch.Generator().manual_seed(1)).to(gpu)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    el, rowptr, colidx, diag = _csr(C, lib, t, N, 3, gpu)
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    C.check(lib.fem_csr_fill(C.ptr(K), C.ptr(el), el.shape[0], 4, 3, N, C.ptr(rowptr), C.ptr(colidx), C.ptr(vals),
                             C.stream(gpu)), "fem_csr_fill")
    torch.cuda.synchronize()
    held = sum(x.numel() * x.element_size() for x in (el, rowptr, colidx, diag, vals))
    del el, rowptr, colidx, diag, vals
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 <= (256 << 20) + (16 << 20), (free0 - free1, held)
    C.check(lib.fem_release_scratch(), "fem_release_scratch")
    torch.cuda.empty_cache()
    free2 = torch.cuda.mem_get_info()[0]
    assert free0 - free2 <= (16 << 20), free0 - free2


# ---------------------------------------------------------------- every element family, non-symmetric K_e, edge rows
def _family(npe, unused=5):
    """A small mesh of the npe-node family with `unused` trailing nodes no element touches -> (connectivity, N)."""
    import fem355  # noqa: F401
    from fem355 import mesh
    c, t = {4: lambda: mesh.kuhn_cube(3), 8: lambda: mesh.hex_box(3), 6: lambda: mesh.wedge_box(3),
            10: lambda: mesh.tet10_cube(2)}[npe]()
    assert t.shape[1] == npe
    return t, c.shape[0] + unused


def _random_ke(t, dpn, seed):
    d = t.shape[1] * dpn
    K = torch.randn(t.shape[0], d, d, dtype=F64, generator=torch.Generator().manual_seed(seed))
    off = (K - K.transpose(1, 2)).abs() + torch.eye(d, dtype=F64)
    assert float(off.min()) > 0                               # no entry equals its transpose
    return K


@pytest.mark.parametrize("npe", [4, 8, 6, 10])
def test_csr_pattern_every_family_and_dpn(gpu, npe):
    """fem_csr_pattern for dpn 1, 2, 3, 6: rowptr / colidx bit-equal to the coalesced COO, diagpos at every row (-1
    on the rows of unused nodes), the sizing call's nnz, and the argument error outside dpn 1..6."""
    C, lib = _lib()
    t, N = _family(npe)
    for dpn in (1, 2, 3, 6):
        rp_ref, ci_ref, _, dpos_ref, _, _ = PR.dof_csr_ref(torch.ones(t.shape[0], npe * dpn, npe * dpn, dtype=F64), t,
                                                           dpn, N)
        el = t.to(gpu).contiguous()
        sized = ctypes.c_int64()
        rowptr0 = torch.empty(N * dpn + 1, dtype=I32, device=gpu)
        C.check(lib.fem_csr_pattern(C.ptr(el), el.shape[0], npe, dpn, N, C.ptr(rowptr0), None, None,
                                    ctypes.byref(sized), C.stream(gpu)), "fem_csr_pattern")
        assert sized.value == ci_ref.numel(), dpn
        _, rowptr, colidx, diag = _csr(C, lib, t, N, dpn, gpu)
        assert torch.equal(rowptr0, rowptr)
        assert torch.equal(rowptr.cpu().long(), rp_ref) and torch.equal(colidx.cpu().long(), ci_ref), dpn
        assert torch.equal(diag.cpu().long(), dpos_ref), dpn
        assert bool((dpos_ref[-5 * dpn:] == -1).all()) and bool((dpos_ref[: -5 * dpn] >= 0).all())
    for dpn in (0, 7):
        rowptr = torch.empty(N * max(dpn, 1) + 1, dtype=I32, device=gpu)
        nnz = ctypes.c_int64()
        rc = lib.fem_csr_pattern(C.ptr(el), el.shape[0], npe, dpn, N, C.ptr(rowptr), None, None, ctypes.byref(nnz),
                                 C.stream(gpu))
        assert rc == C.FEM_EARG, dpn


@pytest.mark.parametrize("npe", [4, 8])
@pytest.mark.parametrize("dpn", [1, 3])
def test_csr_fill_nonsymmetric_ke(gpu, npe, dpn):
    """fem_csr_fill of seeded random, non-symmetric K_e (a row / column swap changes every value). Bound per entry:
    the kernel and the reference each sum the entry's n_e <= n contributions in fp64 in their own order, each within
    (n - 1) 2^-53 S of the exact sum, S the sum of the contributions' magnitudes: |v - v_ref| <= 2 n 2^-53 S. A second
    fill adds onto the stored values: 2 n terms of magnitude sum 2 S against twice the reference, the same bound
    with those figures."""
    C, lib = _lib()
    t, N = _family(npe)
    K = _random_ke(t, dpn, 10 * npe + dpn)
    rp_ref, ci_ref, v_ref, _, mag, cnt = PR.dof_csr_ref(K, t, dpn, N)
    el, rowptr, colidx, _ = _csr(C, lib, t, N, dpn, gpu)
    assert torch.equal(rowptr.cpu().long(), rp_ref) and torch.equal(colidx.cpu().long(), ci_ref)
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    Kd = K.to(gpu).contiguous()
    for k in (1, 2):
        C.check(lib.fem_csr_fill(C.ptr(Kd), C.ptr(el), el.shape[0], npe, dpn, N, C.ptr(rowptr), C.ptr(colidx),
                                 C.ptr(vals), C.stream(gpu)), "fem_csr_fill")
        err = (vals.cpu() - k * v_ref).abs()
        bound = PR.sum_bound(k * mag, k * cnt)
        print(f"fem_csr_fill npe {npe} dpn {dpn} fill {k}: worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (k, float((err / bound).max()))


@pytest.mark.parametrize("npe", [4, 8])
@pytest.mark.parametrize("bs", [1, 3])
def test_stored_ke_assembly_nonsymmetric(gpu, npe, bs):
    """SellMatrix.add_element_matrices of the same random non-symmetric K_e, read back through A.csr(): every value of
    the block CSR against the coalesced COO, within the bound of test_csr_fill_nonsymmetric_ke."""
    from fem355 import system
    t, N = _family(npe)
    K = _random_ke(t, bs, 10 * npe + bs)
    rp_ref, ci_ref, v_ref, _, mag, cnt = PR.dof_csr_ref(K, t, bs, N)
    el = t.to(gpu).contiguous()
    g = system.build_graph(el, N)
    A = system.SellMatrix(g, bs).add_element_matrices(K.to(gpu), el)
    nrp, nci, bv = A.csr()
    nrp, nci, bv = nrp.cpu().long(), nci.cpu().long(), bv.cpu()
    # block entry (i, j)[c, c2] -> dof entry (bs i + c, bs j + c2), in the reference's (row, column) order
    brow = torch.repeat_interleave(torch.arange(N), nrp[1:] - nrp[:-1])
    a = torch.arange(bs)
    rows = (bs * brow[:, None, None] + a[None, :, None]).expand(-1, bs, bs).reshape(-1)
    cols = (bs * nci[:, None, None] + a[None, None, :]).expand(-1, bs, bs).reshape(-1)
    order = torch.argsort(rows * (N * bs) + cols)
    rows_ref = torch.repeat_interleave(torch.arange(N * bs), rp_ref[1:] - rp_ref[:-1])
    assert torch.equal(rows[order], rows_ref) and torch.equal(cols[order], ci_ref)
    err = (bv.reshape(-1)[order] - v_ref).abs()
    bound = PR.sum_bound(mag, cnt)
    print(f"stored-K_e assembly npe {npe} bs {bs}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_spmv_csr_short_and_empty_rows(gpu, n):
    """fem_spmv_csr (8 lanes per row, shuffle tree) on a synthetic CSR: row lengths cycling through 0, 1, 7, 8, 9, 17
    and 64 with random columns. Per row |y - y_ref| <= 2 (len + 8) 2^-53 sum |a| |x|: both sums round every product
    once and add len products (the kernel in 8 partials and a 3-level tree) -- each within (len + 8) 2^-53 of it."""
    C, lib = _lib()
    gen = torch.Generator().manual_seed(100 + n)
    lens = torch.tensor([0, 1, 7, 8, 9, 17, 64])[torch.arange(n) % 7]
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(lens, 0)
    nnz = int(rowptr[-1])
    colidx = torch.randint(0, n, (nnz,), generator=gen)
    vals = torch.randn(nnz, dtype=F64, generator=gen)
    x = torch.randn(n, dtype=F64, generator=gen)
    y_ref = R.csr_matvec(rowptr, colidx, vals, x)
    mag = R.csr_matvec(rowptr, colidx, vals.abs(), x.abs())
    rp, ci = rowptr.to(I32).to(gpu), torch.cat([colidx, torch.zeros(1, dtype=torch.long)]).to(I32).to(gpu)
    v, xd = torch.cat([vals, torch.zeros(1, dtype=F64)]).to(gpu), x.to(gpu)
    y = torch.full((n,), float("nan"), dtype=F64, device=gpu)
    C.check(lib.fem_spmv_csr(C.ptr(rp), C.ptr(ci), C.ptr(v), C.ptr(xd), C.ptr(y), n, C.stream(gpu)), "fem_spmv_csr")
    err = (y.cpu() - y_ref).abs()
    bound = 2.0 * (lens + 8).to(F64) * 2.0 ** -53 * mag
    assert bool((y.cpu()[lens == 0] == 0).all())
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_pcg_csr_exhausted_budget(gpu):
    """max_iter = 3 on the golden cube: FEM_PCG_MAXITER with 3 iterations, and x the oracle's third PCG iterate (1e-12
    relative, the tolerance of the 10M iterate tests)."""
    C, lib = _lib()
    g = load_golden("tet4_cube_n4_jit")
    N = g["coords"].shape[0]
    el, rowptr, colidx, _ = _csr(C, lib, g["tets"], N, 3, gpu)
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    K = g["K"].to(gpu).contiguous()
    C.check(lib.fem_csr_fill(C.ptr(K), C.ptr(el), el.shape[0], 4, 3, N, C.ptr(rowptr), C.ptr(colidx), C.ptr(vals),
                             C.stream(gpu)), "fem_csr_fill")
    u_ref, it_ref, status = R.pcg(g["K"], g["tets"], g["F"], g["Minv"], tol=0.0, max_iter=3)
    assert it_ref == 3 and status == "max_iter"
    b = g["F"].to(gpu).reshape(-1).contiguous()
    x = torch.zeros_like(b)
    dinv = g["Minv"].to(gpu).reshape(-1).contiguous()
    it, st = ctypes.c_int(), ctypes.c_int()
    C.check(lib.fem_pcg_csr(C.ptr(rowptr), C.ptr(colidx), C.ptr(vals), 3 * N, C.ptr(b), C.ptr(x), C.ptr(dinv), None,
                            0.0, 3, 0.0, C.MODE_PCG, ctypes.byref(it), ctypes.byref(st), None, C.stream(gpu)),
            "fem_pcg_csr")
    assert st.value == C.PCG_MAXITER and it.value == 3
    assert rel(x.view(N, 3), u_ref) < 1e-12


def test_pcg_csr_int32_columns(gpu):
    """A randomly renumbered kuhn_cube(22) elastic case: 36,501 dofs with columns more than 32,767 rows away, so
    fem_pcg_csr keeps its int32 columns. Converges to the oracle's PCG solution (1e-10, iterations within 2)."""
    C, lib = _lib()
    from fem355 import mesh
    c, t = mesh.kuhn_cube(22, jitter=0.1)
    N = c.shape[0]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(11))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    c, t = c[perm], inv[t]
    K = R.tet4_K(c, t, E, NU)
    F, fixed = mesh.cube_elasticity_case(c)
    dinv = R.diag_preconditioner(K, t, N, dpn=3)
    dinv[fixed] = 0.0
    u_ref, it_ref, status = R.pcg(K, t, F, dinv, tol=PCG_TOL_22, max_iter=3000)
    assert status == "converged"
    el, rowptr, colidx, _ = _csr(C, lib, t, N, 3, gpu)
    rp = rowptr.cpu().long()
    rows = torch.repeat_interleave(torch.arange(3 * N), rp[1:] - rp[:-1])
    assert 3 * N == 36501 and int((colidx.cpu().long() - rows).abs().max()) > 32767
    vals = torch.zeros(colidx.numel(), dtype=F64, device=gpu)
    Kd = K.to(gpu).contiguous()
    C.check(lib.fem_csr_fill(C.ptr(Kd), C.ptr(el), el.shape[0], 4, 3, N, C.ptr(rowptr), C.ptr(colidx), C.ptr(vals),
                             C.stream(gpu)), "fem_csr_fill")
    b = F.to(gpu).reshape(-1).contiguous()
    x = torch.zeros_like(b)
    w = dinv.to(gpu).reshape(-1).contiguous()
    it, st = ctypes.c_int(), ctypes.c_int()
    C.check(lib.fem_pcg_csr(C.ptr(rowptr), C.ptr(colidx), C.ptr(vals), 3 * N, C.ptr(b), C.ptr(x), C.ptr(w), None,
                            PCG_TOL_22, 3000, 0.0, C.MODE_PCG, ctypes.byref(it), ctypes.byref(st), None,
                            C.stream(gpu)), "fem_pcg_csr")
    assert st.value == C.PCG_CONVERGED and abs(it.value - it_ref) <= 2, (it.value, it_ref)
    assert rel(x.view(N, 3), u_ref) < 1e-10
