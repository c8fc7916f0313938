/*
 * fem355 C-ABI — MI355X (gfx950) FEM assembly + Jacobi-PCG.
 *
 * Drop-in boundary for the hot path of sml2004/CUDA-powered-mesh-handling-and-Iterative-solvers
 * (reference @ 2025-04-18; citations are reference-relative file:line). The reference is pure
 * Python/PyTorch, so its "FFI" is its module-level function surface; each entry point below names the
 * reference function whose device work it replaces. The Python mirror of that surface is
 * `cuda-powered-mesh-handling-and-iterative-solvers_amd/{element,solver}.py` (ctypes, `_capi.py`).
 *
 * Conventions
 *   - every pointer is caller-owned DEVICE memory (torch tensors' data_ptr()), except where marked [host];
 *   - coordinates / values are fp64; connectivity is int64 row-major [M, npe] (torch.long, as the reference);
 *   - graph indices (incidence, CSR/SELL pattern) are int32, offsets into value arrays int64;
 *   - dof = dpn * node + component (`solver/element.py:451`); dpn (= block size bs) is 1 or 3;
 *   - every call is asynchronous on `stream` (a hipStream_t; 0 = legacy default) unless marked [sync];
 *   - return value: FEM_OK or one of the FEM_E* codes; fem_last_error() gives a message.
 *
 * Matrix format (the "ELL-blocked" global matrix): SELL-64 with bs x bs blocks. Rows (nodes) are cut into
 * slices of 64; slice s has width w_s = max row length in the slice; entry (s, k, lane) holds block
 * column cols[slice_ptr[s] + 64*k + lane] and its bs*bs values at
 *   vals[bs*bs*slice_ptr[s] + 64*(bs*bs*k + rc) + lane],  rc = r*bs + c (row-major in the block).
 * Padding entries have col = own row and zero values. Columns of a row are ascending.
 */
#ifndef FEM355_H
#define FEM355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fem_stream_t; /* hipStream_t */

enum {
    FEM_OK = 0,
    FEM_EBADTYPE = 1,   /* unsupported element type  -> ValueError (`solver/element.py:427`) */
    FEM_ESINGULAR = 2,  /* singular element, index in *bad_idx -> ValueError (`solver/element.py:857-858`) */
    FEM_EHIP = 3,       /* HIP runtime error -> RuntimeError */
    FEM_ERCCL = 4,      /* RCCL error -> RuntimeError */
    FEM_EARG = 5,       /* bad argument / capacity exceeded */
    FEM_ESTATE = 6,     /* a device-side invariant was found broken (e.g. FEM_PCG_BAD_WINDOW) -> RuntimeError */
};

/* status words of the (P)CG state, mirrored on the host as the reference's print strings
 * (`solver/solver.py:187-198,210-218,226-227,805-811`) */
enum {
    FEM_PCG_RUNNING = 0,
    FEM_PCG_CONVERGED = 1,
    FEM_PCG_MAXITER = 2,
    FEM_PCG_BREAKDOWN = 3,  /* pAp < eps or pAp < 0  (`solver/solver.py:187-192`) */
    FEM_PCG_ALPHA_NAN = 4,  /* (`solver/solver.py:196-198`) */
    FEM_PCG_BETA_NAN = 5,   /* (`solver/solver.py:214-218`) */
    FEM_PCG_SYNC_TIMEOUT = 6, /* persistent schedule: an in-launch wait gave up (seconds without progress); the
                               * iterate is not meaningful -> RuntimeError */
    FEM_PCG_BAD_WINDOW = 7,   /* persistent / fused schedules: a workgroup's gather window lay outside the u-flag
                               * array (an internal invariant broken upstream). The kernel never indexes past the
                               * array; it ends the launch, and fem_pcg_poll / fem_pcg_solve return FEM_ESTATE */
};

/* CG_CONSTRAINED: constrained_conjugate_gradient_solver / new_constrained_conjugate_gradient_solver
 * (`solver/solver.py:512-600`, `:702-759`): the CG_STABLE arithmetic without zeroing x, plus the projections
 * of fem_pcg_set_constraints after every x update */
enum { FEM_MODE_CG_STABLE = 0, FEM_MODE_PCG = 1, FEM_MODE_CG_CONSTRAINED = 2 };
enum { FEM_KIND_ELASTIC = 0, FEM_KIND_POISSON = 1, FEM_KIND_MASS = 2 };
enum { FEM_ISO_SUM = 0, FEM_ISO_STACK = 1, FEM_ISO_VOLUME = 2, FEM_ISO_MASS = 3 };

const char* fem_last_error(void);                 /* [host] message of the last failing call */
int fem_version(void);                            /* [host] ABI version (100 * major + minor) */

/* ------------------------------------------------------------------ element stiffness (L1)
 * fem_tet4_ke: c3d4 element matrices.
 *   kind = FEM_KIND_ELASTIC: Ke [M,12,12] = B^T D B V   — replaces compute_c3d4_K_matrix
 *          (`solver/element.py:883-903`, with B `:835-881`, D `:282-306`, V `:514-541`).
 *   kind = FEM_KIND_POISSON: Ke [M,4,4] = kappa V G G^T (derived P1 Laplacian; no reference function,
 *          SURVEY §8(a) a15); `E` is used as kappa.
 *   Singular check |det[1 x y z]| < 1e-12 -> FEM_ESINGULAR, *bad_idx [device int64] = first bad element
 *   (initialise it to M). */
int fem_tet4_ke(const double* coords, const int64_t* conn, int64_t M, double E, double nu, int kind,
                double* Ke, int64_t* bad_idx, fem_stream_t stream);

/* c3d4 geometry: vol [M] = |det|/6 (compute_tetrahedral_volumes, `solver/element.py:514-541`), grads [M,4,3]
 * (rows of inv([1 x y z]), `:851-866`), B [M,6,12] (compute_c3d4_B_matrix, `:835-881`); outputs may be NULL.
 * kind FEM_KIND_MASS of fem_tet4_ke gives the consistent P1 mass [M,12,12] = rho V (1+delta_ab)/20 (x) I3 with
 * E = rho (compute_c3d4_M_matrix, called at `solver_example.ipynb:221`; no source exists: parity unpinned). */
int fem_tet4_geom(const double* coords, const int64_t* conn, int64_t M, double* vol, double* grads, double* B,
                  int64_t* bad_idx, fem_stream_t stream);

/* fem_iso_ke: isoparametric solids c3d8 / c3d6 / c3d10 (npe = 8 / 6 / 10). The natural derivatives dN
 * [n_ip, npe, 3] and weights w [n_ip] are evaluated on the host exactly as the reference does (its quirks:
 * c3d10 weights summing to 0.45, the float32 line points of c3d6), then
 *   mode FEM_ISO_SUM    : Ke[M,d,d]      = sum_q w_q detJ_q B_q^T D B_q   (signed detJ)
 *   mode FEM_ISO_STACK  : Ke[n_ip,M,d,d] = detJ_q B_q^T D B_q            (`single=False`, Q6)
 *   mode FEM_ISO_VOLUME : Ke[M,d,d]      = B^T D B * wedge volume, one point (c3d6 single=True)
 * Replaces compute_c3d8_K_matrix (`solver/element.py:1754-1803`), compute_c3d6_K_matrix (`:2631-2676`),
 * compute_c3d10_K_matrix (`:1191-1239`). */
int fem_iso_ke(const double* coords, const int64_t* conn, int64_t M, int npe, double E, double nu,
               const double* dN, const double* w, int n_ip, int mode, double* Ke, fem_stream_t stream);
/* fem_iso_ke_sym: the same K_e (modes FEM_ISO_SUM / FEM_ISO_VOLUME) in the packed symmetric form of the internal
 * assembly path: per element only the upper 3x3 blocks (a <= b), row-major over the upper triangle (block (a, b) at
 * (a npe - a (a - 1) / 2 + b - a) * 9, entries r * 3 + c), fem_ke_sym_stride(npe) doubles per element (9 npe (npe + 1)
 * / 2 rounded up to even: c3d10 496 of 900, c3d8 324 of 576, c3d6 190 of 324). The upper blocks equal fem_iso_ke's
 * bit for bit. Consumed by fem_assemble_from_ke_sym; the reference-named functions keep the full [M, d, d]. */
int fem_ke_sym_stride(int npe);
int fem_iso_ke_sym(const double* coords, const int64_t* conn, int64_t M, int npe, double E, double nu,
                   const double* dN, const double* w, int n_ip, int mode, double* Kp, fem_stream_t stream);
/* fem_iso_mass: consistent mass of c3d8 / c3d6 / c3d10 (npe = 8 / 6 / 10) — no reference function exists (the
 * reference notebook calls a compute_c3d4_M_matrix defined nowhere, `solver_example.ipynb:221`): parity unpinned.
 *   Me[M, 3 npe, 3 npe], block (a,b) = rho sum_q w_q |detJ_q| N_a(q) N_b(q) I3
 * Nv [n_ip, npe] shape values and dN [n_ip, npe, 3] natural derivatives at the n_ip (<= 32) points, w [n_ip] weights
 * (element.py picks rules exact for N_a N_b on affine elements). */
int fem_iso_mass(const double* coords, const int64_t* conn, int64_t M, int npe, double rho, const double* Nv,
                 const double* dN, const double* w, int n_ip, double* Me, fem_stream_t stream);
/* the same consistent mass as its scalar factor: Ms [M, npe, npe] with M_e = Ms (x) I3 (block (a, b) = Ms[a][b] I3,
 * the values of fem_iso_mass's diagonal entries bit for bit) -- 1/9 of the bytes; assembled as a bs = 1 matrix on the
 * same node pattern it is the global M_s of M = M_s (x) I3 */
int fem_iso_mass_scalar(const double* coords, const int64_t* conn, int64_t M, int npe, double rho, const double* Nv,
                        const double* dN, const double* w, int n_ip, double* Ms, fem_stream_t stream);
/* J [M,3,3] (J[i][k] = sum_j dN[j][i] x_j[k]), global gradients [M,npe,3] and B [M,6,3npe] of an isoparametric
 * element at one point with natural derivatives dN [npe,3]; outputs may be NULL. Replaces compute_c3d8_Jacobian /
 * _shape_gradients / _B_matrix (`solver/element.py:1601-1694`) and the c3d6 (`:2482-2568`) / c3d10
 * (`:1026-1125`) equivalents. */
int fem_iso_geom(const double* coords, const int64_t* conn, int64_t M, int npe, const double* dN, double* J,
                 double* grads, double* B, fem_stream_t stream);

/* ------------------------------------------------------------------ mesh graph (pattern build)
 * Node -> (element, local) incidence, deterministic (entries sorted ascending by e*npe+local; a stable radix sort
 * of (node, slot) pairs). work: a device workspace of fem_incidence_work_bytes(M*npe, N)
 * bytes (256-aligned), or NULL to allocate it stream-ordered inside the call. */
int64_t fem_incidence_work_bytes(int64_t total, int64_t N);
int64_t fem_scan_work_len(int64_t n);
/* inc_ptr [N+1], inc [M*npe] */
int fem_incidence(const int64_t* conn, int64_t M, int npe, int64_t N, int32_t* inc_ptr, int32_t* inc,
                  int32_t* work, fem_stream_t stream);
/* the same with the connectivity check of the reference's indexing (IndexError in torch) folded in: *bad [device
 * int32] = 1 if any node id is outside [0, N) (such slots are left out), else 0 -- read it before using the result */
int fem_incidence_checked(const int64_t* conn, int64_t M, int npe, int64_t N, int32_t* inc_ptr, int32_t* inc,
                          int32_t* work, int32_t* bad, fem_stream_t stream);

/* Node-graph CSR pattern (block pattern for any dpn): the coalesced COO pattern of the reference's global
 * assembly (`subdivision.ipynb:118-139`) at node granularity. Two passes:
 *   fem_graph_count : row_len [N]  (unique neighbours incl. self; rows of any length, the widest by a selection
 *                     kernel); *overflow [device int, may be NULL] = 1 if some row has a neighbour more than 32767
 *                     rows away (16-bit column deltas do not fit), else 0
 *   fem_graph_fill  : colidx [nnz] sorted per row, diagpos [N] (position of the diagonal; -1 for a node no element touches)
 * rowptr [N+1] is the exclusive scan of row_len (fem_scan_i32). */
int fem_graph_count(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                    int32_t* row_len, int32_t* overflow, fem_stream_t stream);
int fem_graph_fill(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                   const int32_t* rowptr, int32_t* colidx, int32_t* diagpos, fem_stream_t stream);
/* Same pattern in (typically) one pass: rows of at most 32 neighbours from at most 384 candidates are gathered,
 * deduplicated and sorted once by a wave-private kernel into tmp [fem_graph_tmp_len(N)] (int32); the rest fall
 * back to the two-pass kernels above (LDS hash up to 512 neighbours, selection beyond). fem_graph_count2 writes row_len; fem_graph_fill2 copies / fills the rows. */
int64_t fem_graph_tmp_len(int64_t N);
int fem_graph_count2(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                     int32_t* row_len, int32_t* tmp, int32_t* overflow, fem_stream_t stream);
int fem_graph_fill2(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                    const int32_t* rowptr, const int32_t* tmp, int32_t* colidx, int32_t* diagpos,
                    fem_stream_t stream);
/* fem_graph_fill2 + fem_sell_fill + fem_sell_delta16 in one pass over the slices (slice_ptr from fem_sell_widths +
 * fem_scan_i64): colidx, diagpos, SELL cols, the 16-bit deltas dcols [slice_ptr[S]] (0 where they do not fit,
 * *overflow [device int] = 1 then: keep the int32 cols) and csr2sell (may be NULL: fem_sell_csr2sell forms it on
 * demand) -- the same arrays as the three calls. dcols / overflow may be NULL (fem_graph_count2's overflow already
 * told the caller whether the deltas fit). */
int fem_graph_sell_fill(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                        const int32_t* rowptr, const int32_t* tmp, const int64_t* slice_ptr, int32_t* colidx,
                        int32_t* diagpos, int32_t* cols, int16_t* dcols, int64_t* csr2sell, int32_t* overflow,
                        fem_stream_t stream);
/* fem_graph_sell_fill without csr2sell / overflow, plus the bs = 1 solver layout of fem_sell_sl_pattern (pcols, ucol,
 * uoff, and for G > 0 the persistent schedule's gather windows win[2 G]) formed in the same slice pass from the deltas
 * it writes -- the same arrays as fem_sell_sl_pattern, without its separate pass over the deltas. Needs the 16-bit
 * deltas (no neighbour more than 32767 rows away). */
int fem_graph_sell_fill_sl(const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                           const int32_t* rowptr, const int32_t* tmp, const int64_t* slice_ptr, int32_t* colidx,
                           int32_t* diagpos, int32_t* cols, int16_t* dcols, int G, int16_t* pcols, int16_t* ucol,
                           int32_t* uoff, int32_t* win, fem_stream_t stream);
/* exclusive scan of int32 counts -> out[n+1] (out[n] = total); work: int32 [fem_scan_work_len(n)] */
int fem_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* work, fem_stream_t stream);

/* CSR pattern -> SELL-64 pattern. slice_ptr [S+1] int64 (entries, i.e. 64*sum of widths); cols [slice_ptr[S]].
 *   fem_sell_widths: width [S] int64 = 64 * max row length in the slice (scan it with fem_scan_i64)
 *   fem_sell_fill  : cols (padding = own row) and the CSR->SELL entry map csr2sell [nnz] int64 */
int fem_sell_widths(const int32_t* rowptr, int64_t nrows, int64_t* width, fem_stream_t stream);
/* the pattern's sizes for the build's one device-to-host read, in one launch: out5 = {nnz = rowptr[N], SELL entries
 * = slice_ptr[S], *bad (fem_incidence_checked; 0 if NULL), *ovf (fem_graph_count2; 0 if NULL), widest slice =
 * max width[s]} (int64, device) */
int fem_graph_sizes(const int32_t* rowptr, const int64_t* slice_ptr, const int64_t* width, int64_t N,
                    const int32_t* bad, const int32_t* ovf, int64_t* out5, fem_stream_t stream);
/* the CSR -> SELL entry map (as fem_sell_fill writes it) from rowptr and slice_ptr alone */
int fem_sell_csr2sell(const int32_t* rowptr, int64_t nrows, const int64_t* slice_ptr, int64_t* csr2sell,
                      fem_stream_t stream);
int fem_scan_i64(const int64_t* in, int64_t n, int64_t* out, int64_t* work, fem_stream_t stream);
int fem_sell_fill(const int32_t* rowptr, const int32_t* colidx, int64_t nrows, const int64_t* slice_ptr,
                  int32_t* cols, int64_t* csr2sell, fem_stream_t stream);

/* Reverse Cuthill-McKee renumbering of the nodes (opt-in; no reference counterpart -- the reference keeps the file
 * order of `vtk_loader_to_torch`, `solver/element.py:39-90`, which this undoes for the assembled operator) over the
 * node-graph CSR pattern rowptr / colidx above: perm [N] (new -> old), inv [N] (old -> new). Deterministic: level-
 * synchronous Cuthill-McKee from the lowest-(degree, id) node, a level's nodes grouped by their parent's CM index,
 * a parent's children in ascending id; further components from their lowest-id node; nodes no element touches last;
 * the CM order reversed. work: int32 [fem_rcm_work_len(N)]; *levels_out (may be NULL): level steps
 * launched. One host round trip per 48 levels. */
int64_t fem_rcm_work_len(int64_t N);
int fem_rcm(const int32_t* rowptr, const int32_t* colidx, int64_t N, int32_t* perm, int32_t* inv, int32_t* work,
            int* levels_out, fem_stream_t stream);

/* ------------------------------------------------------------------ global assembly (values)
 * Deterministic row-gather: every block row sums its contributions in ascending element order.
 * fem_assemble_from_ke: values from element matrices Ke [M, npe*bs, npe*bs] (the solver-entry path: the
 *   reference hands K[M,d,d] to its CG, `solver/solver.py:144`).
 * fem_assemble_tet4  : values of the c3d4 elastic (bs=3) / Poisson (bs=1) operator computed on the fly
 *   from coordinates (K_e never materialised). E is kappa for Poisson.
 * Both write SELL values (vals must be zeroed by the caller). */
int fem_assemble_from_ke(const double* Ke, const int64_t* conn, int npe, int bs, const int32_t* inc_ptr,
                         const int32_t* inc, int64_t N, const int32_t* rowptr, const int32_t* colidx,
                         const int64_t* csr2sell, const int64_t* slice_ptr, double* vals, fem_stream_t stream);
/* fem_assemble_from_ke with the sizes the caller already knows (nnz = block-CSR entries, ent = SELL entries; -1:
 * read from the device) and store != 0 for a matrix whose values were never written: every SELL value is written
 * (padding zeroed), so the caller skips zeroing the matrix and the kernels skip reading it. Same values bit for bit
 * as zeroing + fem_assemble_from_ke (`solver/solver.py:144`'s K handoff, as above). */
int fem_assemble_from_ke_ex(const double* Ke, const int64_t* conn, int npe, int bs, const int32_t* inc_ptr,
                            const int32_t* inc, int64_t N, const int32_t* rowptr, const int32_t* colidx,
                            const int64_t* csr2sell, const int64_t* slice_ptr, int64_t nnz, int64_t ent, int store,
                            double* vals, fem_stream_t stream);
/* fem_assemble_from_ke_ex with the widest SELL slice in block columns (max_width > 0, from the pattern build): bs = 3
 * then runs the tile form -- the rows of a slice summed together in LDS and written straight into the SELL planes
 * (no block-CSR buffer, csr2sell unused and may be NULL). Same values bit for bit. max_width <= 0: as _ex. */
int fem_assemble_from_ke_ex2(const double* Ke, const int64_t* conn, int npe, int bs, const int32_t* inc_ptr,
                             const int32_t* inc, int64_t N, const int32_t* rowptr, const int32_t* colidx,
                             const int64_t* csr2sell, const int64_t* slice_ptr, int64_t nnz, int64_t ent, int store,
                             int max_width, double* vals, fem_stream_t stream);
int fem_assemble_tet4(const double* coords, const int64_t* conn, double E, double nu, int bs,
                      const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                      const int32_t* colidx, const int64_t* csr2sell, const int64_t* slice_ptr, double* vals,
                      int64_t* bad_idx, fem_stream_t stream);
/* fem_assemble_tet4 with store != 0 for a matrix whose values were never written: every SELL value is written
 * (padding zeroed) and nothing is read, so the caller skips zeroing it. Same values bit for bit as zeroing +
 * fem_assemble_tet4 (csr2sell is not read by the default accumulator kernel; pass it for FEM355_ASM_ROWS). */
int fem_assemble_tet4_ex(const double* coords, const int64_t* conn, double E, double nu, int bs,
                         const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                         const int32_t* colidx, const int64_t* csr2sell, const int64_t* slice_ptr, int store,
                         double* vals, int64_t* bad_idx, fem_stream_t stream);
/* fem_assemble_tet4_ex with the pattern's widest slice (max over slices of (slice_ptr[s+1] - slice_ptr[s]) / 64;
 * 0 = unknown): a P1 pattern of at most 16 columns per row takes the 16-column accumulator window (one sweep per
 * slice, less LDS per workgroup). Same values bit for bit whatever max_width says. */
int fem_assemble_tet4_ex2(const double* coords, const int64_t* conn, double E, double nu, int bs,
                          const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                          const int32_t* colidx, const int64_t* csr2sell, const int64_t* slice_ptr, int store,
                          int max_width, double* vals, int64_t* bad_idx, fem_stream_t stream);

/* SELL -> CSR values (export / testing): csr_vals [nnz*bs*bs] row-major blocks. */
int fem_sell_to_csr_vals(const double* vals, int bs, const int32_t* rowptr, int64_t nrows,
                         const int64_t* csr2sell, const int64_t* slice_ptr, double* csr_vals,
                         fem_stream_t stream);

/* Jacobi: w[i] = 1/A_ii (inf -> 0, `solver/solver.py:830-831`), w[i] = 0 where mask[i] != 0 (fixed DOFs);
 * mask may be NULL. diag read through diagpos (diagpos < 0: diagonal 0, so w = 0 as the reference's inf -> 0);
 * csr2sell may be NULL (the diagonal's SELL entry is then formed from rowptr and slice_ptr). */
int fem_jacobi(const double* vals, int bs, const int32_t* rowptr, const int32_t* diagpos,
               const int64_t* csr2sell, const int64_t* slice_ptr, int64_t nrows, const uint8_t* mask,
               double* w, fem_stream_t stream);

/* diag [nrows*bs] = the block diagonals' diagonal entries; w = 1/diag (inf -> 0, 0 where mask) — the two halves
 * of fem_jacobi, split so a distributed caller can halo-sum the diagonal in between (fem_halo_sum). */
int fem_sell_diag(const double* vals, int bs, const int32_t* diagpos, const int64_t* csr2sell, int64_t nrows,
                  double* diag, fem_stream_t stream);
int fem_jacobi_from_diag(const double* diag, int64_t n, const uint8_t* mask, double* w, fem_stream_t stream);

/* ------------------------------------------------------------------ element-by-element operator
 * y = sum_e P_e^T K_e P_e u — replaces compute_nodal_forces (`solver/element.py:429-464`), deterministic
 * (ascending element order per dof, like the CPU index_add). Ke [M, npe*dpn, npe*dpn]. */
int fem_ebe_apply(const double* Ke, const int64_t* conn, int npe, int dpn, const int32_t* inc_ptr,
                  const int32_t* inc, int64_t N, const double* u, double* y, fem_stream_t stream);
/* diag_K of compute_diagonal_preconditioner (`solver/solver.py:814-833`) before inversion:
 * colzero = 1 reproduces the reference's column-0 slice (`:828`, quirk Q1), 0 the true diagonal. */
int fem_ebe_diag(const double* Ke, const int64_t* conn, int npe, int dpn, const int32_t* inc_ptr,
                 const int32_t* inc, int64_t N, int colzero, double* diag, fem_stream_t stream);
/* out[i] = 1/in[i], inf -> 0 */
int fem_invert_diag(const double* in, int64_t n, double* out, fem_stream_t stream);

/* ------------------------------------------------------------------ stress recovery (post-solve)
 * strain = B u_e, stress = D strain (isotropic D of `solver/element.py:282-306`), tensor rows xx xy xz / xy yy yz /
 * xz yz zz, von Mises. u [N,3]. Outputs sig [.., 3, 3] and vm [..] may each be NULL. */
/* compute_c3d4_element_stress (`solver/element.py:905-937`): sig [M,3,3], vm [M]; bad_idx (nullable, preset to M)
 * receives the lowest element index with |det| < 1e-12 (the reference's B-matrix ValueError, `:857-858`). */
int fem_tet4_stress(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                    double* sig, double* vm, int64_t* bad_idx, fem_stream_t stream);
/* compute_c3d8/c3d6/c3d10_element_stress (`:1696-1752`, `:2570-2629`, `:1127-1189`) at n_ip points with natural
 * derivative tables dN [n_ip, npe, 3] (npe 6, 8, 10) and weights w [n_ip]. layout 0: sum_q w_q sig_q -> [M,3,3] and
 * sum_q w_q vm_q -> [M] (single=True); 1: [M,n_ip,3,3] / [M,n_ip] (c3d8/c3d6 single=False); 2: [n_ip,M,3,3] /
 * [n_ip,M] (c3d10 single=False). */
int fem_iso_stress(const double* coords, const int64_t* conn, int64_t M, int npe, const double* u, double E, double nu,
                   const double* dN, const double* w, int n_ip, int layout, double* sig, double* vm,
                   fem_stream_t stream);
/* compute_stress_tensor (`:308-330`): Voigt [M,6] (xx, yy, zz, xy, yz, xz) -> [M,3,3] */
int fem_voigt_to_tensor(const double* voigt, int64_t M, double* tensor, fem_stream_t stream);
/* compute_von_mises_stress (`:332-353`): [M,3,3] -> [M] */
int fem_von_mises(const double* tensor, int64_t M, double* vm, fem_stream_t stream);
/* compute_node_vm_stress (`:466-504`): out[n] = mean of ev[e] over the incidence of node n (0 if none), summed in
 * ascending element order (the reference's sequential index_add); inc from fem_incidence of the same [M,npe] */
int fem_node_average(const double* ev, int npe, const int32_t* inc_ptr, const int32_t* inc, int64_t N, double* out,
                     fem_stream_t stream);
/* compute_c3d4_surface_forces (`:3343-3362`): out [M,F,3] = sig_e n_ef for normals [M,F,3], sig [M,3,3] */
int fem_face_forces(const double* normals, const double* sig, int64_t M, int F, double* out, fem_stream_t stream);
/* compute_c3d4_shared_face_forces_sum (`:3364-3382`): out [S,3] = ff[e0,f0] + ff[e1,f1], idx [S,2,2] (validated by
 * the caller), ff [M,F,3] */
int fem_shared_face_sum(const int64_t* idx, const double* face_forces, int F, int64_t S, double* out,
                        fem_stream_t stream);

/* ------------------------------------------------------------------ mesh topology
 * Face / edge grouping: every element face of table ftab [F, fpn] (local node indices, element-major flat id
 * e * F + f) is keyed by its sorted node ids and radix-sorted once (stable), which reproduces torch.unique(dim=0)
 * row order and the reference's pairing order (`solver/element.py:543-579,707-762,1293-1334,1474-1532,2234-2283,
 * 2687-2713`). N bounds the node ids (< 2^32); F <= 12, fpn <= 4, M * F < 2^31. [sync] */
typedef struct fem_topo fem_topo;
int fem_topo_create(const int64_t* conn, int64_t M, int npe, const int32_t* ftab, int F, int fpn, int64_t N,
                    fem_stream_t stream, fem_topo** out);
/* number of distinct faces, of faces occurring once (surfaces) and of faces occurring exactly twice (shared) */
int fem_topo_counts(const fem_topo* t, int64_t* n_unique, int64_t* n_single, int64_t* n_pair);
/* shared faces [n_pair, 2, 2] = ((e0, f0), (e1, f1)) in key order, e0 * F + f0 < e1 * F + f1
 * (identify_*_shared_faces) */
int fem_topo_pairs(fem_topo* t, int64_t* out);
/* distinct sorted node tuples [n_unique, fpn] in lexicographic order (element_to_edge) */
int fem_topo_unique(fem_topo* t, int64_t* out);
/* faces occurring once, in face-major order fs * M + e of a caller table of Fs rows: stab [Fs, fpn] gives the
 * output node order, smap [Fs] the context row with the same node set, xtab [Fs] (nullable) the extra node
 * (compute_*_surface_faces_with_*_node). faces [count, fpn], extra [count] may be NULL to only count. [sync] */
int fem_topo_boundary(fem_topo* t, const int64_t* conn, int Fs, const int32_t* smap, const int32_t* stab,
                      const int32_t* xtab, int64_t* faces, int64_t* extra, int64_t* count);
void fem_topo_destroy(fem_topo* t);
/* out [M * T, spe] = conn[:, tab] (c3d8_to_c3d4 `:1555-1581`, c3d6_to_c3d4 `:2424-2446`, c3d10_to_c3d4 `:963-993`) */
int fem_sub_elements(const int64_t* conn, int64_t M, int npe, const int32_t* tab, int T, int spe, int64_t* out,
                     fem_stream_t stream);
/* per element face normals [M, F, 3]: (p[e1] - p[e0]) x (p[e2] - p[e0]) * scale for edges [F, 3]; unit: normalise;
 * flip: negate when dot(n, x[extra] - mean(x[cen[f][0..ncen[f])])) > 0 (cen is [F, 4]).
 * compute_tetrahedral_normals_and_area `:652-705`, compute_hexahedral_normals_and_area `:1418-1472`,
 * compute_wedge_normals_and_area `:2377-2422` */
int fem_element_face_normals(const double* coords, const int64_t* conn, int64_t M, int npe, const int32_t* edges,
                             const int32_t* cen, const int32_t* ncen, const int32_t* extra, int F, double scale,
                             int flip, int unit, double* out, fem_stream_t stream);
/* outward unit normals of surface faces [K, fpn] with extra nodes [K]; second edge to vertex v2
 * (compute_tetrahdral_surface_normals `:581-619`, compute_hexahedral_surface_normals `:1336-1374`,
 * compute_wedge_surface_normals `:2285-2338`) */
int fem_surface_normals(const double* coords, const int64_t* faces, const int64_t* extra, int64_t K, int fpn, int v2,
                        double* out, fem_stream_t stream);

/* ------------------------------------------------------------------ mesh input
 * Legacy VTK unstructured grid (ASCII / BINARY, file versions 2.x-5.x) -> points [N,3] fp64, the count-prefixed
 * cell array pyvista exposes as mesh.cells, and the VTK cell types: the file side of vtk_loader_to_torch
 * (`solver/element.py:39-90`). [host] — plain host memory, no device needed. */
typedef struct fem_vtk fem_vtk;
int fem_vtk_read(const char* path, fem_vtk** out);
int fem_vtk_sizes(const fem_vtk* v, int64_t* n_points, int64_t* n_cells, int64_t* cells_len, int64_t* n_types);
int fem_vtk_copy(const fem_vtk* v, double* points, int64_t* cells, int64_t* types);
void fem_vtk_free(fem_vtk* v);

/* ------------------------------------------------------------------ dof-level CSR layer (SURVEY §8(b) names)
 * The assembled-matrix view of the reference (`subdivision.ipynb:118-139`: rows dof_i, cols dof_j, K_e values
 * row-major, coalesced), dof = dpn * node + comp. [sync] where noted; temporaries are stream-ordered.
 * fem_solid_ke: c3d8 / c3d6 / c3d10 element matrices (type = nodes per element 8 / 6 / 10) from natural points
 *   ip [n_ip,3] and weights w [n_ip] (device); single = 1: sum_q w_q detJ_q B^T D B (c3d6: B at (1/3,1/3,0) times
 *   the wedge volume, ip ignored), single = 0: the per-point stack [n_ip,M,d,d] (c3d6: the weighted sum)
 *   (`solver/element.py:1754-1803`, `:2631-2676`, `:1191-1239`). */
int fem_solid_ke(int type, const double* coords, const int64_t* conn, int64_t M, double E, double nu, const double* ip,
                 const double* w, int n_ip, int single, double* Ke, fem_stream_t stream);
/* [sync] dof CSR pattern: rowptr [n_nodes*dpn+1], *nnz_out; with colidx (nnz, sorted per row) and diagpos
 * [n_nodes*dpn] (nullable) also the columns. Call once with colidx = NULL to size colidx. */
int fem_csr_pattern(const int64_t* conn, int64_t M, int npe, int dofs_per_node, int64_t n_nodes, int32_t* rowptr,
                    int32_t* colidx, int32_t* diagpos, int64_t* nnz_out, fem_stream_t stream);
/* vals += coalesce(P_e^T K_e P_e), Ke [M, npe*dpn, npe*dpn], summed per entry in ascending (element, local) order */
int fem_csr_fill(const double* Ke, const int64_t* conn, int64_t M, int npe, int dpn, int64_t n_nodes,
                 const int32_t* rowptr, const int32_t* colidx, double* vals, fem_stream_t stream);
/* y = A x on the dof CSR (n rows) */
int fem_spmv_csr(const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* x, double* y,
                 int64_t n, fem_stream_t stream);
/* [sync] one-shot solve on the dof CSR: mode FEM_MODE_CG_STABLE (`solver/solver.py:144-229`; fixed_mask dofs held
 * at zero) or FEM_MODE_PCG (`:766-812`; z = dinv r, fixed_mask dofs get dinv = 0). x: initial guess in, solution out;
 * res_hist_out [max_iter] (nullable) receives sqrt(r.z) per iteration. */
int fem_pcg_csr(const int32_t* rowptr, const int32_t* colidx, const double* vals, int64_t n, const double* b,
                double* x, const double* dinv, const uint8_t* fixed_mask, double tol, int max_iter, double eps,
                int mode, int* iters_out, int* status_out, double* res_hist_out, fem_stream_t stream);

/* ------------------------------------------------------------------ SpMV (L2)
 * y = A x on the SELL-64 matrix (nrows block rows of size bs). */
int fem_spmv(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols, const double* vals,
             const double* x, double* y, fem_stream_t stream);
/* 16-bit column deltas: dcols[e] = cols[e] - row (SELL layout); *overflow [device int32, zeroed] = 1 when a
 * delta exceeds +-32767 (then keep the int32 columns). Halves the index stream of every SpMV: 10 instead of
 * 12 bytes per scalar nonzero on banded (e.g. line-numbered or RCM-ordered) meshes. */
int fem_sell_delta16(const int32_t* cols, int64_t nrows, const int64_t* slice_ptr, int16_t* dcols, int32_t* overflow,
                     fem_stream_t stream);
int fem_spmv16(int64_t nrows, int bs, const int64_t* slice_ptr, const int16_t* dcols, const double* vals,
               const double* x, double* y, fem_stream_t stream);
/* measurement entry points (bench.py stream_ceiling): the HBM copy-ceiling probe dst = src and the read-only
 * probe (16-byte loads summed, *out written only to keep the loads alive) over n doubles (n even, 16-byte
 * aligned); grid <= 0: default. */
int fem_stream_copy(const double* src, double* dst, int64_t n, int grid, fem_stream_t stream);
int fem_stream_read(const double* src, double* out, int64_t n, int grid, fem_stream_t stream);

/* ------------------------------------------------------------------ (P)CG (L3)
 * One solve context over a SELL matrix. The whole iteration runs on the device: SpMV + p.q reduction,
 * update + r.z reduction, p/x update; scalars, guards and the stop test live in a device state word,
 * so the host only polls between chunks of iterations.
 *   mode FEM_MODE_CG_STABLE: stable_conjugate_gradient_solver (`solver/solver.py:144-229`), w = free mask
 *        (1 free / 0 fixed), alpha = rs/(pAp+eps), beta = rs_new/(rs_old+eps), stop sqrt(r.r) < tol
 *   mode FEM_MODE_PCG: preconditioned_conjugate_gradient_solver (`solver/solver.py:766-812`), w = M_inv,
 *        no eps, no guards, stop sqrt(r.z) < tol
 * b, x, w are [n = nrows*bs]; x holds u_init on entry and u on exit. hist [max_iter] (may be NULL)
 * receives sqrt(r.z) (sqrt(r.r) for CG) after each iteration. */
typedef struct fem_pcg fem_pcg;   /* opaque */
int fem_pcg_create(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols, const double* vals,
                   const double* b, double* x, const double* w, int mode, double tol, double eps,
                   double* hist, int64_t hist_len, fem_stream_t stream, fem_pcg** out);
/* initial residual r0 = b - A x0 (+ masking in CG mode), z0, p0, r0.z0 */
int fem_pcg_start(fem_pcg* s);
/* enqueue k iterations (no host sync); iterations after a stop are no-ops on the device */
int fem_pcg_iterate(fem_pcg* s, int k);
/* [sync] read iteration count, status and last r.z (or r.r). Guard stops (FEM_PCG_BREAKDOWN / _ALPHA_NAN) report
 * the reference's printed iteration; every other status the completed iterations. Returns FEM_ESTATE (status
 * FEM_PCG_BAD_WINDOW, message in fem_last_error) when a launch found a gather window outside its flag array */
int fem_pcg_poll(fem_pcg* s, int* iters, int* status, double* rz);
/* [debug, test-only] overwrite logical workgroup L's gather window with [lo, hi] in the active schedule's window
 * array (persistent or fused; call after fem_pcg_start): the fault-injection knob behind the FEM_PCG_BAD_WINDOW
 * test. FEM_EARG when the context has no window array */
int fem_pcg_debug_window(fem_pcg* s, int L, int lo, int hi);
/* [sync] diagnostic of a FEM_PCG_SYNC_TIMEOUT: the give-up site code (persistent kernel: 1 grid barrier, 2 u-flag
 * window, 3 rank sums of the DIST build, 5 granule reduction, + 16 * epoch; merged update k_pcg_update2: 4 + 16 * launch since start),
 * 0 for any other status */
int fem_pcg_sync_site(fem_pcg* s, int* site);
/* [sync] out6 = {rz (rs_old), pq (p.Ap), alpha, beta, rz_new, completed iterations} for the host messages */
int fem_pcg_scalars(fem_pcg* s, double* out6);
/* [sync] run to completion: start + chunks of `chunk` iterations until stop or max_iter (persistent schedule:
 * cooperative launches, deferred-schedule re-solve from x0 after a FEM_PCG_SYNC_TIMEOUT) */
int fem_pcg_solve(fem_pcg* s, int max_iter, int chunk, int* iters, int* status, double* rz);
/* kernel schedule: 0 = 3-kernel (SpMV+p.q / r update+r.z / x,p update; the context default), 1 = fused (p formed
 * inside the SpMV from r, w and the previous p; 2 kernels per iteration), 2 = deferred (each kernel finishes the
 * previous kernel's block partials itself: no grid atomics, state banked by launch parity), 3 = persistent
 * (pcg_persist.hpp: the single-reduction iteration as one cooperative launch per chunk, CG state of every row held in
 * registers / LDS of its owning wave, slices past 7 per wave streamed from HBM in the same launch; bs = 1 with
 * 16-bit columns and FEM_TUNE_PAIR, single GPU; otherwise fem_pcg_start falls back to 2; bs = 3: pcg_persist3.hpp,
 * 2 slices per wave on chip, past that the same overflow build), 4 = auto (3 where it applies -- for bs = 3 only
 * while the state fits on chip, else 0). Element-partitioned and constrained contexts accept only 0 (4 maps to 0). */
int fem_pcg_set_schedule(fem_pcg* s, int sched);
/* the SELL entry count of the context's matrix, which MUST equal slice_ptr[nslices] (known to the caller from the
 * pattern build; the paired copy is sized from it): spares fem_pcg_start the device-to-host read (a host sync)
 * before it builds that copy. Optional; without it fem_pcg_start reads the count itself. */
int fem_pcg_set_entries(fem_pcg* s, int64_t entries);
/* [host] the stop tolerance of fem_pcg_create, replaced: a host-side field that takes effect at the next fem_pcg_start
 * (so at the next fem_pcg_solve). The time integrator keeps one context for a whole run and sets each step's tolerance
 * from that step's right-hand side (the reference creates its solver state per call, `solver/solver.py:766-812`). */
int fem_pcg_set_tol(fem_pcg* s, double tol);
/* the schedule the context runs (valid after fem_pcg_start: 3 may have fallen back to 2) */
int fem_pcg_get_schedule(fem_pcg* s);
/* [sync] over the slices [s_begin, s_end) of the context's matrix (s_end < 0: to the last): the slices stored with
 * slice-uniform deltas (FEM_TUNE_PK_UNI; valid after fem_pcg_start), the slice count, and the column-index bytes one
 * SpMV over those slices reads (padding included) */
int fem_pcg_uniform_slices(fem_pcg* s, int64_t s_begin, int64_t s_end, int64_t* uniform, int64_t* nslices,
                           int64_t* index_bytes);
/* [sync] after fem_pcg_start: the slices whose diagonal the persistent launches keep on chip (FEM_TUNE_PK_OFFDIAG),
 * the slice count, and the value bytes one iteration therefore does not read (8 per row of such a slice); zeros for
 * a context that reads the full values. Overflow build: its overflow slices read the full rows and are not counted */
int fem_pcg_offdiag_slices(fem_pcg* s, int64_t* od_slices, int64_t* nslices, int64_t* bytes);
/* [sync, debug, test-only] the plain SELL values (slice_ptr[nslices] doubles, device) rebuilt from the started
 * context's diagonal-free stream and its dense diagonal; rowptr: the pattern's CSR row pointers (device, int32).
 * FEM_EARG when the context reads no such stream */
int fem_pcg_debug_offdiag(fem_pcg* s, const int32_t* rowptr, double* vals);
/* [sync] after fem_pcg_start: the slices the persistent launches read from descriptor records (FEM_TUNE_PK_DESC: every
 * slice-uniform slice of at most 16 streamed entries) and the slice count; 0 when the context's build reads none */
int fem_pcg_desc_slices(fem_pcg* s, int64_t* desc_slices, int64_t* nslices);
/* [sync, debug, test-only] the started context's descriptor records copied to the host: 16 words per slice -- value
 * base (words 0-1), streamed width (2), kd (bits 0-7, signed) | kind (bits 8-15: 0 diagonal-free, 1 full rows,
 * 2 read without a record) | an odd width's last delta (bits 16-31) (3), the streamed deltas two per word, zero-padded
 * (4-11); words 12-15 are unused. FEM_EARG when the context reads no records */
int fem_pcg_debug_desc(fem_pcg* s, uint32_t* records);
/* ------------------------------------------------------------------ solver layout
 * The matrix stored straight in the layout the PCG schedules read, so a solve converts nothing and the matrix is
 * resident once. bs = 1: lane-paired SELL entries (entry k of lane l of a slice of width w at 128 (k / 2) + 2 l + k % 2,
 * the odd tail at 128 (w / 2) + l), and in every slice whose rows take their columns at one sorted list of offsets
 * (slice-uniform) those offsets stored once, the rows' missing offsets holding value 0. bs = 3: the plane-paired
 * layout A (entry E = slice base + 64 k + lane: values (2t, 2t + 1) at 9 (E - lane) + 128 t + 2 lane, value 8 at
 * 9 (E - lane) + 512 + lane), columns the plain 16-bit deltas.
 *   fem_sell_sl_pattern : from the plain 16-bit deltas (fem_graph_sell_fill): pcols [entries] paired deltas, uoff
 *                         [nslices] (-1: per-lane deltas), ucol [2 (entries / 64) + 2] lists; with G > 0 also the
 *                         persistent schedule's gather windows win [2 G] for a G-workgroup grid (G = CUs rounded
 *                         down to a multiple of 8). bs = 3 reads only the windows
 *   fem_assemble_tet4_sl: the c3d4 values (bs = 1: Poisson, kappa = E; bs = 3: elasticity E, nu) into svals
 *                         [entries bs^2] in that layout (store != 0: every value written; else added) --
 *                         fem_assemble_tet4_ex2's sums, bit for bit, at other positions; uoff / ucol unused for bs = 3
 *   fem_assemble_from_ke_sl: bs = 3 stored element matrices (npe 4 / 6 / 8 / 10, the pattern's widest slice
 *                         max_width) into layout A -- fem_assemble_from_ke_ex2's sums, bit for bit
 *   fem_jacobi_sl       : fem_jacobi of such a matrix;  fem_spmv_sl: y = A x (bs = 3: pcols = the plain deltas);
 *   fem_sell_sl_unpair  : its plain SELL values
 *   fem_pcg_set_layout  : a context (16-bit columns set) reads the caller's svals (bs = 1 also pcols / uoff / ucol)
 *                         and windows (nullable) instead of building its own paired copy: no conversion at
 *                         fem_pcg_start; the arrays must outlive the context; vals of fem_pcg_create is then not read. */
int fem_sell_sl_pattern(int64_t nrows, const int64_t* slice_ptr, const int16_t* dcols, int G, int16_t* pcols,
                        int16_t* ucol, int32_t* uoff, int32_t* win, fem_stream_t stream);
int fem_assemble_tet4_sl(const double* coords, const int64_t* conn, double E, double nu, int bs,
                         const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                         const int32_t* colidx, const int64_t* slice_ptr, const int32_t* uoff, const int16_t* ucol,
                         int store, int max_width, double* svals, int64_t* bad_idx, fem_stream_t stream);
/* Per-element modulus scale: the arguments of fem_assemble_tet4_ex2 / fem_assemble_tet4_sl plus scale [M]
 * (device, fp64, required: NULL is FEM_EARG). Element e contributes scale[e] K_e(E, nu) (bs = 3) or
 * scale[e] K_e(kappa = E) (bs = 1): the factor multiplies the element volume when an item is staged and nothing else,
 * so scale = 1 gives the unscaled entry point's bits and a power-of-two scale that power of two times them. The same
 * kernel configurations, store handling, layouts and bad_idx as the unscaled calls; scale is only read and may not
 * alias vals / svals. csr2sell is unused (nullable): the row kernels (FEM355_ASM_ROWS) have no scaled form and that
 * variable is ignored here. */
int fem_assemble_tet4_scaled(const double* coords, const int64_t* conn, double E, double nu, int bs,
                             const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                             const int32_t* colidx, const int64_t* csr2sell, const int64_t* slice_ptr, int store,
                             int max_width, const double* scale, double* vals, int64_t* bad_idx,
                             fem_stream_t stream);
int fem_assemble_tet4_scaled_sl(const double* coords, const int64_t* conn, double E, double nu, int bs,
                                const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                                const int32_t* colidx, const int64_t* slice_ptr, const int32_t* uoff,
                                const int16_t* ucol, int store, int max_width, const double* scale, double* svals,
                                int64_t* bad_idx, fem_stream_t stream);
int fem_assemble_from_ke_sl(const double* Ke, const int64_t* conn, int npe, const int32_t* inc_ptr, const int32_t* inc,
                            int64_t N, const int32_t* rowptr, const int32_t* colidx, const int64_t* slice_ptr,
                            int store, int max_width, double* svals, fem_stream_t stream);
/* bs = 3 assembly from packed symmetric K_e (fem_iso_ke_sym; the tile form of fem_assemble_from_ke_ex2 / _sl): block
 * (a, b) read from the upper block, (b, a) from its transpose, in the same (incidence, b) order -- the same sums as
 * from the full K_e whose lower blocks mirror the upper ones. layout_a = 1: vals is the bs = 3 solver layout (as
 * fem_assemble_from_ke_sl), 0: the plain planes. Internal path of configs[4] (`solver/element.py:1191-1239,1754-1803`
 * K_e, `subdivision.ipynb:118-139` COO assembly semantics). */
int fem_assemble_from_ke_sym(const double* Kp, const int64_t* conn, int npe, const int32_t* inc_ptr,
                             const int32_t* inc, int64_t N, const int32_t* rowptr, const int32_t* colidx,
                             const int64_t* slice_ptr, int store, int max_width, int layout_a, double* vals,
                             fem_stream_t stream);
/* Stiffness and mass of one element family in one pass (configs[4]'s internal path): the bs = 3 K_e [M, 3 npe, 3 npe]
 * into layout A svals (fem_assemble_from_ke_sl's sums, bit for bit) and the scalar Me [M, npe, npe] (the consistent
 * mass factor M_s of M = M_s (x) I3) into the plain bs = 1 SELL values mvals of the same pattern
 * (fem_assemble_from_ke_ex2's bs = 1 sums, bit for bit); store != 0: both fresh (every value written), else both added.
 * One column search and one incidence walk for both matrices. Replaces the two assembly calls a caller of the
 * reference would make over `compute_K_matrix` (`solver/element.py:419-427`) and a mass matrix of the same mesh
 * (`solver_example.ipynb:216,221`), with the COO semantics of `subdivision.ipynb:118-139`. */
int fem_assemble_from_ke_mass_sl(const double* Ke, const double* Me, const int64_t* conn, int npe,
                                 const int32_t* inc_ptr, const int32_t* inc, int64_t N, const int32_t* rowptr,
                                 const int32_t* colidx, const int64_t* slice_ptr, int store, int max_width,
                                 double* svals, double* mvals, fem_stream_t stream);
int fem_jacobi_sl(const double* svals, int bs, const int32_t* rowptr, const int32_t* diagpos,
                  const int64_t* slice_ptr, const int32_t* uoff, const int16_t* ucol, int64_t nrows,
                  const uint8_t* mask, double* w, fem_stream_t stream);
int fem_spmv_sl(int64_t nrows, int bs, const int64_t* slice_ptr, const int16_t* pcols, const double* svals,
                const int32_t* uoff, const int16_t* ucol, const double* x, double* y, fem_stream_t stream);
int fem_sell_sl_unpair(int64_t nrows, int bs, const int64_t* slice_ptr, const int16_t* dcols, const int32_t* uoff,
                       const int16_t* ucol, const int32_t* rowptr, const double* svals, double* vals,
                       fem_stream_t stream);
int fem_pcg_set_layout(fem_pcg* s, const double* svals, const int16_t* pcols, const int32_t* uoff,
                       const int16_t* ucol, const int32_t* win, int G);
/* [host] the persistent build the context's launches run (valid after fem_pcg_start; all 0 when the schedule is not
 * 3): register slots per wave (bs = 1: 1, 2, 4 or 7; bs = 3: 2), 1 for the overflow build, and the packed
 * assignment's slices per wave (0: the even spread) */
int fem_pcg_persist_build(fem_pcg* s, int* slots, int* overflow, int* pack);
/* 1 in *on when the started context's persistent launches reduce d and g through tagged granules
 * (FEM_TUNE_PK_GRAN), 0 when they run the counter barrier or the schedule is not 3 */
int fem_pcg_persist_granules(fem_pcg* s, int* on);
/* 1 in *on when the started context runs the pipelined persistent iteration (FEM_TUNE_PK_GV), else 0 */
int fem_pcg_pipelined(fem_pcg* s, int* on);
/* persistent schedule only: k iterations of the instrumented kernel build; host_out[G * 8] = per-workgroup shader-clock
 * sums of the phases (u wait, SpMV, block sum, barrier + partial sums, step, update + drain + flag, launch prologue,
 * launch epilogue), then host_out[G * 8 + G * 16] = every wave's own SpMV clock sum; *grid = G */
int fem_pcg_persist_profile(fem_pcg* s, int k, unsigned long long* host_out, int* grid);
/* CG_CONSTRAINED projections applied to x once at fem_pcg_start (after r0 = b - A x0) and after every x update:
 *   order 0 (`enforce_constraints`, `solver/solver.py:478-510`): x[rbe2_slave] = x[rbe2_master] (all gathered
 *           before any is written), then x[spc_dof] = spc_val.  G must be 0.
 *   order 1 (`new_enforce_constraints`, `:665-700`): SPC, then RBE2, then for every RBE3 group g in order
 *           x[r3_master[g]] = sum_{e in [r3_ptr[g], r3_ptr[g+1])} r3_w[e] x[r3_slave[e]] / (r3_wsum[g] + 1e-30).
 * All indices are flat dofs (node * dpn + dof) in [0, n); r3_ptr is a CSR offset array with r3_ptr[0] = 0 (one
 * group per (RBE3, dof) pair: `:685-698`). The residual masking of SPC dofs and RBE2 slaves (`r[...] = 0`) is the
 * context's 0/1 weight vector w. All arrays are device-resident and must outlive the context.
 * [sync] validates every index once; FEM_EARG on a bad index, a non-constrained / distributed / graph context. */
int fem_pcg_set_constraints(fem_pcg* s, int order, int64_t R, const int64_t* rbe2_slave, const int64_t* rbe2_master,
                            int64_t S, const int64_t* spc_dof, const double* spc_val, int64_t G,
                            const int64_t* r3_ptr, const int64_t* r3_master, const double* r3_wsum,
                            const int64_t* r3_slave, const double* r3_w);
/* [sync] the same projections applied once to x [n] (stream-ordered), and r [n] (nullable) zeroed at the SPC dofs
 * and RBE2 slaves: `enforce_constraints` / `new_enforce_constraints` as standalone calls
 * (`solver/solver.py:478-510`, `:665-700`). */
int fem_enforce_constraints(double* x, double* r, int64_t n, int order, int64_t R, const int64_t* rbe2_slave,
                            const int64_t* rbe2_master, int64_t S, const int64_t* spc_dof, const double* spc_val,
                            int64_t G, const int64_t* r3_ptr, const int64_t* r3_master, const double* r3_wsum,
                            const int64_t* r3_slave, const double* r3_w, fem_stream_t stream);
/* tuning flags (default FEM_TUNE_REVERSE | FEM_TUNE_PAIR | FEM_TUNE_PK_SC1 | FEM_TUNE_PK_PACK | FEM_TUNE_PK_UNI |
 * FEM_TUNE_UPD1 | FEM_TUNE_PK_OFFDIAG | FEM_TUNE_PK_DESC | FEM_TUNE_PK_GRAN): the SpMV of every schedule sweeps each XCD's slice range backwards on
 * odd iterations, so the matrix tail read last (still in the MI355X's 256 MB memory-side cache) is read first by
 * the next sweep: 67 -> 57 us per SpMV on the 10M Poisson matrix. Results depend on the flags only through the
 * order of the per-block p.q partials (deterministic for a given flag set). */
enum { FEM_TUNE_REVERSE = 1, FEM_TUNE_PAIR = 2, FEM_TUNE_PK_SC1 = 4, FEM_TUNE_PK_PACK = 8, FEM_TUNE_C1F = 16,
       FEM_TUNE_PK_COOP = 32, FEM_TUNE_DIST_FINE = 64, FEM_TUNE_PK_UNI = 128, FEM_TUNE_PK_WIDE = 256,
       FEM_TUNE_DIST_DROP = 512, FEM_TUNE_UPD1 = 1024, FEM_TUNE_U2_HOLD = 2048, FEM_TUNE_U2_SMALL = 4096,
       FEM_TUNE_MF_GATHER = 8192, FEM_TUNE_PK_GV = 16384, FEM_TUNE_PK_OFFDIAG = 32768,
       FEM_TUNE_PK_DESC = 65536, FEM_TUNE_PK_GRAN = 131072, FEM_TUNE_PK_GRAN_SMALL = 262144 };
/* FEM_TUNE_PK_GRAN_SMALL (opt-in, with FEM_TUNE_PK_GRAN): the granule reduction also in the two- and four-slot builds
 * (2 to 4 packed slices per wave: about 0.2M to 1M rows on 256 workgroups). Measured there it is slower than the
 * counter barrier (two slots: 10.1 against 9.5 us per iteration) or no faster (four slots), so those builds keep the
 * barrier by default; same bits either way. */
/* FEM_TUNE_PK_GRAN (default): persistent schedule, bs = 1, single GPU, not the pipelined build, and only the builds
 * the default flag set reaches: those with FEM_TUNE_PK_DESC, FEM_TUNE_PK_OFFDIAG and FEM_TUNE_PK_SC1 all on (1 and 7
 * slots and the instrumented one; 2 and 4 slots with FEM_TUNE_PK_GRAN_SMALL) and the overflow build with
 * FEM_TUNE_PK_OFFDIAG and FEM_TUNE_PK_SC1. Any
 * other flag set keeps the counter barrier without notice: fem_pcg_persist_granules tells which reduction a context
 * runs. With it the per-iteration grid reduction of d = u.Au and g = r.z runs without a barrier: every workgroup
 * publishes its partials as 8-byte {epoch, half a double} granules (one relaxed agent-scope store each) in a parity
 * bank; wave 0 of every workgroup re-reads the d records it still misses, and the workgroup's last wave the g records
 * (published one SpMV phase earlier), until every tag equals the epoch, then sums them in the fixed order of the
 * counter barrier's sums: bit-identical iterates. Holding every d record of an epoch also tells a workgroup that all
 * others finished that SpMV, which is what lets it overwrite u. The group counters are never touched; a give-up
 * reports site 5. The flag may change between launches of a started context: a launch whose reduction differs from
 * the last one's starts the epochs over (sync words and granules zeroed). */
/* FEM_TUNE_PK_DESC (default; needs FEM_TUNE_PK_OFFDIAG and FEM_TUNE_PK_SC1, not the overflow build): the pass that
 * writes the diagonal-free stream also writes one 64-byte record per slice -- value base, streamed width, the
 * diagonal's list position and the slice's delta list -- and the kernel reads a slot's record with scalar loads, one
 * slot ahead (the sweep's first slot before the u-flag wait), instead of three dependent wave-uniform vector loads per
 * slot and the delta words of every round. A round's value loads and u gathers then leave together. The same products
 * in the same order: bit-identical iterates. Slices with per-lane deltas or more than 16 streamed entries are read as
 * before. fem_pcg_desc_slices reports how many slices run from records. */
/* FEM_TUNE_PK_OFFDIAG (default): persistent schedule, bs = 1, single GPU, not the pipelined build -- fem_pcg_start
 * writes a context-private copy of the paired values in which every slice-uniform slice whose delta list holds 0
 * leaves its diagonal out (width w - 1 at the slice's own slice_ptr base, sell_pair.hpp k_sell_offdiag), and the
 * dense diagonal beside it. The kernel keeps each row's diagonal in registers in place of the row's own u, which it
 * re-forms as the rounded product w r, and adds the diagonal term at its list position: 8 bytes and one gather per
 * row and iteration less, the same products in the same order, bit-identical iterates. The shared solver layout and
 * every other reader of it are untouched; slices with per-lane deltas keep their full rows, and so do the overflow
 * slices of the overflow build (their state is in memory: the term would cost two loads to save one).
 * fem_pcg_offdiag_slices reports what the started context left out. */
/* FEM_TUNE_PK_GV (opt-in, set before fem_pcg_start): persistent schedule, bs = 1, single GPU, PCG mode, systems of at
 * most 2 slices per wave (~2M rows on 256 CUs: the 1M-tet cube, a rank share of the 10M one) -- the pipelined
 * (Ghysels-Vanroose) Jacobi-PCG, whose grid reduction runs under the next SpMV (csrc/pcg_persist_gv.hpp). Its
 * iterates leave the single-reduction ones at rounding level (recurrences for M^-1 r and A M^-1 r); other contexts
 * ignore the flag. fem_pcg_pipelined reports whether the started context runs it. */
/* FEM_TUNE_MF_GATHER (A/B): on the element-chunk operator, q = A p is summed from the slots by a gather launch and
 * read by the merged update, instead of the update summing each dof's slots itself (the default; same bits). */
/* FEM_TUNE_U2_HOLD / FEM_TUNE_U2_SMALL (tests only): the merged update's give-up path -- workgroup 0 arrives only after
 * every other workgroup's bounded wait ran out, so the launch must end with FEM_PCG_SYNC_TIMEOUT, no x / p update
 * anywhere and the give-up site 4 (+ 16 * launch); and its grid capped at 8 workgroups, so a small system reaches the
 * loops past the register-cached elements. */
/* FEM_TUNE_UPD1 (default): single-GPU 3-kernel schedule (bs = 3 past the persistent kernel's capacity) -- the r / z
 * update and the x / p update run as ONE launch with every workgroup resident (k_pcg_update2: the last workgroup
 * finishes r.z and releases the others), z kept in registers in between: 8 vector streams per iteration instead of
 * 10. Same recurrences; p = z + beta p rounds z before the add (the two-kernel form may fuse it). */
/* FEM_TUNE_DIST_DROP: fault injection for the multi-GPU failure chain (tests only): the rank publishes no u row and
 * no flag to the other ranks, so their launches give up (FEM_PCG_SYNC_TIMEOUT) within the bounded waits */
/* FEM_TUNE_PK_WIDE: persistent schedule (bs = 1, single GPU) -- keep the 7-slot build when every wave owns at most
 * one slice (by default such systems, e.g. 1M tets, run a one-slot build with 8 lane pairs in flight; A/B switch) */
/* FEM_TUNE_PK_UNI (default): bs = 1 paired copies also record, per 64-row slice whose rows take their columns at one
 * common sorted list of offsets (rows lacking an offset get a zero value there), that list once (sell_pair.hpp
 * k_sell_uniform); the persistent schedule then reads those slices' deltas with wave-uniform loads: 10 -> 8 bytes
 * per matrix entry (every slice of the Kuhn cubes). Same products in the same order per row (+-0 terms between). */
/* FEM_TUNE_DIST_FINE (set before fem_pcg_set_rows): the distributed persistent comm block (u, flags, rank sums) in
 * fine-grained device memory (hipDeviceMallocFinegrained) instead of hipMalloc's coarse-grained memory -- the
 * variant bench.py tries when the coarse-grained one fails its self-check on a multi-GPU node. */
/* FEM_TUNE_PK_COOP: persistent schedule — every launch is a hipLaunchCooperativeKernel (the runtime guarantees that
 * all workgroups are resident at once, or fails the launch). fem_pcg_solve always launches cooperatively and, should
 * a launch still end with FEM_PCG_SYNC_TIMEOUT, re-solves from the saved x0 on the deferred schedule; without the
 * flag fem_pcg_iterate / fem_pcg_profile use plain launches (residency from the occupancy check) and report the
 * timeout status. */
/* FEM_TUNE_C1F: distributed single-reduction contexts run each iteration as ONE launch (k_cg1_fused: step, update,
 * u hand-off to the neighbouring workgroups by flags, SpMV, pack, one two-value grid reduction) instead of
 * k_cg1_update + k_cg1_spmv. */
/* FEM_TUNE_PK_PACK (default): persistent schedule only — each workgroup gives its waves ceil(max slices per
 * workgroup / 16) slices each in order (the last busy wave takes the remainder) instead of spreading them evenly:
 * at 10M 15 waves x 7 slices all stream to the end of the SpMV phase instead of 7-slice waves finishing alone
 * (54.0 -> 51.6 us per iteration; 3M tets 21.6 -> 19.3; equal at 1M and 6M). Same per-row arithmetic, so the
 * iterates change only through the order of the u.v partials. */
/* FEM_TUNE_PK_SC1 (default): persistent schedule only — the u gathers are sc1 (agent-coherent) loads instead of
 * plain loads behind an agent acquire per workgroup and iteration (whose L2 invalidations cost the other workgroups
 * of the XCD their gather window): 58.8 -> 55.9 us per 10M Poisson iteration, bit-identical iterates. */
/* FEM_TUNE_PAIR (default): contexts with 16-bit columns keep a copy of the matrix read with 16-byte value loads,
 * rebuilt from vals / cols16 by every fem_pcg_start: bs = 1 lane-paired (two entries per load, sell_pair.hpp; +257 MB
 * on the 10M Poisson matrix), bs = 3 plane-paired (values 0..7 of a block as four 16-byte loads, sell_pair3.hpp
 * layout A; +1.85 GB on the 10M elasticity matrix). Same products, same summation order per row as the plain layout. */
int fem_pcg_set_tuning(fem_pcg* s, int flags);
/* run the SpMV of this context on 16-bit column deltas (NULL: back to the int32 columns) */
int fem_pcg_set_cols16(fem_pcg* s, const int16_t* dcols);
/* apply the deferred x update of the fused schedule after the last iteration (fem_pcg_solve does this) */
int fem_pcg_finish(fem_pcg* s);
/* capture `k` iterations in a hipGraph and use it for fem_pcg_iterate calls with that k (0 disables) */
int fem_pcg_use_graph(fem_pcg* s, int k);
/* [sync] enqueue k iterations like fem_pcg_iterate, bracketing every `every`-th iteration's three kernels
 * with hip events on the solver stream; ms[0..2] = summed device ms of SpMV+dot / update / p-x update over the
 * n[0..2] sampled launches (bench.py's live per-kernel timing inside its timed region) */
int fem_pcg_profile(fem_pcg* s, int k, int every, double* ms, int* n);
void fem_pcg_destroy(fem_pcg* s);
/* ------------------------------------------------------------------ multi-GPU persistent schedule (rows partitioned)
 * The persistent schedule across ranks (one process per GPU, or several contexts of one process on one GPU for
 * validation): every rank holds the SELL rows of the global matrix it owns (global row / column numbering, all
 * vectors global-length) and runs ONE persistent launch per chunk over its own slices; the u rows another rank
 * gathers are written straight into that rank's comm block (system-scope stores over xGMI + a system release +
 * an epoch flag per workgroup), and the per-iteration sums go rank -> every rank the same way, summed in rank
 * order (bit-identical scalars everywhere). No collective library call inside an iteration. bs = 1 only.
 *   fem_pcg_set_rows  : rank `rank` of `nranks` (<= 8) owns the global slices [split[rank], split[rank+1]) of the
 *                       context's matrix; grid = workgroups of this rank's launches (0: one per CU; a multiple of
 *                       8: several ranks sharing one GPU); allocates the comm block and the gather windows.
 *   fem_pcg_comm_block: [host] the rank's comm block (device memory from hipMalloc: exportable with fem_ipc_handle)
 *   fem_pcg_col_window: [sync] min / max global column of the own rows (exchange between the ranks)
 *   fem_pcg_set_peers : every rank's comm block as mapped in THIS process (own entry ignored) and column window
 *   then fem_pcg_start on EVERY rank, a host barrier over the ranks, and fem_pcg_iterate / fem_pcg_profile /
 *   fem_pcg_poll with the same k on every rank (the first launch after a start forms r0 = b - A x0, u0 and r0.u0
 *   itself). fem_pcg_solve refuses such a context (it cannot place the barrier).
 * fem_ipc_handle / fem_ipc_open / fem_ipc_close: 64-byte hipIpcMemHandle of a device allocation, and its mapping in
 * another process (hipIpcMemLazyEnablePeerAccess). */
int fem_pcg_set_rows(fem_pcg* s, int nranks, int rank, const int64_t* slice_split, int grid);
int fem_pcg_comm_block(fem_pcg* s, void** base, int64_t* bytes);
int fem_pcg_col_window(fem_pcg* s, int64_t* lo, int64_t* hi);
int fem_pcg_set_peers(fem_pcg* s, void* const* bases, const int64_t* need_lo, const int64_t* need_hi);
/* [sync] diagnostics of a distributed persistent context into host_out[n]: which 0 = gather windows [G] first /
 * [G] last global workgroup + the column window, 1 = u-flag of every global workgroup in this rank's comm block,
 * 2 = publication table [G][nranks][2], 3 = rank epoch lines, 4 = local sync words (18 lines' first words) */
int fem_pcg_dist_debug(fem_pcg* s, int which, int32_t* host_out, int64_t n);
/* [host] a stream whose kernels run only on the CUs with cu % nparts == part (hipExtStreamCreateWithCUMask: its own
 * hardware queue) -- several emulated ranks of one process then run their persistent launches side by side */
int fem_stream_create_cu(int part, int nparts, void** stream);
int fem_stream_destroy(void* stream);
/* distributed persistent contexts: every later launch runs the phase-clock build (pcg_persist.hpp PROF) into dev_buf
 * ([G][8] phase sums, then [G][16] per-wave SpMV sums, as fem_pcg_persist_profile); NULL turns it off */
int fem_pcg_set_prof(fem_pcg* s, unsigned long long* dev_buf);
int fem_ipc_handle(void* ptr, char* out64);
int fem_ipc_open(const char* h64, void** ptr);
int fem_ipc_close(void* ptr);
/* [host] free the buffers that destroyed bs = 1 contexts left in the library's recycling cache (capped at
 * FEM355_PCG_CACHE_MB, default 1024 MB; invisible to torch's allocator); returns the MB released */
int fem_pcg_release_cache(void);
/* [host, sync] free the per-stream scratch buffers the library keeps between calls and trim its private stream-
 * ordered pools (capped at 256 MB of retained memory each) to zero; called by the Python layer at exit */
int fem_release_scratch(void);

/* ------------------------------------------------------------------ multi-GPU (element partition, RCCL)
 * One process per GPU. Every rank holds the SELL matrix of ITS elements over its local nodes (unassembled at
 * nodes shared with other ranks) and the global interface list: imap [nI] = local row of global interface node j
 * (-1 if the rank has no copy), ipos [nrows] = interface index of a local row (-1 interior), own [nrows] = 1 on
 * the rows the rank owns (owner = lowest rank touching the node). Each iteration then adds, on the device
 * stream: ONE all-reduce of the compact interface vector of A p (nI*bs doubles) with this rank's p.q partial
 * appended (p . q_rank over all local rows sums to p.q exactly), and one scalar all-reduce of r.z over owned
 * rows. The reference has no multi-device code; this replaces its
 * single-GPU region-growing split (`subdivision.ipynb:194-297`) with a deterministic partition.
 *   fem_comm_unique_id: [host] 128-byte RCCL id from rank 0 (broadcast it with any host transport)
 *   fem_comm_init     : [sync] communicator of this rank on the current HIP device */
int fem_comm_unique_id(char* out128);
int fem_comm_init(int nranks, int rank, const char* id128, void** comm);
int fem_comm_destroy(void* comm);
int fem_allreduce_sum(void* comm, double* buf, int64_t n, fem_stream_t stream);
/* v[interface rows] <- sum over ranks (buf: [nI*bs] scratch) = pack, all-reduce, unpack */
int fem_halo_pack(const double* v, int bs, const int32_t* imap, int64_t nI, double* buf, fem_stream_t stream);
int fem_halo_unpack(double* v, int bs, const int32_t* ipos, int64_t nrows, const double* buf, fem_stream_t stream);
int fem_halo_sum(void* comm, double* v, int bs, const int32_t* imap, int64_t nI, const int32_t* ipos, int64_t nrows,
                 double* buf, fem_stream_t stream);
/* switch a (P)CG context to the distributed iteration (enable=1; 3-kernel schedule, no graph). With comm = NULL
 * the exchanges are left to the caller, who drives the iteration phase by phase (below). */
int fem_pcg_set_dist(fem_pcg* s, int enable, void* comm, int64_t nI, const int32_t* imap, const int32_t* ipos,
                     const uint8_t* own);
/* Distributed iteration variant (call after fem_pcg_set_dist; resets on every fem_pcg_set_dist):
 *   0: the two-reduction PCG above (halo + p.q all-reduce, then the r.z all-reduce; six kernels per iteration)
 *   1: single reduction (Chronopoulos-Gear form of the same PCG): v = A u with u = z carried alongside r, so r.z,
 *      u.v and the interface rows of v ride in ONE all-reduce per iteration (three kernels). Same stop test and
 *      guards; rounding differs from variant 0 (N>1 contract: u within 1e-10, iterations within +-2).
 *      Phases: start 10 | sum | 20 | sum; iteration 4 | sum (buffer: fem_pcg_dist_buffer of that phase). */
int fem_pcg_set_dist_variant(fem_pcg* s, int variant);
/* neighbour exchange for the single-reduction variant (call after fem_pcg_set_dist_variant(s, 1)): the per-iteration
 * all-reduce of [interface rows | g | d] becomes ONE grouped ncclSend/ncclRecv with each of the npeer other ranks
 * (every other rank: the [g, d] pair travels to all). Message i (to and from peer_rank[i], peer_cnt[i] doubles) =
 * [g, d | bs values of each node shared with that rank, ascending global interface index]; the slot layout is the
 * same in both directions. csrc[J * nranks + r] (device int32, J over the nI global interface nodes) = offset of node
 * J's component 0 in the slot of rank r (-1: this rank, -2: r does not touch J or this rank does not); ssrc[r]
 * (device int32) = offset of rank r's [g, d] pair (-1: this rank). The SpMV kernel writes straight into the send
 * slots, the step/update kernels sum the received slots in rank order 0..nranks-1, so shared dofs stay
 * bit-identical across ranks. The maps stay owned by the caller (fem355.dist.p2p_maps builds them). */
int fem_pcg_set_p2p(fem_pcg* s, int nranks, int npeer, const int* peer_rank, const int64_t* peer_cnt,
                    const int32_t* csrc, const int32_t* ssrc);
/* the neighbour-exchange staging buffers (psend / precv, total doubles) */
int fem_pcg_p2p_buffers(fem_pcg* s, double** psend, double** precv, int64_t* total);
/* group path (all P ranks' contexts in one process, ctx[r] = rank r): every rank's message to each peer copied into
 * that peer's receive slot (what the grouped ncclSend/ncclRecv moves) */
int fem_p2p_deliver(fem_pcg* const* ctx, int P, fem_stream_t stream);
/* Phase-driven distributed iteration (what fem_pcg_start/iterate do around ncclAllReduce): phases 10, 11, 12
 * start the solve, phases 0..3 are one iteration; after a phase whose fem_pcg_dist_buffer is non-empty (10, 11:
 * start; 0: interface rows of A p + the p.q partial; 2: the r.z partial) that buffer must be summed over all ranks. Used to validate the distributed kernels with several
 * partitions in ONE process on one GPU (RCCL refuses two ranks on one device). */
int fem_pcg_dist_phase(fem_pcg* s, int phase);
int fem_pcg_dist_buffer(fem_pcg* s, int phase, double** ptr, int64_t* n);
/* dev_ptr_array: DEVICE array of P device pointers; sums the P buffers (rank order) into each of them */
int fem_group_allreduce(double* const* dev_ptr_array, int P, int64_t n, fem_stream_t stream);

/* ------------------------------------------------------------------ element-chunk operator (matrix-free c3d4)
 * y = K x of the c3d4 stiffness (kind FEM_KIND_ELASTIC, bs = 3: K_e of compute_c3d4_K_matrix, `solver/element.py:
 * 883-903`) or the P1 Laplacian (FEM_KIND_POISSON, bs = 1, kappa = E) formed element by element from the vertex
 * coordinates in every application -- the reference's element-by-element product `compute_nodal_forces`
 * (`solver/element.py:429-464`) without K_e in memory. Elements in Morton order, cut into chunks of <= 512 elements /
 * <= 256 nodes; per chunk a fixed-order sum per local node into a slot, per node a fixed-order sum of its slots
 * (deterministic). coords [N,3] and conn [M,4] (int64) must stay alive and unchanged while the operator is used.
 * FEM_ESINGULAR (*bad_idx = smallest element with |det| < 1e-12, `solver/element.py:857-858`), FEM_EARG for a node
 * outside [0, N). */
typedef struct fem_mf fem_mf;
int fem_mf_create(const double* coords, const int64_t* conn, int64_t M, int64_t N, int kind, double E, double nu,
                  int64_t* bad_idx, fem_stream_t stream, fem_mf** out);
int fem_mf_destroy(fem_mf* m);
/* y = K x ([N*bs] each; y overwritten) */
int fem_mf_apply(fem_mf* m, const double* x, double* y, fem_stream_t stream);
/* d = diag(K) [N*bs] (the exact diagonal) */
int fem_mf_diag(fem_mf* m, double* d, fem_stream_t stream);
/* out6 = {chunks, slots, bs, static bytes streamed per application, M, N} */
int fem_mf_info(fem_mf* m, int64_t* out6);
/* device copies of the layout (each nullable): Morton element order [M], chunk element offsets and slot offsets
 * [chunks + 1], slot nodes [slots] */
int fem_mf_order(fem_mf* m, int32_t* eorder, int32_t* cptr, int32_t* sbase, int32_t* cnode, fem_stream_t stream);
/* the context's operator becomes m (nrows = N, bs = m's; create the context with NULL slice_ptr / cols / vals):
 * K1 = the chunk kernel with the p.q reduction + the slot gather, then the merged update; modes PCG and CG_STABLE
 * (FEM_EARG for CG_CONSTRAINED, and fem_pcg_set_constraints refuses an operator context), schedule 0. The context
 * allocates its own slot buffer, so contexts (and fem_mf_apply / fem_mf_diag, which use the operator's) may run on
 * different streams at once. Distributed contexts (fem_pcg_set_dist, element partitions: m = the rank's own
 * elements over its local nodes) run the single-reduction iteration (variant 1, all-reduce or neighbour exchange,
 * not fused): per iteration k_cg1_update, the rank's chunks into the slots, and the slot gather that packs the
 * interface rows and the [g, d] pair -- BASELINE configs[3] with no assembled matrix (`solver/element.py:429-464`
 * per partition, `subdivision.ipynb:248-279`). */
int fem_pcg_set_operator_mf(fem_pcg* s, fem_mf* m);

/* ------------------------------------------------------------------ multi-load-case (P)CG (csrc/pcg_multi.hip)
 * Several right-hand sides of one matrix solved in lock-step: the matrix is streamed once per iteration for all of
 * them. Multi-vectors are [n, nv] row-major (n = nrows * bs; the nv columns of one dof adjacent, 16-byte aligned);
 * nv is 2, 4 or 8 (the caller pads with zero columns), bs 1 or 3; anything else is FEM_EARG. The matrix is the plain
 * SELL-64 layout at the top of this file, columns as 16-bit deltas dcols (column = row + delta) when not NULL, else
 * the int32 cols.
 * fem_spmm: Y = A X (the reference applies K to several vectors by looping `compute_nodal_forces` over them,
 *   `solver/solver.py:1151-1168`), per row and column the summation order of fem_spmv. */
int fem_spmm(int64_t nrows, int bs, int nv, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
             const double* vals, const double* X, double* Y, fem_stream_t stream);
/* One context for nv columns of which the first nactive are solved; the rest are padding, frozen from the start,
 * never updated and never reported (their B and X columns must be zero). B, X [n, nv]; w [n] is shared by all columns
 * (one matrix, one fixed set); tol [host, nv] is per column; hist [hist_len, nv] (may be NULL) receives sqrt(r.z)
 * (sqrt(r.r) for CG) per iteration and column. Modes FEM_MODE_CG_STABLE and FEM_MODE_PCG, column by column with
 * exactly the semantics documented at fem_pcg_create (mask and eps, the three CG guards reporting the reference's
 * printed iteration, no guards in PCG mode, stop on sqrt(r.r) resp. sqrt(r.z) < tol[j]); FEM_MODE_CG_CONSTRAINED is
 * FEM_EARG. Every column has its own alpha, beta, iteration count and status on the device; a column that has
 * stopped is frozen (x, r, p skipped by predicate), so a breakdown or NaN in one column never reaches another, and
 * a column's bits do not depend on what the other columns hold. Plain launches only; reductions are finished by a
 * later launch in a fixed order (bit-reproducible). */
typedef struct fem_mpcg fem_mpcg;
int fem_mpcg_create(int64_t nrows, int bs, int nv, int nactive, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* vals, const double* B, double* X, const double* w, int mode,
                    const double* tol, double eps, double* hist, int64_t hist_len, fem_stream_t stream,
                    fem_mpcg** out);
/* [sync] run from the X in place until every active column has stopped or max_iter (columns still running then:
 * FEM_PCG_MAXITER); the host enqueues `chunk` iterations at a time and reads the state in between. iters, status,
 * rz: [host, nactive], as fem_pcg_poll reports them per column */
int fem_mpcg_solve(fem_mpcg* s, int max_iter, int chunk, int* iters, int* status, double* rz);
/* [sync] out [host, nactive * 6]: fem_pcg_scalars' six values per column */
int fem_mpcg_scalars(fem_mpcg* s, double* out);
void fem_mpcg_destroy(fem_mpcg* s);

/* ------------------------------------------------------------------ two-level PCG (csrc/pcg_coarse.hip)
 * The Jacobi preconditioner plus an additive coarse correction over aggregates of nodes, each carrying its six
 * rigid-body modes: M^-1 = diag(w) + Z (Z^T A Z)^-1 Z^T. bs must be 3 with three translational dofs per node
 * (anything else, a 6-dof shell system included, is FEM_EARG), k is 1 to FEM_COARSE_MAX_AGG aggregates, m = 6 k. Z is
 * never stored: the row block of node i is R_i = [I_3 | -[rel_i]x] with rel [nrows, 3] the node's position relative to
 * the centre of its aggregate agg [nrows] (int32, -1: in no aggregate); the rows of the dofs with w == 0 are zero.
 * agg_ptr [k + 1] / agg_nodes list every aggregate's nodes, ascending inside an aggregate. The matrix arguments are
 * those of fem_mpcg_create. Plain launches, no floating-point atomics, every sum in an order fixed by the sizes alone
 * (the same bits on every run), rows >= nrows never read or stored.
 * fem_coarse_restrict: c [m] = Z^T r, one workgroup per aggregate, the node list in order.
 * fem_coarse_apply: z = w o r + Z (Einv c) for the dense symmetric Einv [m, m]; y [m] receives Einv c.
 * fem_coarse_galerkin_count / fem_coarse_galerkin / fem_coarse_galerkin_sum: E = Z^T A Z as records. count [nrows]
 *   (int64) = the distinct aggregates among a row's neighbours (0 for a row in none); offset [nrows + 1] its exclusive
 *   scan (fem_scan_i64); every row then writes one record per neighbour aggregate b in ascending id: keys [.] =
 *   agg[row] k + b and rec [., 36] = R_i^T sum_{j in b} A_ij R_j. The caller sorts the keys (stable) into `order`;
 *   the sum adds the records of each of the nkeys distinct keys ukeys (records order[key_ptr[u] .. key_ptr[u + 1]))
 *   in that order into the zero-initialised E [m, m]. */
#define FEM_COARSE_MAX_AGG 512
int fem_coarse_restrict(int64_t nrows, int bs, int k, const int32_t* agg_ptr, const int32_t* agg_nodes,
                        const double* rel, const double* w, const double* r, double* c, fem_stream_t stream);
int fem_coarse_apply(int64_t nrows, int bs, int k, const int32_t* agg, const double* rel, const double* w,
                     const double* Einv, const double* c, const double* r, double* y, double* z, fem_stream_t stream);
int fem_coarse_galerkin_count(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols,
                              const int16_t* dcols, const int32_t* agg, int64_t* count, fem_stream_t stream);
int fem_coarse_galerkin(int64_t nrows, int bs, int k, const int64_t* slice_ptr, const int32_t* cols,
                        const int16_t* dcols, const double* vals, const int32_t* agg, const double* rel,
                        const double* w, const int64_t* offset, int64_t* keys, double* rec, fem_stream_t stream);
int fem_coarse_galerkin_sum(int64_t nkeys, int k, const int64_t* ukeys, const int64_t* key_ptr, const int64_t* order,
                            const double* rec, double* E, fem_stream_t stream);
/* The lock-step context in the shape of fem_mpcg_* at one column, FEM_MODE_PCG's semantics with the two-level z: stop
 * on sqrt(r.z) < tol, hist [hist_len] (may be NULL) receives sqrt(r.z) per iteration. One guard more than
 * FEM_MODE_PCG, because Einv is only numerically positive definite: p.q <= 0 or non-finite stops with
 * FEM_PCG_BREAKDOWN at that iteration. x holds the start vector on entry and the solution on exit. */
typedef struct fem_pcg2 fem_pcg2;
int fem_pcg2_create(int64_t nrows, int bs, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
                    const double* vals, const double* b, double* x, const double* w, int k, const int32_t* agg,
                    const int32_t* agg_ptr, const int32_t* agg_nodes, const double* rel, const double* Einv, double tol,
                    double* hist, int64_t hist_len, fem_stream_t stream, fem_pcg2** out);
/* [sync] run from the x in place; the host enqueues `chunk` iterations at a time and reads the state in between;
 * iterations after a stop are no-ops on the device */
int fem_pcg2_solve(fem_pcg2* s, int max_iter, int chunk, int* iters, int* status, double* rz);
/* [sync] fem_pcg_scalars' six values */
int fem_pcg2_scalars(fem_pcg2* s, double* out6);
void fem_pcg2_destroy(fem_pcg2* s);

/* ------------------------------------------------------------------ mid-edge nodes of c3d4 meshes (csrc/refine.hip)
 * The device side of c3d4_to_c3d10 and refine_c3d4. uedges [E, 2] are the mesh's distinct edges (a < b, lexicographic:
 * fem_topo_unique on the six-edge table). Element e meets its edges in the walk (0,1), (1,2), (2,0), (0,3), (1,3),
 * (2,3): slot 6 e + k.
 * fem_refine_edge_slots: eid [6 M] int32 = the slot's edge (-1: not in the list), minslot [E] (preset to INT64_MAX by
 *   the caller) = the lowest slot naming the edge (integer minimum: independent of the order of arrival).
 * fem_refine_emit: out [M, 10] = the four corners, then N + mid_id[eid[slot]] in walk order (c3d10 node order).
 * fem_refine_nodes: coords_out [N + E, 3] and parents [N + E, 2] int32: node i < N is itself (parents i, i), node
 *   N + mid_id[j] is 0.5 (x[a] + x[b]) of edge j = (a, b), one rounding (parents a, b). N + E must fit int32. */
int fem_refine_edge_slots(const int64_t* conn, int64_t M, const int64_t* uedges, int64_t E, int32_t* eid,
                          int64_t* minslot, fem_stream_t stream);
int fem_refine_emit(const int64_t* conn, int64_t M, int64_t N, const int32_t* eid, const int64_t* mid_id, int64_t* out,
                    fem_stream_t stream);
int fem_refine_nodes(const double* coords, int64_t N, const int64_t* uedges, int64_t E, const int64_t* mid_id,
                     double* coords_out, int32_t* parents, fem_stream_t stream);

/* ------------------------------------------------------------------ geometric multigrid PCG (csrc/multigrid.hip)
 * PCG with z = one V(degree, degree) cycle over nlev >= 2 nested levels, level 0 the coarsest, level nlev - 1 the
 * matrix being solved. Every per-level argument is a host array of nlev device pointers: the level's plain SELL-64
 * matrix (slice_ptr, cols or 16-bit dcols, vals; bs = 1 or 3 on all levels; unused on level 0), its masked Jacobi
 * weights w (zero on the fixed dofs) and, above level 0, parents [N_l, 2] int32 (node i = 0.5 (a + b) of level l - 1,
 * a == b for a carried node) with the child lists child_ptr [N_{l-1} + 1] / child (the nodes of level l that name
 * node c of level l - 1, ascending, once per occurrence). c1 / c2 [nlev, degree] are the Chebyshev scalars of
 * diag(w) A per level and sweep (c1[., 0] = 0), Einv [m0, m0] with m0 = bs N_0 the dense inverse of the masked
 * coarsest matrix (zero rows and columns at its fixed dofs). Plain launches, no floating-point atomics, every sum in
 * an order fixed by the sizes alone, rows >= nrows never read or stored.
 * fem_mg_restrict / fem_mg_prolong: the transfer kernels alone, rc = P^T (mask_f o rf) and xf += mask_f o P xc.
 * fem_mg_apply: z = cycle(r) on the context's stream (r is not written).
 * fem_mg_solve [sync]: FEM_MODE_PCG's iteration from the x in place with that z: stop on sqrt(r.z) < tol, hist
 *   [hist_len] (may be NULL) receives sqrt(r.z); FEM_PCG_BREAKDOWN on p.Ap <= 0 or non-finite (x is then not updated
 *   in that iteration) and on r.z <= 0 or non-finite (an underestimated lmax can make the cycle indefinite; r0.z0 < 0
 *   is reported as iteration 1). r0.z0 == 0 (b = 0 with x = 0: the start vector solves the free rows) is
 *   FEM_PCG_CONVERGED with 0 iterations and x untouched, where FEM_MODE_PCG's alpha would be 0 / 0. The host
 *   enqueues `chunk` iterations at a time and reads the state in between. */
typedef struct fem_mg fem_mg;
int fem_mg_restrict(int64_t nc, int64_t nf, int bs, const int32_t* child_ptr, const int32_t* child, const double* wf,
                    const double* rf, double* rc, fem_stream_t stream);
int fem_mg_prolong(int64_t nf, int64_t nc, int bs, const int32_t* parents, const double* wf, const double* xc,
                   double* xf, fem_stream_t stream);
int fem_mg_create(int nlev, int bs, const int64_t* nrows, const void* const* slice_ptr, const void* const* cols,
                  const void* const* dcols, const void* const* vals, const void* const* w, const void* const* parents,
                  const void* const* child_ptr, const void* const* child, int degree, const double* c1,
                  const double* c2, int64_t m0, const double* Einv, fem_stream_t stream, fem_mg** out);
int fem_mg_apply(fem_mg* s, const double* r, double* z);
/* one fused Chebyshev sweep on the work vectors of `level` >= 1 (timing only: the vectors' contents are scratch) */
int fem_mg_sweep(fem_mg* s, int level);
int fem_mg_solve(fem_mg* s, const double* b, double* x, double tol, int max_iter, int chunk, double* hist,
                 int64_t hist_len, int* iters, int* status, double* rz);
/* [sync] fem_pcg_scalars' six values */
int fem_mg_scalars(fem_mg* s, double* out6);
void fem_mg_destroy(fem_mg* s);

/* ------------------------------------------------------------------ modal analysis (csrc/modal.hip)
 * The tall-skinny kernels of the block LOBPCG that SellMatrix.eig_lowest drives for the lowest eigenpairs of
 * K u = lambda M u. Multi-vectors are [n, nv] row-major as above (nv 2, 4 or 8; 16-byte aligned). Plain launches;
 * every reduction is finished in workgroup order by a following one-workgroup launch (bit-reproducible); rows >= n
 * are never read nor stored. */
enum fem_mass_form {
    FEM_MASS_SELL = 0,  /* mass: the plain bs = 1 SELL values of a matrix on the same pattern; M = M_s (x) I_bs */
    FEM_MASS_DIAG = 1   /* mass: a vector d [n]; M = diag(d) (the reference's lumped mass, `solver/solver.py:1126-1134`) */
};
/* Y = K X and Z = M X in one sweep of the pattern: every gathered block column of X is loaded once for both (the
 * reference forms K X column by column and M X by a broadcast, `solver/solver.py:1084-1313` at `:1207-1220`).
 * Column j of Y equals fem_spmm's bit for bit; FEM_MASS_SELL: column j of Z equals fem_spmm on the mass matrix, per
 * component for bs = 3. Arguments as fem_spmm. */
int fem_spmm_km(int64_t nrows, int bs, int nv, const int64_t* slice_ptr, const int32_t* cols, const int16_t* dcols,
                const double* vals, const double* mass, int mass_form, const double* X, double* Y, double* Z,
                fem_stream_t stream);
/* Output buffer of the two reductions below (doubles): G_K [am, am] row-major at 0, G_M at FEM_MODAL_OUT_GM, the norms
 * ||R_j|| [nv] then ||MX_j|| [nv] at FEM_MODAL_OUT_NORMS. */
#define FEM_MODAL_OUT_GM 576
#define FEM_MODAL_OUT_NORMS 1152
#define FEM_MODAL_OUT_LEN 1168
/* doubles of device workspace (per-workgroup partials) that fem_modal_gram and fem_modal_residual share
 * (`solver/solver.py:1084-1313` keeps no such state: its reductions are torch calls) */
int64_t fem_modal_work_len(void);
/* Gram matrices of the basis S = [X W P] (a = 3; 2: [X W]; 1: X alone): G_K = S^T (K S), G_M = S^T (M S), am = a nv,
 * upper triangle summed in a fixed order and mirrored (`solver/solver.py:1084-1313` at `:1207-1221` builds X^T K X
 * and X^T M X with two matmuls). vecs: [host, 9] device pointers X, W, P, KX, KW, KP, MX, MW, MP, the first a of each
 * triple read once. */
int fem_modal_gram(int64_t n, int nv, int a, const double* const* vecs, double* work, double* out,
                   fem_stream_t stream);
/* R = KX - MX diag(theta), W = w o R (w [n]: zero on fixed dofs), and the norms of R_j and MX_j over the rows with
 * w != 0 (`solver/solver.py:1084-1313` has no residual: it runs a fixed number of sweeps). theta [device, nv]. */
int fem_modal_residual(int64_t n, int nv, const double* KX, const double* MX, const double* w, const double* theta,
                       double* W, double* work, double* out, fem_stream_t stream);
/* In place, for the vectors and their K- and M-products alike (`solver/solver.py:1084-1313` at `:1304`, Y @ Z):
 * P <- W C_W + P C_P, X <- X C_X + P with C [device, a nv, nv] row-major = [C_X; C_W; C_P]. a = 2: no old P;
 * a = 1: X alone, P untouched. W, KW and MW are read only. vecs as fem_modal_gram. */
int fem_modal_rotate(int64_t n, int nv, int a, double* const* vecs, const double* C, fem_stream_t stream);

/* ------------------------------------------------------------------ transient dynamics (csrc/transient.hip)
 * The kernels of the implicit Newmark integrator that system.py NewmarkIntegrator drives for
 * M a + C v + K u = f(t), C = alpha M + beta_R K (the reference has no time integration; its only routine on K and M
 * together is `vectorized_modal_solver`, `solver/solver.py:1084-1313`). Same rules as the modal kernels: plain
 * launches, reductions finished in workgroup order by a one-workgroup launch (bit-reproducible), rows >= n never read
 * nor stored. kvals is read in the layout it is held in: layout_a = 0 the plain SELL planes (bs 1 or 3), layout_a = 1
 * the bs = 3 solver layout A (16-bit deltas required). mass / mass_form as fem_spmm_km. */
/* out = cK K + cM M in K's own layout (out may not alias kvals), entries = slice_ptr[nslices]. FEM_MASS_SELL: every
 * block gets cM ms on its bs diagonal components; FEM_MASS_DIAG: only the diagonal entry of each row's own block
 * (slot diagpos - rowptr of the row) gets cM d. Padding entries stay 0. (`solver/solver.py:1084-1313` never forms a
 * combination of K and M.) */
int fem_sell_axpby_mass(int64_t nrows, int bs, int layout_a, int64_t entries, const int64_t* slice_ptr,
                        const int32_t* rowptr, const int32_t* diagpos, const double* kvals, const double* mass,
                        int mass_form, double cK, double cM, double* out, fem_stream_t stream);
/* b = amp F + M Y[:, 1] + K Y[:, 0] for Y [n, 2] row-major (16-byte aligned) in one sweep of the pattern, one
 * accumulator per row (entries in slot order, the K term of an entry before its mass term). kvals NULL: no stiffness
 * damping, the K stream is not read. F NULL: no load. (The reference applies K by `compute_nodal_forces`,
 * `solver/element.py:429-464`, one vector at a time.) */
int fem_newmark_rhs(int64_t nrows, int bs, int layout_a, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* kvals, const double* mass, int mass_form, double amp,
                    const double* F, const double* Y, double* b, fem_stream_t stream);
/* One pass over the vectors after a step's solve, x = u_new on entry. coef [host, 12] = {a0, a2, a3, dt (1 - gamma),
 * dt gamma, mu, mv, ma, ku, kv, ka, dt}:
 *   a <- a0 (x - u) - a2 v - a3 a;  v <- v + coef[3] a_old + coef[4] a;  u <- x;
 *   Y[:, 1] <- mu u + mv v + ma a;  Y[:, 0] <- ku u + kv v + ka a;  predictor != 0: x <- u + dt v
 * Dofs with w = 0 (fixed) are stored as zeros in all six. All vectors [n], Y [n, 2], 16-byte aligned. (No counterpart in
 * the reference, `solver/solver.py`.) */
int fem_newmark_update(int64_t n, const double* coef, int predictor, double* x, double* u, double* v, double* a,
                       const double* w, double* Y, fem_stream_t stream);
/* doubles of device workspace (per-workgroup partials) of fem_quadform_km (`solver/solver.py` keeps no such state) */
int64_t fem_transient_work_len(void);
/* out [device, 2] = (x^T K x, y^T M y) for X = [x | y] [n, 2] row-major in one sweep: the energy
 * E = (out[0] + out[1]) / 2 with X = [u | v] (`solver/solver.py:1084-1313` at `:1207-1221` forms such products with
 * two matmuls). */
int fem_quadform_km(int64_t nrows, int bs, int layout_a, const int64_t* slice_ptr, const int32_t* cols,
                    const int16_t* dcols, const double* kvals, const double* mass, int mass_form, const double* X,
                    double* work, double* out, fem_stream_t stream);

/* ------------------------------------------------------------------ nonlinear statics (csrc/nonlinear.hip)
 * Geometrically nonlinear (total-Lagrangian) c3d4 elasticity -- the K(u) the reference's newton_raphson_solver
 * (`solver/solver.py:978-1065`) takes from its caller, formed here for two hyperelastic materials. With the gradients
 * g_a and volume V of fem_tet4_geom, F = I + sum_a u_a (x) g_a, J = det F, lam / mu the Lame constants of E, nu:
 *   FEM_MAT_SVK          W = lam/2 (tr E)^2 + mu E:E, E = (F^T F - I)/2; P = F S, S = lam tr(E) I + 2 mu E
 *   FEM_MAT_NEO_HOOKEAN  W = mu/2 (F:F - 3) - mu ln J + lam/2 (ln J)^2;  P = mu (F - F^-T) + lam ln J F^-T
 * fem_tet4_nl: per element the consistent tangent Kt (the Hessian of V W in the element's 12 dofs; packed != 0: the
 *   upper 3x3 blocks in fem_iso_ke_sym's layout for npe = 4, which fem_assemble_from_ke_sym consumes; else the full
 *   [M,12,12] whose upper blocks are the packed ones bit for bit and whose lower blocks are their transposes), the
 *   internal forces fe [M,4,3] = V P g_a, the strain energy we [M] = V W, the Cauchy stress sigma [M,6] = J^-1 P F^T in
 *   fem_voigt_to_tensor's order (xx, yy, zz, xy, yz, xz) and detF [M]. Every output may be NULL; Kt == NULL runs a
 *   build without the tangent work (same fe / we bits). An element with det F <= 0 writes zeros to Kt, fe, sigma, +inf
 *   to we, its det F to detF, and lowers *inverted_idx; the other elements are unaffected. *bad_idx: as fem_tet4_ke
 *   (|det[1 x y z]| < 1e-12; the caller raises FEM_ESINGULAR's error); such an element's outputs are those of an
 *   inverted one with detF 0. Both index words are device int64 preset to M. M == 0: FEM_OK, no launch.
 * fem_tet4_nl_gather: fint [N,3] = the element forces summed per node in ascending incidence order (fem_ebe_apply's
 *   order: the same bits on every run, no atomics) and r = load_factor fext - fint, 0 where mask != 0. fint, r and mask
 *   may be NULL. */
enum { FEM_MAT_SVK = 0, FEM_MAT_NEO_HOOKEAN = 1 };
int fem_tet4_nl(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                int material, int packed, double* Kt, double* fe, double* we, double* sigma, double* detF,
                int64_t* bad_idx, int64_t* inverted_idx, fem_stream_t stream);
int fem_tet4_nl_gather(const double* fe, const int32_t* inc_ptr, const int32_t* inc, int64_t N, const double* fext,
                       double load_factor, const uint8_t* mask, double* fint, double* r, fem_stream_t stream);

/* ------------------------------------------------------------------ elastoplastic statics (csrc/plasticity.hip)
 * Small-strain, rate-independent von Mises (J2) plasticity with linear isotropic hardening on c3d4 (no
 * counterpart in the reference, whose materials are all elastic). With the gradients g_a and volume V of fem_tet4_geom,
 * eps = sym(sum_a u_a (x) g_a), mu = E / (2 (1 + nu)), kappa = E / (3 (1 - 2 nu)); every tensor in
 * fem_voigt_to_tensor's order (xx, yy, zz, xy, yz, xz) as TENSOR components (no engineering factor 2). Committed state
 * per element: the plastic strain ep_n [M,6] (deviatoric) and the accumulated plastic strain alpha_n [M] >= 0.
 *   e = dev eps, s_tr = 2 mu (e - ep_n), q_tr = sqrt(3/2) |s_tr|, f_tr = q_tr - (sigma_y + H alpha_n)
 *   f_tr <= 0: s = s_tr, state unchanged, C = kappa 1(x)1 + 2 mu P_dev
 *   f_tr >  0: dgamma = f_tr / (3 mu + H), n = s_tr / |s_tr|, beta = 1 - 3 mu dgamma / q_tr, s = beta s_tr,
 *              ep_n+1 = ep_n + sqrt(3/2) dgamma n, alpha_n+1 = alpha_n + dgamma,
 *              C = kappa 1(x)1 + 2 mu beta P_dev - 2 mu (3 mu / (3 mu + H) - (1 - beta)) n(x)n
 * fem_tet4_j2: per element the consistent tangent Kt = V B^T C B (packed != 0: the upper 3x3 blocks in
 *   fem_iso_ke_sym's layout for npe = 4, which fem_assemble_from_ke_sym consumes; else the full [M,12,12] whose upper
 *   blocks are the packed ones bit for bit and whose lower blocks are their transposes), the forces fe [M,4,3] =
 *   V sigma g_a with sigma = kappa tr(eps) 1 + s, the incremental potential we [M] = V (kappa/2 tr(eps)^2 +
 *   mu |e - ep_n+1|^2 + H/2 alpha_n+1^2 + sigma_y dgamma) whose derivative in the element's 12 displacements is fe while
 *   the committed state is fixed, sigma [M,6], the trial state ep_out [M,6] / alpha_out [M] and plastic [M] = 1 where
 *   f_tr > 0. ep_in == alpha_in == NULL is the virgin state (zeros). Every output may be NULL; Kt == NULL runs a build
 *   without the tangent work (the same bits in every other output). ep_out / alpha_out may alias ep_in / alpha_in: an
 *   element reads and writes only its own slot. *bad_idx (nullable): as fem_tet4_ke (device int64 preset to M,
 *   |det[1 x y z]| < 1e-12); such an element writes zeros to Kt, fe, we, sigma, plastic and copies its input state
 *   through. M == 0: FEM_OK, no launch. FEM_EARG: sigma_y <= 0, H < 0, nu outside (-1, 0.5), only one of ep_in /
 *   alpha_in. H = 0 (perfect plasticity) is accepted; the tangent is then only semi-definite at the limit load.
 *   The residual is gathered from fe by fem_tet4_nl_gather. */
int fem_tet4_j2(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                double sigma_y, double H, const double* ep_in, const double* alpha_in, int packed, double* Kt,
                double* fe, double* we, double* sigma, double* ep_out, double* alpha_out, uint8_t* plastic,
                int64_t* bad_idx, fem_stream_t stream);

/* ------------------------------------------------------------------ shell elements (csrc/shell.hip)
 * Flat s3 / s4 shells with 6 dofs per node (u, v, w, thx, thy, thz) -- the reference's `solver/shell.py`, formulation
 * quirks included: frame unit = [a; b; c] from edge 0->1 and edge 0->2 (npe 3) / 0->3 (npe 4), local
 * coordinates (x - x0) unit^T of which x, y are used, membrane stiffness on local (u, v), a rotation-only bending block
 * on local (thx, thy), zero rows and columns for w and thz.
 *   D6 [host, 6]: (D00, D01, D22) of the membrane block and (D33, D34, D55) of the bending block of the 6x6 material
 *     matrix (compute_kirchoff_D_matrix, `:15-39`).
 *   pts [host, 4 x 4], npe 4 only: per integration point the factors (1 - xi, 1 + xi, 1 - eta, 1 + eta) as the caller
 *     wants them rounded (the reference's K takes the fp32-rounded 1/sqrt(3), `:651-672,840-842`; its summed B rounds
 *     the factors themselves to fp32, `:814-815,692-704`). The weights are 1.
 * fem_shell_ke: Ke of every element, d = 6 npe (compute_s3_K_matrix `:440-453`, compute_s4_K_matrix `:825-861`):
 *     FEM_SHELL_LOCAL   [M, d, d] in the element's frame, rows 6 n + dof
 *     FEM_SHELL_POINTS  [M, d, d, 4], the four points' terms (npe 4; the reference's single=False)
 *     FEM_SHELL_GLOBAL  [M, d, d] = T^T K T, T = blockdiag(unit) per node, in the block order of the 6-dof assembly:
 *                       rows 3 (h npe + n) + i with h = 0 the translations, h = 1 the rotations of node n
 *   and unit [M,3,3]; Ke or unit may be NULL. A degenerate element (zero edge 0->1, a frame whose second edge is
 *   collinear with the first to 1e-12 of its length, a zero or non-finite det J) is FEM_ESINGULAR's condition:
 *   *bad_idx [device int64, preset to M] = the first such element, its outputs are zeros and the caller raises, as
 *   for fem_tet4_ke. A negative det J (an inverted element) is valid and flips the sign like the reference.
 * fem_shell_geom: at one point (pt [host, 4], npe 4) unit [M,3,3], local [M,npe,3], J [M,2,2], grads [M,npe,2],
 *   B [M,6,d] (`:297-438`, `:599-800`); every output and bad_idx may be NULL.
 * fem_shell_apply: y [N,6] = sum_e R_e^T K_e R_e u for local-frame Ke [M,d,d] and unit [M,3,3] -- replaces
 *   compute_shell_nodal_forces (`:58-102`); a row gather over the node -> element incidence in ascending order, no
 *   atomics, the same bits on every run.
 * fem_shell_stress: nmq [M,6] = D B u_e with B summed over the points, applied to the rows of u [N,6] as they are
 *   (compute_s3_shell_stress `:455-468`, compute_s4_shell_stress `:863-876`). */
enum { FEM_SHELL_LOCAL = 0, FEM_SHELL_POINTS = 1, FEM_SHELL_GLOBAL = 2 };
int fem_shell_ke(const double* coords, const int64_t* conn, int64_t M, int npe, const double* D6, const double* pts,
                 int frame, double* Ke, double* unit, int64_t* bad_idx, fem_stream_t stream);
int fem_shell_geom(const double* coords, const int64_t* conn, int64_t M, int npe, const double* pt, double* unit,
                   double* local, double* J, double* grads, double* B, int64_t* bad_idx, fem_stream_t stream);
int fem_shell_apply(const double* Ke, const double* unit, const int64_t* conn, int npe, const int32_t* inc_ptr,
                    const int32_t* inc, int64_t N, const double* u, double* y, fem_stream_t stream);
int fem_shell_stress(const double* coords, const int64_t* conn, int64_t M, int npe, const double* D6,
                     const double* pts, const double* u, double* nmq, int64_t* bad_idx, fem_stream_t stream);

/* ------------------------------------------------------------------ distributed loads (csrc/loads.hip)
 * Physical loads turned into nodal forces, and the stress recovery that takes the thermal strain off. No reference
 * function exists (its solvers take a finished force array): parity unpinned. All fp64; every nodal sum runs over the
 * node -> element incidence in ascending order (no atomics, the same bits on every run, zero rows for nodes without
 * elements). How an optional array is read is given by a FEM_LOAD_* mode:
 *     FEM_LOAD_NONE absent (NULL) | FEM_LOAD_UNIFORM one value ([1], an acceleration or traction [3]) |
 *     FEM_LOAD_NODAL one row per node | FEM_LOAD_ELEMENT one row per element (T) or per face (p, t)
 * All such arrays are device memory. beta = alpha (D00 + 2 D01) with the isotropic D of `solver/element.py:282-306`.
 * fem_tet4_loads: F [N,3], per node the sum over its incident tets of
 *     body     rho V/4 g (uniform) or rho V/20 (a_a + sum_b a_b) (nodal), V = |det|/6 as the consistent mass;
 *     thermal  V beta dT_e grad N_a = V B_a^T D (alpha dT_e m), m = (1,1,1,0,0,0), gradients and V those of
 *              fem_tet4_ke (a uniform dT gives K_e times the expansion field alpha dT x); dT_e = mean of the four
 *              nodal T - T_ref (nodal), T[e] - T_ref (element) or T[0] - T_ref (uniform).
 *   fe == NULL: one node-centred pass that recomputes each incident tet's geometry; fe [M,4,3] given: the two-pass
 *   form (element vectors, then fem_tet4_nl_gather). bad_idx as fem_tet4_ke (nullable, preset to M). M == 0: F = 0.
 * fem_iso_loads: element vectors fe [M,npe,3] of c3d8 / c3d6 / c3d10 (npe 8 / 6 / 10) from shape values Nv
 *   [n_ip,npe], natural derivatives dN [n_ip,npe,3] and weights w [n_ip] (n_ip <= 32); the caller gathers them with
 *   fem_tet4_nl_gather.
 *     body     rho sum_q w_q |detJ_q| N_a(q) a(q), a(q) uniform or interpolated with Nv;
 *     thermal  sum_q c_q beta dT(q) grad N_a(q), c_q = w_q detJ_q (signed, FEM_ISO_SUM) or the wedge volume at the
 *              single point (FEM_ISO_VOLUME, npe 6, n_ip 1) -- fem_iso_ke's factors; dT(q) interpolated with Nv.
 * fem_face_loads: face vectors fv [F,nf,3] of tri3 / quad4 faces (nf 3 / 4) under a pressure p (against the normal) or
 *   a traction t [3] (exactly one, FEM_LOAD_UNIFORM or FEM_LOAD_ELEMENT): tri3 -(p/3) (A n) or (A/3) t per node; quad4
 *   2x2 Gauss on n dA = x_xi x x_eta. The normal is the right-hand normal of the node order, flipped when it points
 *   from the face centroid towards node extra[f] (extra nullable). A face with a repeated node or zero area gives zeros.
 * fem_tet4_stress_thermal / fem_iso_stress_thermal: fem_tet4_stress / fem_iso_stress (layouts 0 and 1, npe 6 / 8) with
 *   sigma = D (B u_e - alpha dT m) and von Mises of that tensor; dT as the loads above (Nv [n_ip,npe] interpolates it
 *   at the points). */
enum { FEM_LOAD_NONE = 0, FEM_LOAD_UNIFORM = 1, FEM_LOAD_NODAL = 2, FEM_LOAD_ELEMENT = 3 };
int fem_tet4_loads(const double* coords, const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc,
                   int64_t N, double rho, const double* accel, int accel_mode, double E, double nu, double alpha,
                   const double* T, int t_mode, double T_ref, double* fe, double* F, int64_t* bad_idx,
                   fem_stream_t stream);
int fem_iso_loads(const double* coords, const int64_t* conn, int64_t M, int npe, const double* Nv, const double* dN,
                  const double* w, int n_ip, int mode, double rho, const double* accel, int accel_mode, double E,
                  double nu, double alpha, const double* T, int t_mode, double T_ref, double* fe,
                  fem_stream_t stream);
int fem_face_loads(const double* coords, const int64_t* faces, int64_t F, int nf, const int64_t* extra,
                   const double* p, int p_mode, const double* t, int t_mode, double* fv, fem_stream_t stream);
int fem_tet4_stress_thermal(const double* coords, const int64_t* conn, int64_t M, const double* u, double E, double nu,
                            double alpha, const double* T, int t_mode, double T_ref, double* sig, double* vm,
                            int64_t* bad_idx, fem_stream_t stream);
int fem_iso_stress_thermal(const double* coords, const int64_t* conn, int64_t M, int npe, const double* u, double E,
                           double nu, double alpha, const double* T, int t_mode, double T_ref, const double* Nv,
                           const double* dN, const double* w, int n_ip, int layout, double* sig, double* vm,
                           fem_stream_t stream);

/* ------------------------------------------------------------------ linear buckling (csrc/buckling.hip)
 * fem_geo_scalar: the geometric (initial-stress) stiffness of c3d4 / c3d6 / c3d8 / c3d10 (npe = 4 / 6 / 8 / 10) as its
 * scalar factor (the reference has no buckling analysis):
 *   Gs[M, npe, npe], Gs_e[a][b] = sum_q w_q |detJ_q| grad N_a(q)^T sigma_q grad N_b(q),  K_g,e = Gs_e (x) I3
 * -- the form of fem_iso_mass_scalar, so assembled as a bs = 1 matrix on the node pattern it takes every `mass` slot
 * (fem_spmm_km, fem_sell_axpby_mass, fem_quadform_km). dN [n_ip, npe, 3] and w [n_ip] as fem_iso_mass_scalar
 * (n_ip <= 32; c3d4: one point, the P1 derivatives, weight 1/6); |detJ_q| with its sign convention. The stress is
 * formed inside the kernel at the points that integrate Gs: sigma_q = D(E, nu) B_q u_e when u [N, 3] is not NULL, plus
 * the per-element constant sigma0 [M, 3, 3] (upper triangle read: what fem_iso_stress layout 0 / fem_tet4_stress
 * write) when that is not NULL; both NULL is FEM_EARG. bad [M] bytes, zeroed by the caller: bad[e] is set to 1 for an
 * element with detJ = 0 or not finite at a point (its block is then meaningless). Gs_e is symmetric bit for bit (the
 * upper triangle is computed and mirrored). No atomics; FEM_EBADTYPE for another npe. */
int fem_geo_scalar(const double* coords, const int64_t* conn, int64_t M, int npe, const double* u, double E, double nu,
                   const double* sigma0, const double* dN, const double* w, int n_ip, double* Gs, uint8_t* bad,
                   fem_stream_t stream);

/* ------------------------------------------------------------------ topology optimisation (csrc/topopt.hip)
 * The design loop of density-based (SIMP) compliance minimisation on c3d4 around fem_assemble_tet4_scaled* and a PCG
 * solve; the reference has no counterpart. All arrays device memory, fp64 unless noted; no atomics but the atomicMin of
 * *bad_idx; every sum in a fixed order (the same bits on every run). V_e, g_a: volume and gradients of fem_tet4_geom;
 * inc entries are 4 e + a (fem_incidence). Nothing past M elements / N nodes of any array is read or written.
 * fem_topopt_work_len: doubles of workspace `work` that fem_tet4_unit_energy and fem_oc_update need for M elements.
 * fem_tet4_volumes: V [M] = |det| / 6 and (Vn != NULL) Vn [N] = sum of V_e over the elements containing the node, in
 *   incidence order (0 for a node without elements). *bad_idx (nullable, preset to M) as fem_tet4_ke.
 * fem_tet4_unit_energy: ce [M] = u_e^T K_e(E = 1, nu) u_e = V_e (lam1 tr(eps)^2 + 2 mu1 eps:eps), eps = sym(sum_a u_a
 *   (x) g_a), u [N,3]. With rho_t [M] (nullable) s_e = s_min + (1 - s_min) rho_t[e]^penal, else s_e = 1; dct [M]
 *   (nullable, needs rho_t) = -penal (1 - s_min) rho_t[e]^(penal - 1) E0 ce[e]; *compliance (nullable, needs work) =
 *   sum_e s_e E0 ce[e], per-block partials in work summed by one block in block order. A degenerate element
 *   (|det| < 1e-12) writes zeros and lowers *bad_idx (required, preset to M). Outputs may not alias inputs.
 * fem_simp_scale: s [M] = s_min + (1 - s_min) rho_t^penal; s may alias rho_t.
 * fem_density_filter: the node-average filter applied `passes` >= 0 times (0: out = in, bit for bit).
 *   forward (adjoint == 0): y[n] = (sum_{e containing n} V_e x_e) / Vn[n], out[e] = 1/4 sum_a y[e_a] -- keeps constants
 *     and the volume sum_e V_e x_e; scale [M] (nullable) also receives fem_simp_scale(out) from the last pass;
 *   adjoint: y[n] = (1/4 sum_{e containing n} x_e) / Vn[n], out[e] = V_e sum_a y[e_a]; scale must be NULL.
 *   node_tmp [N] (passes > 0) and elem_tmp [M] (passes > 1) are overwritten. out may alias in; in is otherwise
 *   untouched. V / Vn from fem_tet4_volumes.
 * fem_oc_update: the optimality-criteria update with its bisection on the device (no copy to the host, no grid
 *   barrier). b_e = max(0, -dc_e) / V_e, lo_e = max(rho_min, rho_e - move), hi_e = min(1, rho_e + move),
 *   rho_new_e(l) = min(hi_e, max(lo_e, rho_e sqrt(b_e / l))). passive [M] (int8, nullable): 0 free, 1 solid (pinned to
 *   1), -1 void (pinned to rho_min); passive elements count in the volume and not in the bracket. Bracket
 *   [rho_min^2 min_{b_e > 0} b_e, max b_e / rho_min^2]; n_bisect steps at l_mid = sqrt(l_lo) sqrt(l_hi): sum_e V_e
 *   rho_new_e(l_mid) > volfrac sum_e V_e moves l_lo up, else l_hi down; rho_new [M] is taken at l_hi. No free b_e > 0:
 *   rho_new = rho. out [2] = (max_e |rho_new_e - rho_e|, sum_e V_e rho_new_e / sum_e V_e). rho_new may alias rho;
 *   rho, dc, V, passive are otherwise untouched; work is overwritten. */
int64_t fem_topopt_work_len(int64_t M);
int fem_tet4_volumes(const double* coords, const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc,
                     int64_t N, double* V, double* Vn, int64_t* bad_idx, fem_stream_t stream);
int fem_tet4_unit_energy(const double* coords, const int64_t* conn, int64_t M, const double* u, double nu,
                         const double* rho_t, double penal, double s_min, double E0, double* ce, double* dct,
                         double* work, double* compliance, int64_t* bad_idx, fem_stream_t stream);
int fem_simp_scale(const double* rho_t, int64_t M, double penal, double s_min, double* s, fem_stream_t stream);
int fem_density_filter(const int64_t* conn, int64_t M, const int32_t* inc_ptr, const int32_t* inc, int64_t N,
                       const double* V, const double* Vn, const double* in, int passes, int adjoint, double penal,
                       double s_min, double* node_tmp, double* elem_tmp, double* out, double* scale,
                       fem_stream_t stream);
int fem_oc_update(const double* rho, const double* dc, const double* V, const int8_t* passive, int64_t M,
                  double volfrac, double move, double rho_min, int n_bisect, double* work, double* rho_new,
                  double* out, fem_stream_t stream);

/* ---- explicit dynamics (csrc/explicit.hip): central differences on the element chunks of a fem_mf layout
 * M a + alpha M v + f_int(u) = amp(t) f_ext with the lumped mass M, integrated in leapfrog form:
 *   v_{n+1/2} = ((1 - alpha dt/2) v_{n-1/2} + dt (amp_n f_ext - f_int(u_n)) / m) / (1 + alpha dt/2),
 *   u_{n+1} = u_n + dt v_{n+1/2};  the first step after a start (or a change of dt) takes v_{1/2} = v_0 + (dt/2) a_0.
 * Materials: FEM_MAT_LINEAR (small strain, the operator of fem_mf_apply), FEM_MAT_SVK, FEM_MAT_NEO_HOOKEAN (total
 * Lagrangian, the forces of fem_tet4_nl). Everything is stream-ordered; only fem_xd_status synchronises.
 * fem_xd_lumped_mass: mass [N] = sum over the node's elements of rho V_e / 4 in the layout's fixed order (0 for a node
 *   of no element). Uses the layout's own scratch: one stream at a time, as fem_mf_apply.
 * fem_xd_stable_dt: dt_e [M] (nullable) = 1 / (c_d sqrt(sum_a |g_a|^2)), c_d^2 = (max(lam, 0) + 2 mu) / rho, and
 *   *dt_min (device) = min_e dt_e (+inf for M == 0) <= 2 / omega_max of the lumped-mass pencil: with the lumped
 *   element mass rho V / 4 the largest element eigenvalue is <= 4 c_d^2 sum_a |g_a|^2. A degenerate element gives 0.
 * fem_xd_create: an integrator on the layout `mf` (FEM_KIND_ELASTIC; its E, nu are the material's; it must outlive
 *   the integrator). mass [N] from fem_xd_lumped_mass, mask [3N] uint8 (nullable; != 0: the dof stays at u = v = a = 0;
 *   a node of zero mass is held as well), alpha >= 0 the mass-proportional damping, u, v, a [3N] the caller's state
 *   arrays: after fem_xd_start and after every fem_xd_run they hold u_n, v_n, a_n of the time reached.
 * fem_xd_start: u <- u0, v <- v0 (NULL: zero), step 0, status cleared, a <- (amp0 fext - f_int(u0)) / m - alpha v0
 *   (fext [3N] nullable).
 * fem_xd_run: nsteps steps of dt from the state reached: two launches per step (force, update) and, on the steps n
 *   with n % energy_every == 0 (n counted from the start), a one-workgroup sum; no host synchronisation. amps (host,
 *   [nsteps + 1], read during the call): the load factor at the run's times t_n .. t_{n + nsteps} (unused with fext
 *   NULL). rec_dofs [nrec] (device, distinct dofs): row k of rec_u / rec_v / rec_a [nsteps, nrec] gets u, v =
 *   (v_{-1/2} + v_{+1/2}) / 2 and a of those dofs at the run's step k (before its advance). energies [rows, 4]
 *   (device): per energy step (kinetic sum m v_n^2 / 2, strain, external power amp f_ext . v_n, amp f_ext . u_n).
 *   Consecutive runs with the same dt continue the same trajectory bit for bit.
 *   An element with det F <= 0 (nonlinear materials) or a degenerate reference element contributes zero force and
 *   records the first such step; the first step that produced a non-finite u or v is recorded too. Neither stops the
 *   run.
 * fem_xd_force: fint [3N] = f_int(u) for any u (the integrator's state is untouched except that an inverted element
 *   is recorded at the current step).
 * fem_xd_status: out2 = (first inverted step, first non-finite step), -1 for none; synchronises the stream.
 * fem_xd_info: out4 = (steps taken since the start, chunks, workgroups of the update, values per energy row). */
enum { FEM_MAT_LINEAR = 2 };
typedef struct fem_xd fem_xd;
int fem_xd_lumped_mass(fem_mf* mf, double rho, double* mass, fem_stream_t stream);
int fem_xd_stable_dt(const double* coords, const int64_t* conn, int64_t M, double E, double nu, double rho,
                     double* dt_e, double* dt_min, fem_stream_t stream);
int fem_xd_create(fem_mf* mf, int material, double rho, const double* mass, const uint8_t* mask, double alpha,
                  double* u, double* v, double* a, fem_stream_t stream, fem_xd** out);
int fem_xd_destroy(fem_xd* h);
int fem_xd_start(fem_xd* h, const double* u0, const double* v0, const double* fext, double amp0,
                 fem_stream_t stream);
int fem_xd_run(fem_xd* h, int64_t nsteps, double dt, const double* amps, const double* fext, int64_t nrec,
               const int64_t* rec_dofs, double* rec_u, double* rec_v, double* rec_a, int64_t energy_every,
               double* energies, fem_stream_t stream);
int fem_xd_force(fem_xd* h, const double* u, double* fint, fem_stream_t stream);
int fem_xd_status(fem_xd* h, int64_t* out2, fem_stream_t stream);
int fem_xd_info(fem_xd* h, int64_t* out4);

/* ---- explicit dynamics: frictional penalty contact of the mesh nodes with up to FEM_XD_MAX_SURFACES rigid analytic
 * surfaces that may translate (csrc/explicit.hip, k_xd_update_c). x = X + u_n is a node's position.
 *   plane     g = (x - c) . n (n points into the side the body may occupy), nu = n
 *   sphere    r = x - c, g = |r| - R, nu = r / |r|; inside (a cavity): g = R - |r|, nu = -r / |r|
 *   cylinder  infinite, axis through c along n: r = (x - c) - ((x - c) . n) n, g and nu as for the sphere
 * A node with |r| = 0, with g >= 0 or of zero mass gets no force. Normal force f_n = k p nu, p = max(0, -g),
 * k = kappa m / dt^2 (m the node's lumped mass, dt the run's step). Friction, for the touched surfaces in index order:
 * f_t = -min(mu |f_n|, m |vt| / sigma) vt / |vt|, vt the tangential part of v* - w, v* the new half-step velocity formed
 * with every normal force and the friction of the surfaces before, w the surface velocity, sigma = dt c2 (dt / 2 in the
 * first step after a start or a change of dt): friction never reverses sliding. Components on held dofs are dropped
 * (v* is 0 there). The step's force is amp f_ext - f_int + f_c; everything else is as in fem_xd_run.
 * fem_xd_contact: attach (nsurf = 1 .. 8) or clear (nsurf = 0) the contact set. surfaces (host, [nsurf, 13], read
 *   during the call): kind (FEM_SURF_*), inside (0 / 1), c (3), n (3: unit normal or axis; unused for a sphere),
 *   R (> 0; unused for a plane), mu >= 0, and the velocity (3) a fem_xd_start uses. 0 < kappa < 4; kappa <=
 *   4 (1 - s^2) keeps omega dt <= 2 when dt = s x the bound of fem_xd_stable_dt. dt0 > 0: the step of the penalty
 *   stiffness and friction cap at a fem_xd_start, whose a_0 then includes the contact force at the attached positions.
 *   node_word (device, [N] uint8, nullable = every surface; it must outlive the set): bit s set -> the node may touch
 *   surface s. With a set attached fem_xd_run is refused: fem_xd_run_contact takes the motion.
 * fem_xd_run_contact: fem_xd_run with the set's motion. offsets, velocities (host, [nsteps + 1, nsurf, 3], read during
 *   the call): surface s stands at c + offsets[k][s] with velocity velocities[k][s] during the run's step k; row nsteps
 *   serves the closing evaluation of v_n, a_n. No launch is added outside history and energy steps and nothing
 *   synchronises. history (device, [rows, nsurf, 5]): on the steps n with n % contact_every == 0 (n from the start; 0:
 *   none) per surface the reaction on it (-sum of the contact force its nodes received, 3 values), the number of nodes
 *   in contact and the largest penetration. contact_energies (device, [energy rows, 3]): on the energy steps the
 *   penalty energy sum k p^2 / 2, the friction power sum f_t . (v_n - w) and the power of the moving surfaces
 *   sum f_c . w. On those steps the kinetic energy and the two load terms of `energies` are summed per node, not per
 *   dof: they may differ from fem_xd_run's in the last bits; u, v, a and the recorded rows of a run whose surfaces are
 *   never touched are fem_xd_run's bit for bit. */
enum { FEM_SURF_PLANE = 0, FEM_SURF_SPHERE = 1, FEM_SURF_CYLINDER = 2 };
enum { FEM_XD_MAX_SURFACES = 8 };
int fem_xd_contact(fem_xd* h, int64_t nsurf, const double* surfaces, double kappa, double dt0,
                   const uint8_t* node_word, fem_stream_t stream);
int fem_xd_run_contact(fem_xd* h, int64_t nsteps, double dt, const double* amps, const double* fext, int64_t nrec,
                       const int64_t* rec_dofs, double* rec_u, double* rec_v, double* rec_a, int64_t energy_every,
                       double* energies, const double* offsets, const double* velocities, int64_t contact_every,
                       double* history, double* contact_energies, fem_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEM355_H */
