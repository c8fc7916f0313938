"""Multi-GPU persistent Jacobi-PCG: the single-GPU persistent schedule (csrc/pcg_persist.hpp) spread over ranks by
ROWS, with every per-iteration exchange done inside the running kernels (no collective library call per iteration).

The reference has no multi-device code (its only decomposition is the single-GPU region growing of
`subdivision.ipynb:194-297`); this is the MI355X-native counterpart of DESIGN.md §6's element-partitioned RCCL path
for the bs = 1 (Poisson) system, designed for the strong-scaling target of SURVEY §8(e):
  * partition: the global SELL-64 slices split into `nranks` contiguous ranges of (nearly) equal size; rank r owns
    the rows of its slices. The ordering of the rows (lexicographic on the Kuhn cube, RCM-like on meshes from
    `mesh.py`) keeps the rows a rank gathers from others within a band next to its range;
  * each rank assembles the GLOBAL rows it owns from the elements touching them (global node ids, rows of other
    ranks left partial and never read), so the matrix rows, the Jacobi weights and every per-row operation are
    those of the single-GPU system;
  * every rank's comm block (u, per-workgroup epoch flags, rank sums) is mapped into every other rank through
    hipIpc handles; a workgroup whose rows another rank gathers stores them into that rank's u with system-scope
    stores, releases, and raises its flag there; the grid barrier of every iteration is followed by a rank-level
    exchange of the two sums, summed in rank order on every rank (identical scalars everywhere, deterministic);
  * one process per GPU (bench.py N > 1), or - for validation on one GPU - several ranks as contexts of one process
    on separate streams sharing the CUs (`EmulatedGroup`), or several processes on one GPU (`FEM355_DIST_SAME_GPU`).
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass

import torch

from . import _capi as C
from . import system as _sys

F64, I64 = torch.float64, torch.int64


def slice_split(n_rows: int, nranks: int):
    """Global slice bounds [nranks + 1] of the row partition (contiguous, sizes within one slice of each other)."""
    ns = (n_rows + 63) // 64
    if ns < nranks:
        raise ValueError(f"{n_rows} rows ({ns} slices) cannot be split over {nranks} ranks")
    return [r * ns // nranks for r in range(nranks + 1)]


def rank_rows(n_rows: int, split, rank: int):
    return split[rank] * 64, min(split[rank + 1] * 64, n_rows)


def rank_elements(elements: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    """Elements with at least one node among the rows [lo, hi) (their global connectivity)."""
    return elements[((elements >= lo) & (elements < hi)).any(dim=1)].contiguous()


@dataclass
class RankSetup:
    A: "_sys.SellMatrix"
    w: torch.Tensor
    lo: int
    hi: int


def assemble_rank(coords, elements, split, rank, kind="poisson", E=1.0, nu=0.0, fixed_mask=None) -> RankSetup:
    """The global rows [lo, hi) of rank `rank`: pattern + values from the elements touching them, Jacobi weights
    (zero on fixed dofs, uint8 mask over the global dofs). kind "poisson" (bs = 1) or "elastic" (bs = 3: the block
    rows of the rank's nodes, k_pcg_persist3)."""
    N = coords.shape[0]
    lo, hi = rank_rows(N, split, rank)
    el = rank_elements(elements, lo, hi)
    A = _sys.assemble_tet4_system(coords, el, kind, E, nu)
    if A.g.dcols is None:
        raise ValueError("the distributed persistent schedule needs 16-bit column deltas (banded rows)")
    w = A.jacobi(fixed_mask)
    return RankSetup(A, w, lo, hi)


class RankRunner:
    """One rank's persistent PCG context over its rows of the global system (vectors global-length)."""

    TUNE_DEFAULT, TUNE_DIST_FINE, TUNE_DIST_DROP = 1 | 2 | 4 | 8 | 128, 64, 512

    def __init__(self, rs: RankSetup, b, split, rank, nranks, tol=0.0, mode=C.MODE_PCG, eps=1e-30, grid=0,
                 stream=None, x0=None, fine=False, drop=None, gv=False):
        """gv: the pipelined (Ghysels-Vanroose) DIST build (FEM_TUNE_PK_GV; bs = 1, PCG mode, <= 2 slices per wave
        on this rank -- else the single-reduction build runs, see pipelined())."""
        self.lib = C.lib()
        A = rs.A
        self.A, self.rs, self.rank, self.nranks = A, rs, rank, nranks
        self.device = A.device
        self.b = b.to(device=A.device, dtype=F64).contiguous().view(-1)
        self.w = rs.w
        self.x = (torch.zeros(A.n, dtype=F64, device=A.device) if x0 is None
                  else x0.to(device=A.device, dtype=F64).clone().contiguous().view(-1))
        self.stream = stream if stream is not None else torch.cuda.Stream(device=A.device)
        self.stream.wait_stream(torch.cuda.current_stream(A.device))
        self.h = ctypes.c_void_p()
        with C.device_scope(A.device):
            C.check(self.lib.fem_pcg_create(A.g.n_nodes, A.bs, C.ptr(A.g.slice_ptr), C.ptr(A.g.cols),
                                            C.ptr(A.plain_values()), C.ptr(self.b), C.ptr(self.x), C.ptr(self.w), mode, float(tol), float(eps),
                                            None, 0, ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(self.h)),
                    "fem_pcg_create")
            C.check(self.lib.fem_pcg_set_entries(self.h, A.g.sell_entries), "fem_pcg_set_entries")
            A.attach_cols16(self.h)
            # plain_values() above may have formed the plain copy on the current stream: ordered before this stream
            self.stream.wait_stream(torch.cuda.current_stream(A.device))
            # fine: comm block in fine-grained memory (coherent for the other GPUs' accesses; the default until a
            # real multi-GPU run has shown hipMalloc memory coherent there too). drop: fault injection (tests) --
            # this rank publishes nothing; FEM355_DIST_DROP_RANK=r selects rank r from the environment
            if drop is None:
                drop = os.environ.get("FEM355_DIST_DROP_RANK", "") == str(rank)
                if drop:   # fault injection from the environment is never silent (bench.py labels its line too)
                    print(f"[rank {rank}] FAULT INJECTION ACTIVE: FEM355_DIST_DROP_RANK={rank} -- this rank publishes "
                          "nothing; every persistent multi-GPU launch will time out", file=sys.stderr, flush=True)
            if fine or drop or gv:   # (before fem_pcg_set_rows: the pipelined build's comm block has a second m region)
                C.check(self.lib.fem_pcg_set_tuning(self.h, self.TUNE_DEFAULT | (self.TUNE_DIST_FINE if fine else 0)
                                                    | (self.TUNE_DIST_DROP if drop else 0)
                                                    | (C.TUNE_PK_GV if gv else 0)), "fem_pcg_set_tuning")
            sp = (ctypes.c_int64 * (nranks + 1))(*split)
            C.check(self.lib.fem_pcg_set_rows(self.h, nranks, rank, sp, int(grid)), "fem_pcg_set_rows")
            base, nbytes = ctypes.c_void_p(), ctypes.c_int64()
            C.check(self.lib.fem_pcg_comm_block(self.h, ctypes.byref(base), ctypes.byref(nbytes)), "fem_pcg_comm_block")
            self.block = base.value
            self.block_bytes = nbytes.value
            lo, hi = ctypes.c_int64(), ctypes.c_int64()
            C.check(self.lib.fem_pcg_col_window(self.h, ctypes.byref(lo), ctypes.byref(hi)), "fem_pcg_col_window")
            self.col_window = (lo.value, hi.value)

    def ipc_handle(self) -> bytes:
        buf = ctypes.create_string_buffer(64)
        C.check(self.lib.fem_ipc_handle(ctypes.c_void_p(self.block), buf), "fem_ipc_handle")
        return bytes(buf.raw)

    def set_peers(self, bases, windows):
        n = self.nranks
        arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(b) if b else None for b in bases])
        los = (ctypes.c_int64 * n)(*[w[0] for w in windows])
        his = (ctypes.c_int64 * n)(*[w[1] for w in windows])
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_set_peers(self.h, arr, los, his), "fem_pcg_set_peers")

    def start(self):
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_start(self.h), "fem_pcg_start")

    def iterate(self, k):
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_iterate(self.h, int(k)), "fem_pcg_iterate")

    def profile(self, k):
        """k iterations as one launch, hip events around it on the solver stream -> device ms."""
        ms = (ctypes.c_double * 3)()
        cnt = (ctypes.c_int * 3)()
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_profile(self.h, int(k), int(k), ms, cnt), "fem_pcg_profile")
        return ms[0]

    def poll(self):
        it, stt, rz = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_poll(self.h, ctypes.byref(it), ctypes.byref(stt), ctypes.byref(rz)),
                    "fem_pcg_poll")
        return it.value, stt.value, rz.value

    def sync_site(self):
        v = ctypes.c_int()
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_sync_site(self.h, ctypes.byref(v)), "fem_pcg_sync_site")
        return v.value

    def effective_schedule(self):
        return int(self.lib.fem_pcg_get_schedule(self.h))

    def pipelined(self):
        """True when the started rank runs the pipelined DIST build."""
        on = ctypes.c_int()
        C.check(self.lib.fem_pcg_pipelined(self.h, ctypes.byref(on)), "fem_pcg_pipelined")
        return bool(on.value)

    def persist_build(self):
        """(register slots per wave, overflow build, packed slices per wave) of the started rank's launches."""
        sl, ov, pk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        C.check(self.lib.fem_pcg_persist_build(self.h, ctypes.byref(sl), ctypes.byref(ov), ctypes.byref(pk)),
                "fem_pcg_persist_build")
        return sl.value, ov.value, pk.value

    def debug(self, which, n):
        buf = (ctypes.c_int32 * n)()
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_dist_debug(self.h, int(which), buf, int(n)), "fem_pcg_dist_debug")
        return list(buf)

    def set_prof(self, buf):
        with C.device_scope(self.device):
            C.check(self.lib.fem_pcg_set_prof(self.h, C.ptr(buf)), "fem_pcg_set_prof")

    def own_x(self):
        bs = self.A.bs
        return self.x[self.rs.lo * bs:self.rs.hi * bs]

    def close(self):
        if self.h:
            self.lib.fem_pcg_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EmulatedGroup:
    """`nranks` ranks as contexts of ONE process on ONE GPU (validation of the distributed kernel without a
    multi-GPU box): each rank gets grid = CUs / nranks workgroups and its own stream, so the ranks' persistent
    launches run concurrently; the comm blocks are plain device pointers (no IPC)."""

    def __init__(self, coords, elements, nranks, b, fixed_mask=None, kind="poisson", E=1.0, nu=0.0, tol=0.0,
                 mode=C.MODE_PCG, x0=None, fine=False, drop_rank=-1, gv=False):
        dev = coords.device
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        # a multiple of 8 workgroups per rank within its CU-mask share (at 3+ ranks leave headroom: the masks are
        # laid over the CU numbering, which need not split evenly into usable CUs)
        grid = (ncu // nranks) // 8 * 8 if nranks <= 2 else int(ncu / nranks * 0.85) // 8 * 8
        N = coords.shape[0]
        self.split = slice_split(N, nranks)
        self.ranks = []
        self._raw_streams = []
        lib = C.lib()
        for r in range(nranks):
            # a CU-masked stream per rank: its own hardware queue and its own CUs, so the ranks' launches run side by
            # side (plain streams may share a queue and then serialise: the first rank would wait for the second)
            raw = ctypes.c_void_p()
            with C.device_scope(dev):
                C.check(lib.fem_stream_create_cu(r, nranks, ctypes.byref(raw)), "fem_stream_create_cu")
            self._raw_streams.append(raw.value)
            st = torch.cuda.ExternalStream(raw.value, device=dev)
            rs = assemble_rank(coords, elements, self.split, r, kind, E, nu, fixed_mask)
            self.ranks.append(RankRunner(rs, b, self.split, r, nranks, tol=tol, mode=mode, grid=grid, x0=x0,
                                         stream=st, fine=fine, drop=(r == drop_rank), gv=gv))
        torch.cuda.synchronize(dev)
        bases = [rr.block for rr in self.ranks]
        windows = [rr.col_window for rr in self.ranks]
        for rr in self.ranks:
            rr.set_peers(bases, windows)
        self.n = N

    def start(self):
        for rr in self.ranks:
            rr.start()
        torch.cuda.synchronize()   # the host barrier between every rank's start and any rank's launch

    def iterate(self, k):
        for rr in self.ranks:   # one launch per rank, each on its own stream: they run concurrently
            rr.iterate(k)
        torch.cuda.synchronize()

    def poll_ranks(self):
        return [rr.poll() for rr in self.ranks]

    def poll(self):
        polls = self.poll_ranks()
        its = {p[0] for p in polls}
        sts = {p[1] for p in polls}
        assert len(its) == 1 and len(sts) == 1, f"ranks disagree: {polls}"
        return polls[0]

    def solve(self, max_iter=20000, chunk=512):
        self.start()
        done, it, stt = 0, 0, C.PCG_RUNNING
        while done < max_iter:
            k = min(chunk, max_iter - done)
            self.iterate(k)
            done += k
            it, stt, _ = self.poll()
            if stt != C.PCG_RUNNING:
                break
        return it, stt

    def x(self):
        bs = self.ranks[0].A.bs
        out = torch.empty(self.n * bs, dtype=F64, device=self.ranks[0].x.device)
        for rr in self.ranks:
            out[rr.rs.lo * bs:rr.rs.hi * bs] = rr.own_x()
        return out

    def close(self):
        for rr in self.ranks:
            rr.close()
        torch.cuda.synchronize()
        for raw in self._raw_streams:
            C.lib().fem_stream_destroy(ctypes.c_void_p(raw))
        self._raw_streams = []


# ============================================================================ one process per GPU (bench.py N > 1)
def connect(run: RankRunner, tdist, rank: int, world: int):
    """Exchange comm-block IPC handles and column windows over torch.distributed (gloo), map the other ranks'
    blocks into this process, hand them to the kernel. Returns the opened mappings (close with `disconnect`)."""
    mine = (run.ipc_handle(), run.col_window)
    allv = [None] * world
    tdist.all_gather_object(allv, mine)
    lib = C.lib()
    bases, opened, err = [], [], ""
    with C.device_scope(run.device):
        for q, (h, _) in enumerate(allv):
            if q == rank:
                bases.append(run.block)
                continue
            p = ctypes.c_void_p()
            rc = lib.fem_ipc_open(h, ctypes.byref(p))
            if rc != C.FEM_OK:   # e.g. no peer access between these GPUs
                err = f"rank {rank}: fem_ipc_open of rank {q}'s block: {(lib.fem_last_error() or b'').decode()}"
                break
            bases.append(p.value)
            opened.append(p.value)
    # every rank learns whether every rank could map every block, so they all leave (or all stay) together
    fail = torch.tensor([1 if err else 0], dtype=torch.int32)
    tdist.all_reduce(fail, op=tdist.ReduceOp.MAX)
    if int(fail[0]):
        disconnect(opened, run.device)
        raise C.FemError(err or "another rank could not map the comm blocks")
    run.set_peers(bases, [w for _, w in allv])
    return opened


def disconnect(opened, dev):
    lib = C.lib()
    with C.device_scope(dev):
        for p in opened:
            lib.fem_ipc_close(ctypes.c_void_p(p))


# comm-block variants tried in order by bench_persist: fine-grained device memory first (coherent for peer GPUs by
# construction), hipMalloc memory second (faster local polls, coherence across GPUs not yet shown on hardware)
ATTEMPTS = ("fine-grained", "coarse-grained")


def bench_persist(a, metric, rank, world, dev, tdist, same_gpu=False, kind="poisson"):
    """bench.py at N > 1 on the persistent multi-GPU schedule: the 10M-tet Poisson (bs = 1, k_pcg_persist) or
    elasticity (bs = 3, k_pcg_persist3) system row-partitioned over the ranks (strong scaling), self-checked against
    the single-GPU persistent solve on rank 0's GPU before it is timed. Returns (True, the bench dict on rank 0 / None
    elsewhere), or (False, None) when the check fails, so the caller can measure the RCCL path instead; raises
    C.FemError on every rank alike when the schedule does not apply (a rank's slices past the on-chip capacity)."""
    import os
    import sys
    import time
    from . import mesh as _mesh

    def barrier_sync():
        torch.cuda.synchronize(dev)
        tdist.barrier()

    def tmax(v):
        t = torch.tensor([v], dtype=torch.float64)
        tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        return float(t[0])

    def tmin(v):
        t = torch.tensor([v], dtype=torch.float64)
        tdist.all_reduce(t, op=tdist.ReduceOp.MIN)
        return float(t[0])

    def tsum(v):
        t = torch.tensor([v], dtype=torch.float64)
        tdist.all_reduce(t)
        return float(t[0])

    lib = C.lib()
    raw_stream = None
    grid = 0
    if same_gpu:   # validation: all ranks on one GPU, each on its own CU share (CU-masked stream)
        raw = ctypes.c_void_p()
        with C.device_scope(dev):
            C.check(lib.fem_stream_create_cu(rank, world, ctypes.byref(raw)), "fem_stream_create_cu")
        raw_stream = raw.value
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        grid = (ncu // world) // 8 * 8

    def stream():
        return torch.cuda.ExternalStream(raw_stream, device=dev) if raw_stream else torch.cuda.Stream(device=dev)

    def release_stream():
        if raw_stream:
            torch.cuda.synchronize(dev)
            lib.fem_stream_destroy(ctypes.c_void_p(raw_stream))

    fine = True   # comm-block variant of the current attempt (see ATTEMPTS)
    # bench.py --pipelined 1 (opt-in): the pipelined DIST build (Poisson); its iterates leave the single-reduction
    # ones at rounding level, so the self-check compares against the single-GPU pipelined solve at 1e-8
    gv = bool(getattr(a, "pipelined", 0)) and kind == "poisson"
    check_tol = 1e-8 if gv else 1e-10

    bs = 1 if kind == "poisson" else 3
    E, nu = (1.0, 0.0) if kind == "poisson" else (113.8e9, 0.342)
    if bs == 3:   # on-chip capacity of k_pcg_persist3 (no overflow build across ranks): decided alike on every rank
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        ns = ((a.n + 1) ** 3 + 63) // 64
        cap = (grid or (ncu // 8) * 8) * 16 * 2
        if (ns + world - 1) // world > cap:
            raise C.FemError(f"{(ns + world - 1) // world} slices per rank exceed the bs = 3 on-chip capacity {cap}")

    def case(coords):
        f, fixed = _mesh.cube_poisson_case(coords) if kind == "poisson" else _mesh.cube_elasticity_case(coords)
        gm = torch.zeros((coords.shape[0], bs), dtype=torch.uint8, device=dev)
        gm[fixed] = 1
        return f.reshape(-1).to(F64).contiguous(), gm.view(-1)

    def solve(coords, tets, b, gmask, rtol, max_iter=20000, chunk=8192):
        N = coords.shape[0]
        split = slice_split(N, world)
        rs = assemble_rank(coords, tets, split, rank, kind, E, nu, fixed_mask=gmask)
        lo, hi = rs.lo * bs, rs.hi * bs
        bz = tsum(float(torch.dot(b[lo:hi], (rs.w * b)[lo:hi])))
        tol = rtol * bz ** 0.5
        run = RankRunner(rs, b, split, rank, world, tol=tol, grid=grid, stream=stream(), fine=fine, gv=gv)
        opened = connect(run, tdist, rank, world)
        barrier_sync()
        t0 = time.perf_counter()
        run.start()
        barrier_sync()   # every rank's start (zeroed words) before any rank's first launch
        done, it, stt = 0, 0, C.PCG_RUNNING
        while done < max_iter:
            k = min(chunk, max_iter - done)
            run.iterate(k)
            done += k
            it, stt, _ = run.poll()
            if stt != C.PCG_RUNNING:   # converged, or a bounded wait gave up (FEM_PCG_SYNC_TIMEOUT): one launch
                break
        barrier_sync()
        t_solve = tmax(time.perf_counter() - t0)
        x_own = run.own_x().clone()
        barrier_sync()
        disconnect(opened, dev)
        run.close()
        return rs, x_own, it, stt, t_solve, split

    # warm the rank-local kernels (module loads, first-launch costs) before the assembly is timed
    c0, t0_ = _mesh.kuhn_cube(20, device=dev)
    b0, m0 = case(c0)
    assemble_rank(c0, t0_, slice_split(c0.shape[0], world), rank, kind, E, nu, fixed_mask=m0)

    coords, tets = _mesh.kuhn_cube(a.n, device=dev)
    N = coords.shape[0]
    b, gmask = case(coords)
    barrier_sync()
    t0 = time.perf_counter()
    split = slice_split(N, world)
    rs = assemble_rank(coords, tets, split, rank, kind, E, nu, fixed_mask=gmask)
    barrier_sync()
    t_asm = tmax(time.perf_counter() - t0)
    del rs
    # self-check against the single-GPU persistent solve on rank 0's GPU (the iterates may differ only by the
    # grouping of the partial sums): a mapping or coherence problem of the real transport shows up here. Attempts
    # in ATTEMPTS order; each first solves the small warm-up cube (a transport that does not work gives up there,
    # within one bounded launch: DESIGN.md §6.1 budget), then the full system. All fail -> the caller measures RCCL.
    ref_x = None
    if rank == 0:
        from . import system as _system
        A = _system.assemble_tet4_system(coords, tets, kind, E, nu)
        w = A.jacobi(gmask)
        tol = a.rtol * float(torch.sqrt(torch.dot(b, w * b)))
        ref = A.pcg(b, w=w, tol=tol, max_iter=20000, schedule=3,
                    tune=(C.TUNE_DEFAULT | C.TUNE_PK_GV) if gv else None)
        ref_x, ref_it, ref_st = ref.x.cpu(), ref.iterations, ref.status
        del A, w, ref
    verdict = [0, "not run"]
    attempts_log = []
    for attempt in ATTEMPTS:
        fine = attempt == "fine-grained"
        ta = time.perf_counter()
        _, _, it0, st0, _, _ = solve(c0, t0_, b0, m0, 1e-6)
        warm_ok = tmin(1.0 if st0 == C.PCG_CONVERGED else 0.0) > 0
        if not warm_ok:
            verdict = [0, f"{attempt} comm blocks: warm-up solve status {st0} after {it0} iterations"]
        else:
            rs, x_own, it, stt, t_solve, split = solve(coords, tets, b, gmask, a.rtol)
            parts = [None] * world
            tdist.all_gather_object(parts, (rs.lo, rs.hi, x_own.cpu()))
            ok, why = 1, ""
            if rank == 0:
                x = torch.empty(N * bs, dtype=F64)
                for lo, hi, xp in parts:
                    x[lo * bs:hi * bs] = xp
                err = float((x - ref_x).abs().max() / ref_x.abs().max())
                ok = int(stt == C.PCG_CONVERGED and ref_st == C.PCG_CONVERGED and abs(it - ref_it) <= 1 and err < check_tol)
                why = f"{attempt} comm blocks: status {stt} / {ref_st}, iterations {it} / {ref_it}, x rel diff {err:.3e}"
            verdict = [ok, why]
            tdist.broadcast_object_list(verdict, src=0)
        attempts_log.append({"comm_block": attempt, "ok": bool(verdict[0]), "why": verdict[1],
                             "seconds": round(tmax(time.perf_counter() - ta), 3)})
        if verdict[0]:
            break
        print(f"[rank {rank}] persistent multi-GPU schedule failed its self-check ({verdict[1]})", file=sys.stderr,
              flush=True)
    del c0, t0_, b0, m0
    if not verdict[0]:
        print(f"[rank {rank}] measuring the RCCL path instead", file=sys.stderr, flush=True)
        release_stream()
        return False, None

    # fixed-iteration timing: W warm-up steps, then exactly K steps as one launch per rank, max over ranks
    run = RankRunner(rs, b, split, rank, world, tol=0.0, grid=grid, stream=stream(), fine=fine, gv=gv)
    opened = connect(run, tdist, rank, world)
    barrier_sync()
    run.start()
    pipelined = tmin(1.0 if run.pipelined() else 0.0) > 0
    barrier_sync()
    if a.warmup > 0:
        run.profile(a.warmup)
    barrier_sync()
    t0 = time.perf_counter()
    ms = run.profile(a.steps)
    barrier_sync()
    dt = tmax(time.perf_counter() - t0)
    it2, stt2, _ = run.poll()
    ms_max = tmax(ms)
    # column-index bytes of this rank's slices as stored (slice-uniform delta lists where they qualify)
    n_uni, _, idx_own = _sys.uniform_slices(run.lib, run.h, split[rank], split[rank + 1])
    barrier_sync()
    disconnect(opened, dev)
    A = rs.A
    lo, hi = rs.lo, rs.hi
    nnz_own = int(A.g.rowptr[hi] - A.g.rowptr[lo])
    n_own = hi - lo
    # this rank's bytes per iteration (with the stored format's index bytes)
    alg_own = 8 * bs * bs * nnz_own + (idx_own if n_uni else 2 * nnz_own) + 4 * (n_own + 1) + 16 * n_own * bs
    alg_total = tsum(float(alg_own))
    run.close()
    # every rank must have run exactly the W + K iterations of the timed launches: a launch that gave up
    # (FEM_PCG_SYNC_TIMEOUT) or stopped early on any rank publishes nothing; the caller measures RCCL instead
    ok_steps = tmin(1.0 if (it2 == a.warmup + a.steps and stt2 == C.PCG_RUNNING) else 0.0) > 0
    if not ok_steps:
        print(f"[rank {rank}] persistent multi-GPU timed launch did not complete its steps (iterations {it2}, "
              f"status {stt2}); measuring the RCCL path instead", file=sys.stderr, flush=True)
        release_stream()
        return False, None
    out = None
    if rank == 0:
        per_it = ms_max * 1e-3 / a.steps
        achieved = alg_own / per_it / 1e9
        from . import system as _system
        ceiling = _system.stream_ceiling(dev)
        out = {
            "metric": metric, "value": a.steps / dt, "unit": "CG iterations/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{tets.shape[0]:,}-tet P1 {kind} Kuhn cube n={a.n}, Jacobi-PCG fixed "
                                   f"iterations, rows partitioned over {world} GPUs, persistent schedule per GPU with "
                                   "in-kernel hand-offs over xGMI (IPC-mapped comm blocks), no collective per "
                                   "iteration" + (" [ranks emulated on ONE GPU]" if same_gpu else ""),
                       "tets": int(tets.shape[0]), "dofs": N * bs, "parallelism": f"row partition x{world}",
                       "comm_block": "fine-grained" if fine else "coarse-grained (hipMalloc)",
                       "self_check": verdict[1], "attempts": attempts_log},
            "dofs_per_s": N * bs / (t_asm + t_solve), "assembly_ms": t_asm * 1e3, "solve_ms": t_solve * 1e3,
            "solve_iters": it, "solve_status": stt, "pipelined": pipelined,
            "kernel_ms": {"persist_iteration_max_over_ranks": per_it * 1e3, "iterations_per_launch": a.steps},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                         "frac": achieved / 8000.0, "traffic": None,
                         "kernel": ("k_pcg_persist_gv" if pipelined else "k_pcg_persist" if bs == 1 else "k_pcg_persist3")
                                   + "<DIST> (rank 0's rows; per GPU)",
                         "algorithmic_bytes": alg_own,
                         "algorithmic_bytes_all_ranks": alg_total,
                         "aggregate_GBps": alg_total / per_it / 1e9,
                         "per": "iteration (whole PCG iteration in the persistent kernel)",
                         "stream_ceiling_GBps": ceiling, "frac_of_stream_read": achieved / ceiling["read"]},
            "cpu_baseline": None,
        }
    release_stream()
    return True, out
