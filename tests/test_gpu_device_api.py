"""GPU tests of the device API (include/nccl_device.h): kernels of the caller's own that read and write peers' windows
and synchronise through LSA barriers. The kernels are tests/native/devapi_kernels.hip (libdevapi_kernels.so, launched
through ctypes); expected values come from numpy, compared bit for bit.

Ranks share the box's one GPU: in one process (ncclCommInitAll with a repeated device; at most 4 ranks, every kernel on a
stream with a hardware queue of its own, nccl_amd.dedicated_stream(), since the ranks spin on each other) or as spawned
processes (8 ranks only so). Buffers carry guard bytes in front and behind, checked unchanged."""
import ctypes
import multiprocessing as mp
import os
import queue
import subprocess

import numpy as np

import pytest

from tests.test_gpu_broadcast import FILL, Buf, _comms, _destroy, _torch

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLIB = os.path.join(ROOT, "tests", "native", "libdevapi_kernels.so")

COUNTS = (1, 511, 4097, (1 << 18) + 3)
GRIDS = (1, 4)
SEND_OFF, RECV_OFF = 16, 32     # byte offsets into the windows the kernels are given
INVALID_ARGUMENT, INVALID_USAGE, TIMEOUT, SYSTEM_ERROR = 4, 5, 8, 2

_K = None
_STREAMS = []


def _kernels():
    """libdevapi_kernels.so, loaded after libnccl.so (its DT_NEEDED libnccl.so.2 is then the loaded one)."""
    global _K
    if _K is None:
        import nccl_amd
        nccl_amd.load()
        assert os.path.exists(KLIB), f"{KLIB} missing: make devapi-kernels"
        k = ctypes.CDLL(KLIB)
        P, S, I, U, U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64
        for name in ("lsa_allreduce_u32", "lsa_allreduce_f32", "lsa_alltoall"):
            getattr(k, name).argtypes = [P, P, S, P, S, S, I, P]
        k.barrier_rounds.argtypes = [P, U, U, I, P, I, I, I, P]
        k.resource_stamp.argtypes = [P, U, S, U, P, I, P]
        k.pointer_dump.argtypes = [P, P, S, U, P, P]
        k.timed_sync.argtypes = [P, I, U64, P, P]
        _K = k
    return _K


def _dedicated(n):
    """n streams with a hardware queue each, made once per process."""
    import nccl_amd
    while len(_STREAMS) < n:
        _STREAMS.append(nccl_amd.dedicated_stream(0))
    return _STREAMS[:n]


def _cs(n, env=None):
    """n in-process ranks on GPU 0, each with a dedicated stream."""
    cs = _comms(n, env)
    return [(c, s) for (c, _), s in zip(cs, _dedicated(n))]


def _grouped(cs, fn):
    """fn(comm, stream) for every rank of this process; collective host calls of several ranks go inside a group."""
    import nccl_amd
    if len(cs) == 1:
        return [fn(*cs[0])]
    with nccl_amd.group():
        return [fn(c, s) for c, s in cs]


def _layout_total(n, barriers, buffers):
    """ncclDevCommResourceLayout's totalBytes (include/nccl_device.h), restated."""
    up = lambda x, a: (x + a - 1) // a * a
    at = up(4 * barriers, 128) + up(4 * barriers * n, 128)
    for size, align in buffers:
        at = up(at, max(align, 128)) + size
    return up(max(at, 1), 4096)


class Rank:
    """One rank's windows and DevComm: send / recv buffers of `nbytes` (+ the offsets) registered as symmetric windows."""

    def __init__(self, comm, stream, nbytes):
        self.comm, self.stream = comm, stream
        self.send, self.recv = Buf(nbytes + 64), Buf(nbytes + 64)
        self.swin = self.rwin = self.dc = None


def _setup(cs, nbytes, barriers, buffers=()):
    torch = _torch()
    rs = [Rank(c, s, nbytes) for c, s in cs]
    by = {id(r.comm): r for r in rs}
    torch.cuda.synchronize()
    for w, b in (("swin", "send"), ("rwin", "recv")):
        wins = _grouped(cs, lambda c, s: c.register_window(getattr(by[id(c)], b).ptr, getattr(by[id(c)], b).nbytes))
        for r, win in zip(rs, wins):
            setattr(r, w, win)
    for r, dc in zip(rs, _grouped(cs, lambda c, s: c.dev_comm_create(barriers, buffers))):
        r.dc = dc
    return rs


def _teardown(rs, destroy_comms=True):
    for r in rs:
        r.stream.synchronize()
    for r in rs:
        r.comm.dev_comm_destroy(r.dc)
        r.comm.deregister_window(r.swin)
        r.comm.deregister_window(r.rwin)
    if destroy_comms:
        for r in rs:
            r.comm.destroy()


def _inputs(kind, count, n, seed):
    """Every rank's input (any process can compute all of them) and the expected result, folded in rank order."""
    xs = []
    for r in range(n):
        rng = np.random.default_rng(seed * 131 + r)
        if kind == "u32":
            xs.append(rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32))
        else:
            xs.append((rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4, count)).astype(np.float32))
    acc = xs[0].copy()
    for r in range(1, n):
        acc = (acc + xs[r]).astype(xs[0].dtype)     # uint32 wraps; fp32 rounds per add, in order 0..n-1
    return xs, acc


def _want_recv(nbytes_view, payload):
    want = np.full(nbytes_view, FILL, dtype=np.uint8)
    want[RECV_OFF:RECV_OFF + payload.nbytes] = payload.view(np.uint8)
    return want


def _fill(buf, off, arr):
    torch = _torch()
    raw = np.full(buf.nbytes, FILL, dtype=np.uint8)
    raw[off:off + arr.nbytes] = arr.view(np.uint8)
    buf.view.copy_(torch.from_numpy(raw))


def allreduce_case(rs, n, kind, count, grid, seed):
    """One LSA AllReduce on every rank of this process (ranks rs, of n in all). Returns error strings."""
    torch = _torch()
    k = _kernels()
    xs, want = _inputs(kind, count, n, seed)
    for r in rs:
        _fill(r.send, SEND_OFF, xs[r.comm.rank])
        r.recv.view.fill_(FILL)
    torch.cuda.synchronize()
    fn = k.lsa_allreduce_u32 if kind == "u32" else k.lsa_allreduce_f32
    for r in rs:
        rc = fn(r.dc.ptr, r.swin.handle, SEND_OFF, r.rwin.handle, RECV_OFF, count, grid, r.stream.cuda_stream)
        assert rc == 0, f"launch failed: hipError {rc}"
    errs = []
    what = f"allreduce {kind} n={n} count={count} grid={grid} seed={seed}"
    for r in rs:
        r.stream.synchronize()
        if r.comm.async_error():
            errs.append(f"rank {r.comm.rank} {what}: async error {r.comm.async_error()}")
            continue
        errs += r.recv.check(_want_recv(r.recv.nbytes, want), f"rank {r.comm.rank} {what}")
        sent = np.full(r.send.nbytes, FILL, dtype=np.uint8)
        sent[SEND_OFF:SEND_OFF + xs[r.comm.rank].nbytes] = xs[r.comm.rank].view(np.uint8)
        errs += r.send.check(sent, f"rank {r.comm.rank} send window {what}")
    return errs


def allreduce_matrix(cs, n):
    """Counts x grids x {u32, f32}, each case run twice on the same DevComm (the barrier epochs carry over)."""
    rs = _setup(cs, 4 * max(COUNTS), max(GRIDS))
    errs, seed = [], 0
    for kind in ("u32", "f32"):
        for count in COUNTS:
            for grid in GRIDS:
                for _ in range(2):
                    seed += 1
                    errs += allreduce_case(rs, n, kind, count, grid, seed)
                if errs:
                    break
    _teardown(rs, destroy_comms=False)
    return errs


def alltoall_cases(cs, n):
    torch = _torch()
    k = _kernels()
    errs = []
    sizes = (16, 4097)
    rs = _setup(cs, n * max(sizes), 4)
    for seed, bb in enumerate(sizes):
        data = [np.random.default_rng(7000 + seed * 17 + r).integers(0, 256, n * bb, dtype=np.uint8) for r in range(n)]
        for r in rs:
            _fill(r.send, SEND_OFF, data[r.comm.rank])
            r.recv.view.fill_(FILL)
        torch.cuda.synchronize()
        for r in rs:
            rc = k.lsa_alltoall(r.dc.ptr, r.swin.handle, SEND_OFF, r.rwin.handle, RECV_OFF, bb, 4, r.stream.cuda_stream)
            assert rc == 0
        for r in rs:
            r.stream.synchronize()
            me = r.comm.rank
            want = np.concatenate([data[p][me * bb:(me + 1) * bb] for p in range(n)])
            errs += r.recv.check(_want_recv(r.recv.nbytes, want), f"rank {me} alltoall n={n} block={bb}")
            if r.comm.async_error():
                errs.append(f"rank {me}: async error {r.comm.async_error()}")
    _teardown(rs, destroy_comms=False)
    return errs


def barrier_rounds_cases(cs, n, grid=4, rounds=200):
    """CTA and wave variants, with acq_rel syncs around plain slot accesses and with relaxed syncs (no fence) around
    system-scope atomic slot accesses, each launched twice on one DevComm; every rank's mismatch count must be 0."""
    torch = _torch()
    k = _kernels()
    errs = []
    for warp in (0, 1):
        units = grid * (4 if warp else 1)
        rs = _setup(cs, 64, units, [(4 * n * units, 128)])
        for relaxed in (0, 1):
            bad = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in rs]
            torch.cuda.synchronize()
            for launch in range(2):
                first = 1 + (2 * relaxed + launch) * rounds
                for r, b in zip(rs, bad):
                    rc = k.barrier_rounds(r.dc.ptr, r.dc.buffer_handles[0], first, rounds, b.data_ptr(), grid, warp,
                                          relaxed, r.stream.cuda_stream)
                    assert rc == 0
                for r in rs:
                    r.stream.synchronize()
            what = f"{'wave' if warp else 'cta'} barriers, {'relaxed' if relaxed else 'acq_rel'}"
            for r, b in zip(rs, bad):
                if int(b.item()) != 0:
                    errs.append(f"rank {r.comm.rank} n={n} {what}: {int(b.item())} stale slots")
                if r.comm.async_error():
                    errs.append(f"rank {r.comm.rank} {what}: async error {r.comm.async_error()}")
        _teardown(rs, destroy_comms=False)
    return errs


def pointer_cases(cs, n):
    """pointer_dump against the host getters for every peer at offsets {0, 16, size-1}; bounds of the host getters."""
    torch = _torch()
    import nccl_amd
    k = _kernels()
    lib = nccl_amd.load()
    errs = []
    rs = _setup(cs, 4096, 1, [(1000, 256)])

    def host(fn, win, off, p):
        out = ctypes.c_void_p()
        rc = fn(win, off, p, ctypes.byref(out))
        return rc, out.value

    for r in rs:
        me, size, h = r.comm.rank, r.send.nbytes, r.dc.buffer_handles[0]
        out = torch.zeros(5 * n + 3, dtype=torch.int64, device="cuda")
        for off in (0, 16, size - 1):
            torch.cuda.synchronize()
            assert k.pointer_dump(r.dc.ptr, r.swin.handle, off, h, out.data_ptr(), r.stream.cuda_stream) == 0
            r.stream.synchronize()
            got = [int(v) & (2 ** 64 - 1) for v in out.cpu().tolist()]
            lsa = [host(lib.ncclGetLsaDevicePointer, r.swin.handle, off, p) for p in range(n)]
            peer = [host(lib.ncclGetPeerDevicePointer, r.swin.handle, off, p) for p in range(n)]
            res = [host(lib.ncclGetLsaDevicePointer, r.dc.resource_window, h * 128, p) for p in range(n)]
            if any(rc for rc, _ in lsa + peer + res):
                errs.append(f"rank {me} off={off}: a host getter failed {lsa} {peer} {res}")
                continue
            want = ([v for _, v in lsa] + [v for _, v in peer] + [v for _, v in peer]
                    + [r.comm.window_user_ptr(r.swin) + off] + [v for _, v in res] + [res[me][1]]
                    + [v for _, v in res] + [h * 128])
            if got != want:
                errs.append(f"rank {me} off={off}: device {[hex(v) for v in got]} host {[hex(v) for v in want]}")
            if r.swin.lsa_pointer(off, me) != r.send.ptr + off:
                errs.append(f"rank {me} off={off}: the local pointer is not userPtr + offset")
        for fn in (lib.ncclGetLsaDevicePointer, lib.ncclGetPeerDevicePointer):
            if host(fn, r.swin.handle, size, 0)[0] != INVALID_ARGUMENT:
                errs.append(f"rank {me}: offset == size accepted")
            if host(fn, r.swin.handle, 0, n)[0] != INVALID_ARGUMENT or host(fn, r.swin.handle, 0, -1)[0] != INVALID_ARGUMENT:
                errs.append(f"rank {me}: peer out of range accepted")
        if h * 128 % 256:
            errs.append(f"rank {me}: buffer handle {h} is not 256-byte aligned")
    _teardown(rs, destroy_comms=False)
    return errs


def graph_cases(cs, n):
    """One captured lsa_allreduce_u32 launch, replayed 3 times with new inputs (n ranks, one per process)."""
    torch = _torch()
    k = _kernels()
    errs = []
    count, grid = 4097, 4
    rs = _setup(cs, 4 * count, grid)
    (r,) = rs
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    xs, want = _inputs("u32", count, n, 900)
    _fill(r.send, SEND_OFF, xs[r.comm.rank])
    r.recv.view.fill_(FILL)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        rc = k.lsa_allreduce_u32(r.dc.ptr, r.swin.handle, SEND_OFF, r.rwin.handle, RECV_OFF, count, grid,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for rep in range(3):
        xs, want = _inputs("u32", count, n, 901 + rep)
        _fill(r.send, SEND_OFF, xs[r.comm.rank])
        r.recv.view.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        errs += r.recv.check(_want_recv(r.recv.nbytes, want), f"rank {r.comm.rank} graph replay {rep}")
    if r.comm.async_error():
        errs.append(f"rank {r.comm.rank}: async error {r.comm.async_error()}")
    del g
    _teardown(rs, destroy_comms=False)
    return errs


# ---------------------------------------------------------------- spawned ranks (one process each)
# tests/test_gpu_broadcast.py's _spawn runs ONE worker process that looks its job up in that module's own JOBS table
# (for cases that read the kernel or debug log). Here every rank is a process of its own, sharing a unique id, as in
# that file's test_multi_process; the jobs of one rank count run in one set of processes, started once per session.

RANK_JOBS = {"allreduce": allreduce_matrix, "alltoall": alltoall_cases, "barrier_rounds": barrier_rounds_cases,
             "pointers": pointer_cases, "graph": graph_cases}


def _rank_main(rank, nranks, uid, jobs, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(nranks, rank, uid)
        cs = [(comm, torch.cuda.Stream())]
        out = {}
        for job in jobs:
            out[job] = RANK_JOBS[job](cs, nranks)
            torch.cuda.synchronize()
        comm.destroy()
        q.put((rank, out))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, {job: [f"rank {rank} exception {e!r}\n{traceback.format_exc()}"] for job in jobs}))


_SPAWNED = {}


def _spawned(nranks, jobs):
    """Run `jobs` on nranks spawned processes, once per session; {job: error strings of every rank}."""
    key = (nranks, tuple(jobs))
    if key in _SPAWNED:
        return _SPAWNED[key]
    _torch()
    import nccl_amd
    uid = nccl_amd.get_unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rank_main, args=(r, nranks, uid, jobs, q)) for r in range(nranks)]
    for p in ps:
        p.start()
    results = {}
    try:
        while len(results) < nranks:
            r, out = q.get(timeout=240)
            results[r] = out
    except queue.Empty:
        pass
    for p in ps:
        if p.is_alive() and len(results) < nranks:
            p.kill()
        p.join(timeout=60)
    assert len(results) == nranks, f"only {len(results)} of {nranks} ranks reported"
    _SPAWNED[key] = {job: [e for r in sorted(results) for e in results[r][job]] for job in jobs}
    return _SPAWNED[key]


N2_JOBS = ("pointers", "allreduce", "graph")
N8_JOBS = ("allreduce", "barrier_rounds")


# ---------------------------------------------------------------- 1. properties and lifecycle

def test_properties_and_lifecycle(built):
    import nccl_amd
    lib = nccl_amd.load()
    cs = _cs(2)
    for c, _ in cs:
        p = c.query_properties()
        assert (p.rank, p.nRanks, p.cudaDev, p.nvmlDev) == (c.rank, 2, 0, -1)
        assert p.deviceApiSupport and not p.multimemSupport and p.hostRmaSupport
        assert (p.ginType, p.railedGinType, p.nLsaTeams) == (0, 0, 1)
    base = [c.mem_stats() for c, _ in cs]
    bufs = [(1000, 256)]
    first = _grouped(cs, lambda c, s: c.dev_comm_create(4, bufs))      # created inside a group
    total = _layout_total(2, 4, bufs)
    assert [c.mem_stats() for c, _ in cs] == [b + total for b in base]
    for (c, _), d in zip(cs, first):
        assert (d.struct.rank, d.struct.nRanks, d.struct.lsaRank, d.struct.lsaSize) == (c.rank, 2, c.rank, 2)
        assert d.struct.lsaBarrierCount == 4 and d.buffer_handles[0] * 128 % 256 == 0
    second = _grouped(cs, lambda c, s: c.dev_comm_create(64, ()))       # two DevComms alive at once
    total2 = _layout_total(2, 64, ())
    assert [c.mem_stats() for c, _ in cs] == [b + total + total2 for b in base]
    assert all(a.resource_window != b.resource_window for a, b in zip(first, second))

    # requirements without a counterpart here: ncclInvalidUsage, checked before anything collective happens
    refused = dict(lsaMultimem=True, ginConnectionType=1, ginForceEnable=True, barrierCount=1, railGinBarrierCount=1,
                   worldGinBarrierCount=1, lsaLLA2ABlockCount=1, lsaLLA2ASlotCount=1, ginSignalCount=1,
                   ginCounterCount=1, teamRequirementsList=0x1000)
    for c, _ in cs:
        for field, value in refused.items():
            q = nccl_amd.DevCommRequirements.default(lsaBarrierCount=1, **{field: value})
            dc = nccl_amd.DevCommStruct()
            assert lib.ncclDevCommCreate(c.ptr, ctypes.byref(q), ctypes.byref(dc)) == INVALID_USAGE, field
            assert field.split("[")[0] in lib.ncclGetLastError(None).decode(), field
        for counts in ((1, 0), (0, 1)):   # gin counts in a resource list entry
            res = nccl_amd.DevResourceRequirements(bufferSize=64, bufferAlign=64, ginSignalCount=counts[0],
                                                   ginCounterCount=counts[1])
            q = nccl_amd.DevCommRequirements.default(resourceRequirementsList=ctypes.pointer(res))
            dc = nccl_amd.DevCommStruct()
            assert lib.ncclDevCommCreate(c.ptr, ctypes.byref(q), ctypes.byref(dc)) == INVALID_USAGE
        q = nccl_amd.DevCommRequirements.default(lsaBarrierCount=nccl_amd.DEV_MAX_LSA_BARRIERS + 1)
        dc = nccl_amd.DevCommStruct()
        assert lib.ncclDevCommCreate(c.ptr, ctypes.byref(q), ctypes.byref(dc)) == INVALID_ARGUMENT
    # caller structs with a bad magic or size, on a live communicator: ncclInvalidArgument, nothing created
    for c, _ in cs:
        for field, value in (("magic", 0), ("magic", 0x1234), ("size", 8), ("size", 0)):
            p = nccl_amd.CommProperties.default()
            p.rank = -7
            setattr(p, field, value)
            assert lib.ncclCommQueryProperties(c.ptr, ctypes.byref(p)) == INVALID_ARGUMENT, (field, value)
            assert p.rank == -7                     # not filled in
            q = nccl_amd.DevCommRequirements.default(lsaBarrierCount=1)
            setattr(q, field, value)
            dc = nccl_amd.DevCommStruct()
            assert lib.ncclDevCommCreate(c.ptr, ctypes.byref(q), ctypes.byref(dc)) == INVALID_ARGUMENT, (field, value)
            assert dc.magic == 0
        assert lib.ncclCommQueryProperties(c.ptr, None) == INVALID_ARGUMENT
        q = nccl_amd.DevCommRequirements.default(lsaBarrierCount=1)
        assert lib.ncclDevCommCreate(c.ptr, None, ctypes.byref(nccl_amd.DevCommStruct())) == INVALID_ARGUMENT
        assert lib.ncclDevCommCreate(c.ptr, ctypes.byref(q), None) == INVALID_ARGUMENT
        # a DevComm struct that ncclDevCommCreate did not make (magic 0), and a live one with its magic wiped
        assert lib.ncclDevCommDestroy(c.ptr, ctypes.byref(nccl_amd.DevCommStruct())) == INVALID_ARGUMENT
        assert lib.ncclDevCommDestroy(c.ptr, None) == INVALID_ARGUMENT
        wiped = nccl_amd.DevCommStruct.from_buffer_copy(first[c.rank].struct)
        wiped.magic = 0
        assert lib.ncclDevCommDestroy(c.ptr, ctypes.byref(wiped)) == INVALID_ARGUMENT
    assert [c.mem_stats() for c, _ in cs] == [b + total + total2 for b in base]
    # ranks that disagree fail together and keep nothing
    made = []
    with pytest.raises(nccl_amd.NcclError) as ei:
        with nccl_amd.group():
            for c, _ in cs:
                made.append(c.dev_comm_create(2 + c.rank, ()))
    assert ei.value.code == INVALID_ARGUMENT
    assert all(d.struct.magic == 0 and d.resource_window == 0 for d in made)
    assert [c.mem_stats() for c, _ in cs] == [b + total + total2 for b in base]

    for (c, _), a, b in zip(cs, first, second):
        c.dev_comm_destroy(a)
        assert c.mem_stats() == base[c.rank] + total2
        c.dev_comm_destroy(b)
        assert c.mem_stats() == base[c.rank]
        assert lib.ncclDevCommDestroy(c.ptr, ctypes.byref(b.struct)) == INVALID_ARGUMENT   # destroyed already
    # a live DevComm goes with its communicator
    _grouped(cs, lambda c, s: c.dev_comm_create(1, ()))
    _destroy(cs)


def test_window_handle_failure_is_collective(built):
    """One rank of an in-process communicator cannot allocate its window handle (a test knob makes rank 1's fail): the
    registration fails on both ranks, neither keeps a window or a DevComm, and the next registration works."""
    import nccl_amd
    cs = _cs(2)
    bufs = [Buf(4096) for _ in cs]
    base = [c.mem_stats() for c, _ in cs]
    os.environ["NCCL_AMD_TEST_WIN_HANDLE_FAIL"] = "1"
    try:
        wins, dcs = [], []
        with pytest.raises(nccl_amd.NcclError):
            with nccl_amd.group():
                for (c, _), b in zip(cs, bufs):
                    wins.append(c.register_window(b.ptr, b.nbytes))
        assert [w.handle for w in wins] == [0, 0]
        with pytest.raises(nccl_amd.NcclError):
            with nccl_amd.group():
                for c, _ in cs:
                    dcs.append(c.dev_comm_create(2, ()))
        assert all(d.struct.magic == 0 for d in dcs)
        assert [c.mem_stats() for c, _ in cs] == base
    finally:
        del os.environ["NCCL_AMD_TEST_WIN_HANDLE_FAIL"]
    wins = _grouped(cs, lambda c, s: c.register_window(bufs[c.rank].ptr, bufs[c.rank].nbytes))
    assert all(w.handle for w in wins)
    for (c, _), w in zip(cs, wins):
        assert w.lsa_pointer(0, 1 - c.rank) == bufs[1 - c.rank].ptr
        c.deregister_window(w)
    _destroy(cs)


# ---------------------------------------------------------------- 2. pointers

def test_pointers_in_process(built):
    cs = _cs(3)
    errs = pointer_cases(cs, 3)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_pointers_spawned(built):
    errs = _spawned(2, N2_JOBS)["pointers"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 3. LSA AllReduce

@pytest.mark.parametrize("n", [2, 3, 4])
def test_lsa_allreduce_in_process(built, n):
    cs = _cs(n)
    errs = allreduce_matrix(cs, n)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("n", [2, 8])
def test_lsa_allreduce_spawned(built, n):
    errs = _spawned(n, N2_JOBS if n == 2 else N8_JOBS)["allreduce"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 4. store-based AlltoAll

def test_lsa_alltoall_in_process(built):
    cs = _cs(3)
    errs = alltoall_cases(cs, 3)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_lsa_alltoall_spawned(built):
    errs = _spawned(4, ("alltoall",))["alltoall"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 5. barrier rounds

@pytest.mark.parametrize("n", [2, 4])
def test_barrier_rounds_in_process(built, n):
    cs = _cs(n)
    errs = barrier_rounds_cases(cs, n)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_barrier_rounds_spawned(built):
    errs = _spawned(8, N8_JOBS)["barrier_rounds"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 6. resource buffers

def test_resource_buffers(built):
    torch = _torch()
    k = _kernels()
    n = 3
    cs = _cs(n)
    bufs = [(1000, 256), (65536, 4096)]
    rs = _setup(cs, 64, 4, bufs)
    bad = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in rs]
    torch.cuda.synchronize()
    for r in rs:
        hs = r.dc.buffer_handles
        assert hs[0] * 128 % 256 == 0 and hs[1] * 128 % 4096 == 0, hs
        assert hs[0] * 128 + 1000 <= hs[1] * 128 and hs[1] * 128 + 65536 <= _layout_total(n, 4, bufs)
    for seed in (1, 2):   # twice: the second round's stamps replace the first's
        for r, b in zip(rs, bad):
            for h, (size, _) in zip(r.dc.buffer_handles, bufs):
                assert k.resource_stamp(r.dc.ptr, h, size, seed, b.data_ptr(), 4, r.stream.cuda_stream) == 0
        for r in rs:
            r.stream.synchronize()
    assert [int(b.item()) for b in bad] == [0] * n
    assert [r.comm.async_error() for r in rs] == [0] * n
    _teardown(rs)


# ---------------------------------------------------------------- 7. interop with the library's own operations

def test_interop_with_collectives_and_puts(built):
    """On one stream per rank: ncclAllReduce on the symmetric windows, the LSA kernel, ncclPutSignal / ncclWaitSignal,
    the LSA kernel again."""
    torch = _torch()
    import nccl_amd
    n, count = 2, 4097
    cs = _cs(n)
    rs = _setup(cs, 4 * count, 4)
    xs, want = _inputs("u32", count, n, 501)
    for r in rs:
        _fill(r.send, SEND_OFF, xs[r.comm.rank])
        r.recv.view.fill_(FILL)
    torch.cuda.synchronize()
    with nccl_amd.group():
        for r in rs:
            r.comm.all_reduce_raw(r.send.ptr + SEND_OFF, r.recv.ptr + RECV_OFF, count, 3, 0, r.stream.cuda_stream)
    errs = []
    for r in rs:
        r.stream.synchronize()
        errs += r.recv.check(_want_recv(r.recv.nbytes, want), f"rank {r.comm.rank} ncclAllReduce")
    errs += allreduce_case(rs, n, "u32", count, 4, 502)
    # each rank puts its first 1024 bytes behind the peer's payload offset, and waits for the peer's put
    for r in rs:
        r.recv.view.fill_(FILL)
    torch.cuda.synchronize()
    with nccl_amd.group():
        for r in rs:
            r.comm.put_signal_raw(r.send.ptr + SEND_OFF, 1024, 1, 1 - r.comm.rank, r.rwin, RECV_OFF, r.stream.cuda_stream)
            r.comm.wait_signal([(1 - r.comm.rank, 1)], stream=r.stream)
    xs2, _ = _inputs("u32", count, n, 502)
    for r in rs:
        r.stream.synchronize()
        put = xs2[1 - r.comm.rank].view(np.uint8)[:1024]
        errs += r.recv.check(_want_recv(r.recv.nbytes, put), f"rank {r.comm.rank} ncclPutSignal")
    errs += allreduce_case(rs, n, "f32", count, 1, 503)
    assert [r.comm.async_error() for r in rs] == [0] * n
    _teardown(rs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 8. child communicators

def test_child_communicators(built):
    import nccl_amd
    cs = _cs(4)
    with nccl_amd.group():
        kids = [c.split(c.rank // 2, c.rank) for c, _ in cs]
    errs = []
    pairs = [[(kids[0], cs[0][1]), (kids[1], cs[1][1])], [(kids[2], cs[2][1]), (kids[3], cs[3][1])]]
    for pair in pairs:
        assert [k.nranks for k, _ in pair] == [2, 2] and [k.rank for k, _ in pair] == [0, 1]
    # both children's DevComms are created in one group; then an AllReduce inside each pair
    flat = pairs[0] + pairs[1]
    rs = _setup(flat, 4 * 4097, 4)
    for i, grp in enumerate((rs[:2], rs[2:])):
        for kind in ("u32", "f32"):
            errs += allreduce_case(grp, 2, kind, 4097, 4, 600 + 10 * i + len(kind))
    _teardown(rs)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 9. graph replay

def test_graph_replay_spawned(built):
    errs = _spawned(2, N2_JOBS)["graph"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 10. bounded waits

def test_timed_sync_times_out(built):
    """Only rank 0 syncs, with 20 ms of 100 MHz ticks: ncclTimeout in its output word, nothing recorded."""
    torch = _torch()
    k = _kernels()
    cs = _cs(2)
    dcs = _grouped(cs, lambda c, s: c.dev_comm_create(1, ()))
    out = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert k.timed_sync(dcs[0].ptr, 1, 2_000_000, out.data_ptr(), cs[0][1].cuda_stream) == 0
    cs[0][1].synchronize()
    assert int(out.item()) == TIMEOUT
    assert [c.async_error() for c, _ in cs] == [0, 0]
    _destroy(cs)


def test_untimed_sync_gives_up_like_the_library(built):
    """NCCL_AMD_SPIN_TIMEOUT_MS=200 on a fresh communicator, only rank 0 syncs: the kernel ends and the communicator
    reports what the library's own timed-out kernels report (tests/test_gpu_api.py::test_spin_timeout_reports_async_error)."""
    torch = _torch()
    import nccl_amd
    k = _kernels()
    cs = _cs(2, {"NCCL_AMD_SPIN_TIMEOUT_MS": "200"})
    dcs = _grouped(cs, lambda c, s: c.dev_comm_create(1, ()))
    out = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert k.timed_sync(dcs[0].ptr, 0, 0, out.data_ptr(), cs[0][1].cuda_stream) == 0
    cs[0][1].synchronize()
    assert int(out.item()) == 0          # the kernel ran to its end
    assert cs[0][0].async_error() == SYSTEM_ERROR
    x = torch.ones(16, device="cuda")
    with pytest.raises(nccl_amd.NcclError):
        cs[0][0].allreduce(x, x, nccl_amd.SUM, stream=cs[0][1])
    for c, _ in cs:
        c.abort()


# ---------------------------------------------------------------- 11. the native example

@pytest.mark.parametrize("n", [2, 4])
def test_native_example(built, n):
    exe = os.path.join(ROOT, "tests", "native", "devapi_example")
    assert os.path.exists(exe), f"{exe} missing: make devapi-example"
    env = dict(os.environ, NCCL_AMD_SPIN_TIMEOUT_MS="30000")
    r = subprocess.run([exe, str(n)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and f"OK n={n}" in r.stdout, r.stdout + r.stderr
