"""GPU tests of ncclBroadcast / ncclBcast: the expected output is the root's bytes on every rank, compared bit for bit.

Ranks share the box's one GPU (ncclCommInitAll with a repeated device, NCCL_MULTI_RANK_GPU_ENABLE=1) or run as
spawned processes. Cases that read the kernel log (NCCL_AMD_KERNEL_LOG is read when the library loads) or the debug
log run in a spawned worker, like tests/test_gpu_ref_tuner.py. Every buffer carries guard bytes in front and behind,
checked unchanged."""
import multiprocessing as mp
import os
import queue

import numpy as np

import pytest

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")

GUARD, FILL = 64, 0x5A
TYPE_SIZE = {0: 1, 1: 1, 2: 4, 4: 8, 6: 2, 7: 4}   # int8, uint8, int32, int64, fp16, fp32
BCAST_KERNEL = "collKernel<unsigned char, 0, 6>"   # COLL_BCAST in the byte-typed unit
GARBAGE_PTR = 0xDEAD0000


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch


def _payload(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


class Buf:
    """nbytes at byte offset GUARD + mis of a storage that is FILL everywhere else (`data`, if given, in the view)."""

    def __init__(self, nbytes, mis=0, data=None, pinned=False):
        import torch
        total = GUARD + mis + nbytes + GUARD
        if pinned:
            self.store = torch.full((total,), FILL, dtype=torch.uint8).pin_memory()
        else:
            self.store = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        self.lo, self.nbytes = GUARD + mis, nbytes
        self.view = self.store[self.lo: self.lo + nbytes]
        self.ptr = self.store.data_ptr() + self.lo   # (an empty view has no data_ptr of its own)
        if data is not None:
            self.view.copy_(torch.from_numpy(data))

    def check(self, want, what):
        """The view holds `want` bit for bit and the guard bytes around it are untouched."""
        from tests import gpu_cases as G
        errs = []
        raw = self.store.cpu().numpy()
        got = raw[self.lo: self.lo + self.nbytes]
        if not G.same_bits(got, want, 1):
            bad = np.nonzero(got != want)[0]
            errs.append(f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[:5].tolist()} got "
                        f"{got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}")
        if not (np.all(raw[:self.lo] == FILL) and np.all(raw[self.lo + self.nbytes:] == FILL)):
            errs.append(f"{what}: bytes outside the buffer were written")
        return errs


def bcast_case(cs, nbytes, dtype, root, mode="oop", mis=0, seed=0, pinned_root=False, off_root_send=None):
    """One Broadcast of nbytes (as count = nbytes / sizeof(dtype) elements) on every (comm, stream) of this process.
    mode: "oop" (the root's sendbuff != recvbuff), "inplace" (the root's sendbuff == recvbuff through ncclBroadcast),
    "bcast" (ncclBcast on every rank). Off the root sendbuff is `off_root_send` (None: a null pointer).
    mis: byte misalignment of every buffer, or one per rank. Returns error strings."""
    import torch
    import nccl_amd
    ts = TYPE_SIZE[dtype]
    assert nbytes % ts == 0
    want = _payload(nbytes, seed)
    plan = []
    for comm, stream in cs:
        r = comm.rank
        m = mis[r % len(mis)] if isinstance(mis, (list, tuple)) else mis
        is_root = r == root
        pin = pinned_root and is_root
        if mode == "oop" and is_root:
            sb, rb = Buf(nbytes, m, want, pin), Buf(nbytes, m, None, pin)
            plan.append((comm, stream, sb.ptr, rb, sb))
        elif is_root:
            rb = Buf(nbytes, m, want, pin)
            plan.append((comm, stream, rb.ptr, rb, None))
        else:
            plan.append((comm, stream, off_root_send, Buf(nbytes, m), None))
    torch.cuda.synchronize()
    lib = nccl_amd.load()
    with nccl_amd.group():
        for comm, stream, sp, rb, _ in plan:
            if mode == "bcast":
                rc = lib.ncclBcast(rb.ptr, nbytes // ts, dtype, root, comm.ptr, stream.cuda_stream)
                assert rc == 0, f"ncclBcast returned {rc}"
            else:
                comm.broadcast_raw(sp, rb.ptr, nbytes // ts, dtype, root, stream.cuda_stream)
    errs = []
    what = f"n={len(cs)} bytes={nbytes} dt={dtype} root={root} {mode} mis={mis}"
    for comm, stream, _, rb, sb in plan:
        stream.synchronize()
        if comm.async_error():
            errs.append(f"rank {comm.rank} {what}: async error {comm.async_error()}")
            continue
        errs += rb.check(want, f"rank {comm.rank} {what}")
        if sb is not None:  # the root's input is untouched
            errs += sb.check(want, f"root sendbuff {what}")
    return errs


def _comms(n, env=None):
    """n ranks on GPU 0 in this process, created under `env` (the knobs are read at communicator init)."""
    torch = _torch()
    import nccl_amd
    env = dict(env or {})
    env["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        torch.cuda.set_device(0)
        comms = nccl_amd.Communicator.init_all([0] * n)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return list(zip(comms, [torch.cuda.Stream() for _ in range(n)]))


def _destroy(cs):
    for c, _ in cs:
        c.destroy()


# ---------------------------------------------------------------- spawned workers (kernel log / debug log)

def _worker_main(job, env, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
        os.environ.update(env)
        klog = f"/tmp/nccl_amd_bcast_kernels_{os.getpid()}.log"
        dlog = f"/tmp/nccl_amd_bcast_debug_{os.getpid()}.log"
        for f in (klog, dlog):
            if os.path.exists(f):
                os.remove(f)
        os.environ["NCCL_AMD_KERNEL_LOG"] = klog
        if "NCCL_DEBUG" in env:
            os.environ["NCCL_DEBUG_FILE"] = dlog
        import torch
        torch.cuda.set_device(0)
        errs = JOBS[job]()
        torch.cuda.synchronize()
        out = (errs, open(klog).read().splitlines() if os.path.exists(klog) else [],
               open(dlog).read() if os.path.exists(dlog) else "")
        for f in (klog, dlog):
            if os.path.exists(f):
                os.remove(f)
        q.put(out)
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put(([f"exception {e!r}\n{traceback.format_exc()}"], [], ""))


def _spawn(job, env):
    _torch()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_main, args=(job, env, q))
    p.start()
    try:
        out = q.get(timeout=240)
    except queue.Empty:
        p.kill()
        raise AssertionError(f"worker {job} did not report")
    p.join(timeout=60)
    return out


def _job_small():
    errs = []
    for n in (2, 3, 5):
        cs = _comms(n)
        seed = 0
        for root in range(n):
            for nbytes in (1, 5, 8, 9, 56, 57, 4099):
                for dtype in (1, 6, 7, 4):
                    if nbytes % TYPE_SIZE[dtype]:
                        continue
                    seed += 1
                    errs += bcast_case(cs, nbytes, dtype, root, "oop", seed=seed)
                    errs += bcast_case(cs, nbytes, dtype, root, "bcast", seed=seed + 5000)
            if errs:
                break
        _destroy(cs)
    return errs


DIRECT_ENV = {"NCCL_PROTO": "Simple", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2", "NCCL_MAX_CTAS": "7"}


def _job_direct():
    errs = []
    for n in (2, 3, 4):
        cs = _comms(n)
        seed = 100 * n
        for root in range(n):
            for nbytes, dtype in ((5, 1), (16 * n + 1, 1), (70_001, 1), (300_001 * 4, 7), (((1 << 20) + 16) * 4, 7)):
                seed += 1
                errs += bcast_case(cs, nbytes, dtype, root, "oop", seed=seed)
            # in place at the root, misaligned bases (1, 3, and one offset per rank as test_rank_dependent_misalignment)
            errs += bcast_case(cs, 70_001, 1, root, "inplace", seed=seed + 1)
            errs += bcast_case(cs, 300_001 * 4, 7, root, "inplace", seed=seed + 2)
            errs += bcast_case(cs, 16 * n + 1, 1, root, "oop", mis=1, seed=seed + 3)
            errs += bcast_case(cs, 70_001, 1, root, "oop", mis=3, seed=seed + 4)
            errs += bcast_case(cs, 300_001 * 4, 7, root, "bcast", mis=1, seed=seed + 5)
            for mis in ([0, 1, 3], [3, 0, 1], [1, 1, 0]):
                errs += bcast_case(cs, 70_001, 1, root, "oop", mis=mis, seed=seed + 6)
                errs += bcast_case(cs, 300_001 * 4, 7, root, "inplace", mis=mis, seed=seed + 7)
            if errs:
                break
        errs += bcast_case(cs, 300_001 * 4, 7, n - 1, "oop", seed=seed + 8, pinned_root=True)
        _destroy(cs)
    return errs


def _job_group():
    """One group: four Broadcasts (roots 0..2, four types, two on LL and two direct) beside an AllReduce."""
    import torch
    import nccl_amd
    import oracle
    n = 3
    cs = _comms(n)
    ops = [(1000, 1, 2), (64 * 7, 4, 0), (300_001 * 4, 7, 1), (200_002, 6, 2)]  # (bytes, dtype, root)
    wants = [_payload(b, 900 + k) for k, (b, _, _) in enumerate(ops)]
    count = 50_001
    ins = [oracle.fill(7, 77 + r, count) for r in range(n)]
    bufs = {}
    for comm, _ in cs:
        r = comm.rank
        per = []
        for k, (b, dt, root) in enumerate(ops):
            per.append((Buf(b, 0, wants[k]) if r == root else None, Buf(b)))
        bufs[r] = (per, torch.from_numpy(ins[r]).cuda(), torch.zeros(count, device="cuda"))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for comm, stream in cs:
            per, x, y = bufs[comm.rank]
            for (send, recv), (b, dt, root) in zip(per, ops):
                comm.broadcast_raw(send.ptr if send is not None else None, recv.ptr, b // TYPE_SIZE[dt], dt, root,
                                   stream.cuda_stream)
            comm.allreduce(x, y, nccl_amd.SUM, stream=stream)
    errs = []
    want_ar = oracle.all_reduce(ins, 7, 0)
    for comm, stream in cs:
        stream.synchronize()
        if comm.async_error():
            errs.append(f"rank {comm.rank}: async error {comm.async_error()}")
            continue
        per, _, y = bufs[comm.rank]
        for k, (_, recv) in enumerate(per):
            errs += recv.check(wants[k], f"group op {k} rank {comm.rank}")
        if not np.array_equal(y.cpu().numpy(), want_ar):
            errs.append(f"group AllReduce rank {comm.rank} differs")
    _destroy(cs)
    return errs


def _job_registered():
    """Buffers registered with ncclCommRegister, then inside symmetric windows: Broadcast keeps the staged kernel."""
    import torch
    import nccl_amd
    n, nbytes = 2, 300_000
    cs = _comms(n)
    errs = []
    for how in ("register", "window"):
        want = _payload(nbytes, 31 if how == "register" else 32)
        allocs = [torch.full((8 << 20,), FILL, dtype=torch.uint8, device="cuda") for _ in cs]
        if how == "register":
            hs = [c.register_buffer(a.data_ptr(), a.numel()) for (c, _), a in zip(cs, allocs)]
        else:
            with nccl_amd.group():
                hs = [c.register_window(a.data_ptr(), a.numel()) for (c, _), a in zip(cs, allocs)]
        root = 1
        send = [a[4096:4096 + nbytes] for a in allocs]
        recv = [a[524288:524288 + nbytes] for a in allocs]
        send[root].copy_(torch.from_numpy(want))
        torch.cuda.synchronize()
        with nccl_amd.group():
            for (c, s), sv, rv in zip(cs, send, recv):
                c.broadcast_raw(sv.data_ptr(), rv.data_ptr(), nbytes, 1, root, s.cuda_stream)
        for (c, s), a, rv in zip(cs, allocs, recv):
            s.synchronize()
            if c.async_error():
                errs.append(f"{how} rank {c.rank}: async error {c.async_error()}")
            elif not np.array_equal(rv.cpu().numpy(), want):
                errs.append(f"{how} rank {c.rank}: output differs")
            elif not bool((a[524288 + nbytes:] == FILL).all()):
                errs.append(f"{how} rank {c.rank}: bytes behind the output were written")
        for (c, _), h in zip(cs, hs):
            c.deregister_buffer(h) if how == "register" else c.deregister_window(h)
    _destroy(cs)
    return errs


def _job_tuner():
    cs = _comms(2)
    errs = bcast_case(cs, 1 << 20, 7, 1, "oop", seed=5)
    _destroy(cs)
    return errs


JOBS = {"small": _job_small, "direct": _job_direct, "group": _job_group, "registered": _job_registered,
        "tuner": _job_tuner}


# ---------------------------------------------------------------- tests

def test_one_rank(built):
    """n = 1: the copy kernel out of place, nothing in place; counts 0, 1 and 70_001 on fp32 and uint8; a pinned case."""
    cs = _comms(1)
    errs = []
    for dtype in (7, 1):
        for count in (0, 1, 70_001):
            for mode in ("oop", "inplace", "bcast"):
                errs += bcast_case(cs, count * TYPE_SIZE[dtype], dtype, 0, mode, seed=count + dtype)
    errs += bcast_case(cs, 70_001, 1, 0, "oop", seed=3, pinned_root=True)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("env", [{}, {"NCCL_AMD_LL128": "1", "NCCL_AMD_LL_BYTES": "1024"}], ids=["default", "ll128"])
def test_small_sizes_run_ll(built, env):
    """n in {2, 3, 5}, every root, 1 .. 4099 bytes in four types, out of place and ncclBcast, non-root sendbuff null:
    all on the LL kernel — with NCCL_AMD_LL128=1 and the LL range ended at 1 KiB, 4099 bytes on LL64 lines."""
    errs, kernels, _ = _spawn("small", env)
    assert not errs, "\n".join(errs[:20])
    assert any("::llKernel<unsigned char, 0, 1, 0>" in k for k in kernels), kernels
    assert not any(BCAST_KERNEL in k for k in kernels), kernels
    assert any("::llKernel<unsigned char, 0, 1, 1>" in k for k in kernels) == bool(env), kernels


def test_ll_parity_run_ahead(built):
    """LL Broadcasts back to back with no host synchronisation, roots rotating, sizes alternating 8 bytes and ~2 KiB:
    the token lines keep the parity double-buffering safe. Then the same interleaved with LL AllReduces and Reduces."""
    import torch
    import nccl_amd
    import oracle
    n = 3
    cs = _comms(n)
    errs = []
    for interleave in (False, True):
        ops = []  # (kind, per-rank buffers, want)
        for i in range(10):
            nbytes = 8 if i % 2 == 0 else 2040 + i
            want = _payload(nbytes, 300 + i + 50 * interleave)
            root = i % n
            per = {r: (Buf(nbytes, 0, want) if r == root else None, Buf(nbytes)) for r in range(n)}
            ops.append(("bcast", per, want, root, nbytes))
            if interleave:
                count = 64 + i
                ins = [oracle.fill(7, 400 + i * n + r, count) for r in range(n)]
                per = {r: (torch.from_numpy(ins[r]).cuda(), torch.zeros(count, device="cuda")) for r in range(n)}
                kind = "allreduce" if i % 2 == 0 else "reduce"
                want = oracle.all_reduce(ins, 7, 0) if kind == "allreduce" else oracle.reduce(ins, 7, 0, (i + 1) % n)
                ops.append((kind, per, want, (i + 1) % n, count))
        torch.cuda.synchronize()
        for kind, per, want, root, size in ops:
            with nccl_amd.group():
                for comm, stream in cs:
                    b = per[comm.rank]
                    if kind == "bcast":
                        comm.broadcast_raw(b[0].ptr if b[0] is not None else None, b[1].ptr, size, 1, root,
                                           stream.cuda_stream)
                    elif kind == "allreduce":
                        comm.allreduce(b[0], b[1], nccl_amd.SUM, stream=stream)
                    else:
                        comm.reduce(b[0], b[1], nccl_amd.SUM, root=root, stream=stream)
        for comm, stream in cs:
            stream.synchronize()
            if comm.async_error():
                errs.append(f"rank {comm.rank}: async error {comm.async_error()}")
        for k, (kind, per, want, root, size) in enumerate(ops):
            for r in range(n):
                if kind == "bcast":
                    errs += per[r][1].check(want, f"interleave={interleave} op {k} rank {r}")
                elif kind == "allreduce" or r == root:
                    if not np.array_equal(per[r][1].cpu().numpy(), want):
                        errs.append(f"interleave={interleave} op {k} {kind} rank {r} differs")
        if errs:
            break
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_direct_scatter_gather(built):
    """The staged kernel with 4 KiB slots, 2 slots, 7 channels (many steps, slot reuse): n in {2, 3, 4}, every root, 5
    bytes (blocks 1 .. n-1 empty) to 4 MiB + 64, out of place, in place at the root, misaligned and rank-dependent
    bases, a pinned-host root."""
    errs, kernels, _ = _spawn("direct", DIRECT_ENV)
    assert not errs, "\n".join(errs[:20])
    assert any(BCAST_KERNEL in k for k in kernels), kernels
    assert not any("::llKernel" in k for k in kernels), kernels


CREDIT_ENVS = [{"NCCL_AMD_AG_PULL": "1"}, {"NCCL_AMD_RS_PULL": "1", "NCCL_AMD_AG_PULL": "1"},
               {"NCCL_AMD_AG_PULL": "1", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2"},
               {"NCCL_AMD_AG_PULL": "0", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2"},
               {"NCCL_AMD_RS_PULL": "1", "NCCL_AMD_AG_PULL": "0"}]


@pytest.mark.parametrize("env", CREDIT_ENVS,
                         ids=["ag_pull", "both_pulls", "ag_pull_tiny_slots", "push_tiny_slots", "rs_pull_push"])
def test_credit_sequences_survive(built, env):
    """Broadcasts of every root between the other collectives on one communicator, under both gathers and both
    scatters: every collective finds its slots and counters where it expects them (the others against the oracle)."""
    from tests import gpu_cases as G
    cs = _comms(3, env)
    b = lambda root, nbytes: ("broadcast", nbytes, root)  # noqa: E731
    seq = [b(2, 100_003), ("allgather", 7, 0, 70_001, 0), b(0, 300_001 * 4), ("allreduce", 7, 0, 300_001, 0),
           ("reduce", 7, 0, 100_003, 1), b(1, 70_001), ("reducescatter", 7, 0, 3 * 40_000, 0), b(2, 1 << 20),
           ("allreduce", 6, 2, 1_000_003, 0), ("allgather", 2, 0, 5, 0)]
    errs = []
    for rep in range(2):
        for i, op in enumerate(seq):
            if op[0] == "broadcast":
                errs += bcast_case(cs, op[1], 1, op[2], "oop" if rep == 0 else "inplace", seed=2000 * rep + i)
            else:
                coll, dt, rop, count, root = op
                errs += G.run_case(cs, coll, dt, rop, count, 0, seed=1000 * rep + i, root=root)
            if errs:
                break
    _destroy(cs)
    assert not errs, "\n".join(errs[:10])


def test_group_batches(built):
    """Four Broadcasts of one group — different roots, types and sizes — form one LL batch and one staged batch."""
    errs, kernels, log = _spawn("group", {"NCCL_DEBUG": "TRACE"})
    assert not errs, "\n".join(errs[:20])
    ll = [ln for ln in log.splitlines() if "LL batch:" in ln]
    staged = [ln for ln in log.splitlines() if "staged batch:" in ln]
    # one line of each per rank (three ranks in the worker), each naming Broadcast and holding two ops
    assert len(ll) == 3 and all("2 ops (first Broadcast)" in ln for ln in ll), ll
    assert len(staged) == 3 and all("2 Broadcast ops" in ln for ln in staged), staged
    assert any("collBatchKernel<unsigned char, 0, 6>" in k for k in kernels), kernels


def test_graph_capture(built):
    """A direct and an LL Broadcast captured per rank, replayed three times with new root contents."""
    import torch
    import nccl_amd
    cs = _comms(2)
    comms = [c for c, _ in cs]
    streams = [nccl_amd.dedicated_stream(0), nccl_amd.dedicated_stream(0)]
    big, small = 1 << 20, 1000
    x = [torch.zeros(big, dtype=torch.uint8, device="cuda") for _ in range(2)]
    y = [torch.zeros(big, dtype=torch.uint8, device="cuda") for _ in range(2)]
    z = [torch.zeros(small, dtype=torch.uint8, device="cuda") for _ in range(2)]
    graphs = [torch.cuda.CUDAGraph() for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(2):
        with torch.cuda.graph(graphs[r], stream=streams[r]):
            comms[r].broadcast_raw(x[r].data_ptr(), y[r].data_ptr(), big // 4, 7, 0, streams[r].cuda_stream)
            comms[r].bcast(z[r], root=1, stream=streams[r])
    errs = []
    for it in range(3):
        wb, ws = _payload(big, 600 + it), _payload(small, 700 + it)
        x[0].copy_(torch.from_numpy(wb))
        z[1].copy_(torch.from_numpy(ws))
        z[0].zero_()
        for r in range(2):
            y[r].zero_()
        torch.cuda.synchronize()
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        torch.cuda.synchronize()
        for r in range(2):
            if comms[r].async_error():
                errs.append(f"replay {it} rank {r}: async error {comms[r].async_error()}")
            elif not (np.array_equal(y[r].cpu().numpy(), wb) and np.array_equal(z[r].cpu().numpy(), ws)):
                errs.append(f"replay {it} rank {r} differs")
    del graphs
    _destroy(cs)
    assert not errs, "\n".join(errs)


def test_registered_buffers_stay_staged(built):
    errs, kernels, _ = _spawn("registered", {"NCCL_PROTO": "^LL"})
    assert not errs, "\n".join(errs[:20])
    assert any(BCAST_KERNEL in k for k in kernels), kernels
    assert not any("symKernel" in k for k in kernels), kernels


def _mp_worker(rank, nranks, uid, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(nranks, rank, uid)
        cs = [(comm, torch.cuda.Stream())]
        errs = []
        for i, (root, nbytes) in enumerate([(0, 1000), (3, 1000), (0, 300_001), (3, 300_001 * 4)]):
            errs += bcast_case(cs, nbytes, 1, root, "oop" if i % 2 == 0 else "bcast", seed=800 + i)
        comm.destroy()
        q.put((rank, errs))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, [f"rank {rank} exception: {e!r}"]))


def test_multi_process(built):
    """Four processes on one GPU, roots 0 and 3, an LL and a direct size; each process checks its own rank."""
    _torch()
    import nccl_amd
    nranks = 4
    uid = nccl_amd.get_unique_id()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_mp_worker, args=(r, nranks, uid, q)) for r in range(nranks)]
    for p in ps:
        p.start()
    results = {}
    try:
        while len(results) < nranks:
            r, errs = q.get(timeout=240)
            results[r] = errs
    except queue.Empty:
        pass
    for p in ps:
        if p.is_alive() and len(results) < nranks:
            p.kill()
        p.join(timeout=60)
    assert len(results) == nranks, f"only {len(results)} of {nranks} ranks reported"
    bad = [e for r in sorted(results) for e in results[r]]
    assert not bad, "\n".join(bad[:20])


def test_tuner_plugin_row(built, tmp_path):
    """The reference's example tuner with a broadcast row: the direct kernel on the plugin's 3 channels."""
    plugin = os.path.join(REF, "libnccl-tuner-example.so")
    if not os.path.exists(plugin):
        pytest.fail(f"{plugin} missing: build it with `make -C oracle ref` (needs /root/reference) before the GPU run")
    conf = tmp_path / "nccl_tuner.conf"
    conf.write_text("broadcast,0,4294967295,ring,simple,3,-1,-1\n")
    errs, kernels, _ = _spawn("tuner", {"NCCL_TUNER_PLUGIN": plugin, "NCCL_TUNER_CONFIG_FILE": str(conf)})
    assert not errs, "\n".join(errs[:20])
    assert any(BCAST_KERNEL in k and " grid=3 " in k for k in kernels), kernels


def test_arguments(built):
    """root outside 0 .. n-1 is ncclInvalidArgument and the communicator stays usable; with NCCL_CHECK_POINTERS=1 a
    garbage sendbuff passes off the root and fails on it."""
    import nccl_amd
    cs = _comms(2, {"NCCL_CHECK_POINTERS": "1"})
    (c0, s0), (c1, s1) = cs
    b = Buf(4096)
    for root in (2, -1):
        with pytest.raises(nccl_amd.NcclError) as ei:
            c0.broadcast_raw(b.ptr, b.ptr, 1024, 7, root, s0.cuda_stream)
        assert ei.value.code == nccl_amd.Result.InvalidArgument
    errs = bcast_case(cs, 4096, 7, 0, "oop", seed=1)                                   # still usable
    errs += bcast_case(cs, 300_001, 1, 1, "oop", seed=2, off_root_send=GARBAGE_PTR)    # garbage off the root: unread
    host = np.zeros(4096, dtype=np.uint8)                                              # unregistered host memory
    errs += bcast_case(cs, 4096, 1, 0, "oop", seed=3, off_root_send=host.ctypes.data)
    assert not errs, "\n".join(errs)
    with pytest.raises(nccl_amd.NcclError) as ei:                                      # the same pointer on the root
        c1.broadcast_raw(GARBAGE_PTR, b.ptr, 4096, 1, 1, s1.cuda_stream)
    assert ei.value.code == nccl_amd.Result.InvalidArgument
    errs = bcast_case(cs, 1000, 1, 1, "bcast", seed=4)
    _destroy(cs)
    assert not errs, "\n".join(errs)


def test_python_tensors(built):
    """Communicator.broadcast / bcast on torch tensors: a small Linear's parameters from rank 0 to rank 1."""
    import torch
    import nccl_amd
    cs = _comms(2)
    torch.manual_seed(11)
    models = [torch.nn.Linear(37, 19).cuda(), torch.nn.Linear(37, 19).cuda()]
    assert not torch.equal(models[0].weight, models[1].weight)
    ref = [p.detach().clone() for p in models[0].parameters()]
    out = torch.zeros(1000, dtype=torch.float16, device="cuda")
    src = torch.randn(1000, device="cuda").half()
    torch.cuda.synchronize()
    with torch.no_grad():
        for p0, p1 in zip(models[0].parameters(), models[1].parameters()):
            with nccl_amd.group():
                cs[0][0].bcast(p0.data, root=0, stream=cs[0][1])
                cs[1][0].bcast(p1.data, root=0, stream=cs[1][1])
        with nccl_amd.group():
            cs[0][0].broadcast(None, out, root=1, stream=cs[0][1])   # sendbuf=None off the root
            cs[1][0].broadcast(src, src, root=1, stream=cs[1][1])
    torch.cuda.synchronize()
    assert all(c.async_error() == 0 for c, _ in cs)
    for want, p0, p1 in zip(ref, models[0].parameters(), models[1].parameters()):
        assert torch.equal(p0, want) and torch.equal(p1, want)
    assert torch.equal(out, src)
    with pytest.raises(ValueError):
        cs[1][0].broadcast(None, out, root=1)   # the root needs a sendbuf
    _destroy(cs)
