"""GPU tests of the one-sided operations ncclPutSignal / ncclSignal / ncclWaitSignal: payloads are random bytes from a
seed, the expected window contents plain numpy slicing, compared bit for bit.

Ranks share the box's one GPU (ncclCommInitAll with a repeated device, NCCL_MULTI_RANK_GPU_ENABLE=1) or run as spawned
processes. Every rank owns a source buffer and a target buffer (tests/test_gpu_broadcast.py's Buf: guard bytes in front
and behind, checked unchanged), each registered as a window over exactly its view, so a put that ends at the window's
end ends at the guard bytes. Before a phase every target fills its window with a kernel and reads it back (stale lines
in its caches); after its wait it reads the window with a kernel on the same stream.

One thread drives all ranks of a process, so a phase either sits in one group (every rank's puts, then its wait) or is
issued in dependency order; the free order belongs to the multi-process test."""
import multiprocessing as mp
import os
import queue

import numpy as np

import pytest

from tests.test_gpu_broadcast import CREDIT_ENVS, FILL, TYPE_SIZE, Buf, _comms, _destroy, _payload, _torch, bcast_case
from tests.test_gpu_p2p import p2p_case, ring_shift

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu
BIG = (4 << 20) + 64
SIZES = (0, 1, 15, 16, 17, 4095, 4097, (64 << 10) + 1, BIG)
CHUNK_ENV = {"NCCL_AMD_P2P_CHUNK_BYTES": "4096"}
SYM, NONSYM = 1, 0


class Arenas:
    """Per rank of this process a source Buf and a target Buf, registered as windows over their views (collective:
    inside one group when one thread drives several ranks). tgt_bytes may be one size per rank."""

    def __init__(self, cs, src_bytes, tgt_bytes, tgt_flags=SYM):
        import nccl_amd
        self.cs = cs
        self.n = cs[0][0].nranks
        sizes = list(tgt_bytes) if isinstance(tgt_bytes, (list, tuple)) else [tgt_bytes] * self.n
        self.tgt_bytes = sizes
        self.src = {c.rank: Buf(src_bytes) for c, _ in cs}
        self.tgt = {c.rank: Buf(sizes[c.rank]) for c, _ in cs}
        with nccl_amd.group():
            self.swin = {c.rank: c.register_window(self.src[c.rank].ptr, src_bytes, SYM) for c, _ in cs}
        with nccl_amd.group():
            self.twin = {c.rank: c.register_window(self.tgt[c.rank].ptr, sizes[c.rank], tgt_flags) for c, _ in cs}
        assert all(w.handle for w in list(self.swin.values()) + list(self.twin.values()))
        self.src_bytes = src_bytes

    def release(self):
        for c, _ in self.cs:
            c.deregister_window(self.twin[c.rank])
            c.deregister_window(self.swin[c.rank])


def _dtype_for(nbytes, k):
    """One of uint8 / fp16 / fp32 / int64 whose size divides nbytes, rotating with k."""
    order = (1, 6, 7, 4)
    for i in range(4):
        dt = order[(k + i) % 4]
        if nbytes % TYPE_SIZE[dt] == 0:
            return dt
    return 1


class Phase:
    """The puts of one phase, in issue order: (src, dst, nbytes, src_mis, dst_off[, dtype]); `signals`: (src, dst)
    bare ncclSignal calls issued after the puts. Sources are laid out one after the other in the source window, each
    at a 16-byte boundary plus its misalignment. Puts of different sources to one target must not overlap."""

    def __init__(self, ar, puts, seed, signals=()):
        torch = _torch()
        self.ar, self.signals = ar, list(signals)
        self.src_img = {r: np.full(ar.src_bytes, FILL, dtype=np.uint8) for r in ar.src}
        self.want = {r: np.full(ar.tgt_bytes[r], FILL, dtype=np.uint8) for r in ar.tgt}
        self.puts = []
        cursor = {r: 0 for r in range(ar.n)}
        for k, p in enumerate(puts):
            src, dst, nbytes, smis, doff = p[:5]
            dtype = p[5] if len(p) > 5 else 1
            assert nbytes % TYPE_SIZE[dtype] == 0
            soff = (cursor[src] + 15) // 16 * 16 + smis
            cursor[src] = soff + nbytes
            assert cursor[src] <= ar.src_bytes
            data = _payload(nbytes, seed * 1000 + k)
            if src in self.src_img:
                self.src_img[src][soff:soff + nbytes] = data
            if dst in self.want:
                self.want[dst][doff:doff + nbytes] = data
            self.puts.append((src, dst, nbytes, soff, doff, dtype))
        for r, b in ar.src.items():
            b.view.copy_(torch.from_numpy(self.src_img[r]))
        for r, b in ar.tgt.items():   # the target fills its window with a kernel and reads it back
            b.store.fill_(FILL)
            assert int(b.store.cpu()[b.lo]) == FILL
        torch.cuda.synchronize()

    def expected_signals(self, dst):
        """{src: signals raised for dst in this phase}"""
        cnt = {}
        for src, d, *_ in self.puts:
            if d == dst:
                cnt[src] = cnt.get(src, 0) + 1
        for src, d in self.signals:
            if d == dst:
                cnt[src] = cnt.get(src, 0) + 1
        return cnt

    def issue_puts(self, comm, stream):
        ar, r = self.ar, comm.rank
        for src, dst, nbytes, soff, doff, dtype in self.puts:
            if src == r:
                comm.put_signal_raw(ar.src[r].ptr + soff, nbytes // TYPE_SIZE[dtype], dtype, dst, ar.twin[r], doff,
                                    stream.cuda_stream)
        for src, dst in self.signals:
            if src == r:
                comm.signal(dst, stream=stream)

    def issue_wait(self, comm, stream):
        cnt = self.expected_signals(comm.rank)
        if cnt:
            comm.wait_signal(sorted(cnt.items()), stream=stream)

    def finish(self, what):
        """After everything was issued: every rank reads its window with a kernel on its own stream, then the host
        compares the windows, their guard bytes and the (unchanged) sources."""
        torch = _torch()
        snaps, errs = {}, []
        for comm, stream in self.ar.cs:
            with torch.cuda.stream(stream):
                snaps[comm.rank] = self.ar.tgt[comm.rank].store.clone()
        for comm, stream in self.ar.cs:
            stream.synchronize()
            if comm.async_error():
                errs.append(f"rank {comm.rank} {what}: async error {comm.async_error()}")
        if errs:
            return errs
        for comm, _ in self.ar.cs:
            r = comm.rank
            b = self.ar.tgt[r]
            raw = snaps[r].cpu().numpy()
            got, want = raw[b.lo:b.lo + b.nbytes], self.want[r]
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                errs.append(f"rank {r} {what}: {bad.size} of {want.size} window bytes differ, first at {bad[:5].tolist()} "
                            f"got {got[bad[:3]].tolist()} want {want[bad[:3]].tolist()}")
            if not (np.all(raw[:b.lo] == FILL) and np.all(raw[b.lo + b.nbytes:] == FILL)):
                errs.append(f"rank {r} {what}: bytes outside the window were written")
            errs += self.ar.src[r].check(self.src_img[r], f"rank {r} {what} source")
        return errs


def rma_phase(ar, puts, seed, what, signals=()):
    """One phase in one group: every rank of this process issues its puts and signals, then one wait for everything the
    phase raises for it."""
    import nccl_amd
    ph = Phase(ar, puts, seed, signals)
    with nccl_amd.group():
        for comm, stream in ar.cs:
            ph.issue_puts(comm, stream)
            ph.issue_wait(comm, stream)
    return ph.finish(f"{what} seed={seed}")


# ---------------------------------------------------------------- spawned workers (kernel log, the wait that times out)

def _job_kernels():
    cs = _comms(2, CHUNK_ENV)
    ar = Arenas(cs, 1 << 20, 1 << 20)
    errs = rma_phase(ar, [(0, 1, 300_001, 0, 0), (1, 0, 17, 3, 5)], 1, "kernel log")
    ar.release()
    _destroy(cs)
    return errs


def _job_ordering():
    """Rank 0: one group of five puts to rank 1 at overlapping offsets (the last writer wins) and two bare signals.
    Rank 1 waits for 3 and then for 4 signals: exactly the seven raised. Then two puts whose data would cross if the
    stream's workgroups did not keep issue order: a 4096-byte misaligned put (one workgroup, element-wise stores) and an
    8192-byte put in two parts whose second part, on another workgroup that had nothing to do for the first put, covers
    the same bytes; the later put's data must stay. A last wait for one more signal must time out. The waiting rank's
    communicator is then aborted, not destroyed: its error word is set, and ncclCommDestroy's drain of outstanding
    credits is for communicators in working order; its peer, which never waited, is destroyed normally."""
    import nccl_amd
    cs = _comms(2, CHUNK_ENV)
    (c0, s0), (c1, s1) = cs
    ar = Arenas(cs, 1 << 20, 1 << 17)
    puts = [(0, 1, 70_001, 0, 100), (0, 1, 4097, 3, 50), (0, 1, 16, 0, 4000), (0, 1, 40_000, 1, 3000), (0, 1, 5, 0, 3003)]
    ph = Phase(ar, puts, 7, signals=[(0, 1), (0, 1)])
    with nccl_amd.group():
        ph.issue_puts(c0, s0)
    c1.wait_signal([(0, 3)], stream=s1)
    c1.wait_signal([(0, 2), (0, 2)], stream=s1)   # duplicate descriptors add up
    errs = ph.finish("ordering")
    if errs:
        return errs
    ph = Phase(ar, [(0, 1, 4096, 1, 6000), (0, 1, 8192, 0, 2000)], 8)
    with nccl_amd.group():
        ph.issue_puts(c0, s0)
    c1.wait_signal([(0, 2)], stream=s1)
    errs = ph.finish("data order across workgroups")
    if errs:
        return errs
    c1.wait_signal([(0, 1)], stream=s1)           # nothing left to consume: the spin times out
    s1.synchronize()
    if c1.async_error() == 0:
        errs.append("a wait for one more signal passed after every raised signal was consumed")
    c1.abort()
    c0.destroy()
    return errs


JOBS = {"kernels": _job_kernels, "ordering": _job_ordering}


def _worker_main(job, env, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
        os.environ.update(env)
        klog = f"/tmp/nccl_amd_rma_kernels_{os.getpid()}.log"
        if os.path.exists(klog):
            os.remove(klog)
        os.environ["NCCL_AMD_KERNEL_LOG"] = klog
        import torch
        torch.cuda.set_device(0)
        errs = JOBS[job]()
        torch.cuda.synchronize()
        out = (errs, open(klog).read().splitlines() if os.path.exists(klog) else [])
        if os.path.exists(klog):
            os.remove(klog)
        q.put(out)
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put(([f"exception {e!r}\n{traceback.format_exc()}"], []))


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


# ---------------------------------------------------------------- tests

@pytest.mark.parametrize("n", [2, 3])
def test_put_and_wait(built, n):
    """Every rank puts to the next and waits for the previous: 0 .. 4 MiB + 64 bytes in 4 KiB parts (the larger ones
    over many workgroups), source misaligned by 0 and 3, at window offset 0, 5 and ending exactly at the window's end,
    as uint8 / fp16 / fp32 / int64 where the size divides. Stale target lines, guard bytes, unchanged sources."""
    cs = _comms(n, CHUNK_ENV)
    tgt = BIG + 64
    ar = Arenas(cs, BIG + 16, tgt)
    errs, k = [], 0
    for nbytes in SIZES:
        for smis in (0, 3):
            for off in (0, 5, tgt - nbytes):
                k += 1
                dt = _dtype_for(nbytes, k)
                puts = [(r, (r + 1) % n, nbytes, smis, off, dt) for r in range(n)]
                errs += rma_phase(ar, puts, k, f"n={n} bytes={nbytes} smis={smis} off={off} dt={dt}")
        if errs:
            break
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_ordering_and_exact_counts(built):
    """Five overlapping puts and two signals in one group; waits of 3 and 4 consume exactly those; a third wait, under
    a 2 s spin timeout, reports an async error instead of passing."""
    errs, _ = _spawn("ordering", {"NCCL_AMD_SPIN_TIMEOUT_MS": "2000"})
    assert not errs, "\n".join(errs[:20])


def test_patterns(built):
    """The guide's three patterns at n = 4, self peers included: a barrier by ncclSignal, an all-to-all by put, and a
    ping-pong whose ping leaves late (a device-side delay in front of it, so the wait really waits) and whose reply is
    put straight out of the window the ping arrived in: the kernel behind the wait must read the ping's bytes."""
    import nccl_amd
    torch = _torch()
    n, blk = 4, 70_001
    cs = _comms(n, CHUNK_ENV)
    ar = Arenas(cs, n * (blk + 16), n * blk + 64)
    everyone = [(a, b) for a in range(n) for b in range(n)]
    errs = rma_phase(ar, [], 1, "barrier", signals=everyone)
    errs += rma_phase(ar, [(a, b, blk, 0, a * blk) for a, b in everyone], 2, "all-to-all")
    errs += rma_phase(ar, [(a, b, 1000 + 16 * a + b, 3, a * blk + 5) for a, b in everyone], 3, "all-to-all misaligned")
    errs += rma_phase(ar, [], 4, "barrier again", signals=everyone)
    # ping-pong between ranks 1 and 3, issued in dependency order; tensors through Communicator.put_signal
    (c1, s1), (c3, s3) = cs[1], cs[3]
    ph = Phase(ar, [(1, 3, 4099, 0, 64)], 5)
    src = ar.src[1].view[:4099]
    with torch.cuda.stream(s1):
        torch.cuda._sleep(40_000_000)   # the ping leaves tens of milliseconds late: rank 3's wait has to wait for it
    c1.put_signal(src, 3, ar.twin[1], 64, stream=s1)
    c3.wait_signal([(1, 1)], stream=s3)
    c3.put_signal(ar.tgt[3].view[64:64 + 4099], 1, ar.twin[3], 8192, stream=s3)   # forward what just arrived
    c1.wait_signal([(3, 1)], stream=s1)
    ph.want[1][8192:8192 + 4099] = ph.want[3][64:64 + 4099]
    errs += ph.finish("ping-pong")
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_one_rank(built):
    """A one-rank communicator: the guide's barrier and all-to-all loops with the only peer being oneself, overlapping
    self puts in issue order, an empty put."""
    cs = _comms(1, CHUNK_ENV)
    ar = Arenas(cs, 1 << 20, 1 << 20)
    errs = rma_phase(ar, [], 1, "one-rank barrier", signals=[(0, 0)])
    errs += rma_phase(ar, [(0, 0, 300_001, 3, 5)], 2, "one-rank all-to-all")
    errs += rma_phase(ar, [(0, 0, 70_001, 0, 100), (0, 0, 4097, 1, 50), (0, 0, 0, 0, 7), (0, 0, 8192, 0, 2000)], 3,
                      "one-rank overlapping puts", signals=[(0, 0)])
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("env", [CREDIT_ENVS[0], CREDIT_ENVS[3]], ids=["ag_pull", "push_tiny_slots"])
def test_interleaved_with_collectives(built, env):
    """Puts, signals and waits between AllReduce, Broadcast and send / recv on one communicator: the one-sided
    operations touch none of the pairs' sequences, and everything stays bit-exact."""
    from tests import gpu_cases as G
    n = 3
    cs = _comms(n, dict(env, **CHUNK_ENV))
    ar = Arenas(cs, 1 << 20, 1 << 20)
    ring = lambda nbytes, off: [(r, (r + 1) % n, nbytes, 0, off) for r in range(n)]  # noqa: E731
    errs = []
    for rep in range(2):
        errs += rma_phase(ar, ring(300_001, 5), 10 * rep + 1, f"rep {rep} ring")
        errs += G.run_case(cs, "allreduce", 7, 0, 300_001, 0, seed=100 + rep)
        errs += rma_phase(ar, [(a, b, 4097, 3, a * 8192) for a in range(n) for b in range(n)], 10 * rep + 2, f"rep {rep} all pairs")
        errs += bcast_case(cs, 300_001 * 4, 1, 2, "oop", seed=200 + rep)
        errs += p2p_case(cs, ring_shift(n, 70_001), 300 + rep, 1, f"rep {rep} send/recv")
        errs += rma_phase(ar, ring(17, 0), 10 * rep + 3, f"rep {rep} small ring", signals=[(0, 2), (2, 0)])
        errs += G.run_case(cs, "allreduce", 6, 2, 1_000, 0, seed=400 + rep)
        if errs:
            break
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:10])


def test_graph_capture(built):
    """A put + wait pair captured per rank, replayed three times with new contents."""
    import torch
    import nccl_amd
    cs = _comms(2, CHUNK_ENV)
    comms = [c for c, _ in cs]
    streams = [nccl_amd.dedicated_stream(0), nccl_amd.dedicated_stream(0)]
    nb = 300_001
    ar = Arenas(cs, 1 << 20, 1 << 20)
    graphs = [torch.cuda.CUDAGraph() for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(2):
        with torch.cuda.graph(graphs[r], stream=streams[r]):
            with nccl_amd.group():
                comms[r].put_signal_raw(ar.src[r].ptr + 3, nb, 1, 1 - r, ar.twin[r], 5, streams[r].cuda_stream)
                comms[r].wait_signal([(1 - r, 1)], stream=streams[r])
    errs = []
    for it in range(3):
        data = [_payload(nb, 600 + 2 * it + r) for r in range(2)]
        for r in range(2):
            ar.src[r].view[3:3 + nb].copy_(torch.from_numpy(data[r]))
            ar.tgt[r].store.fill_(FILL)
            assert int(ar.tgt[r].store.cpu()[0]) == FILL
        torch.cuda.synchronize()
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        snaps = []
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                snaps.append(ar.tgt[r].store.clone())
        torch.cuda.synchronize()
        for r in range(2):
            want = np.full(ar.tgt[r].store.numel(), FILL, dtype=np.uint8)
            lo = ar.tgt[r].lo + 5
            want[lo:lo + nb] = data[1 - r]
            if comms[r].async_error():
                errs.append(f"replay {it} rank {r}: async error {comms[r].async_error()}")
            elif not np.array_equal(snaps[r].cpu().numpy(), want):
                errs.append(f"replay {it} rank {r} differs")
    del graphs
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs)


def test_non_symmetric_window(built):
    """A window of another size on every rank is a valid target within the size the peer registered and refused beyond
    it; a source outside every symmetric window — a plain buffer, or that non-symmetric window — is refused. The
    refused calls enqueue nothing and the communicator goes on working."""
    import nccl_amd
    cs = _comms(2, CHUNK_ENV)
    (c0, s0), (c1, s1) = cs
    ar = Arenas(cs, 1 << 16, [4096, 12_288], NONSYM)
    plain = Buf(4096)

    def refused(fn):
        with pytest.raises(nccl_amd.NcclError) as ei:
            fn()
        assert ei.value.code == nccl_amd.Result.InvalidArgument

    refused(lambda: c1.put_signal_raw(ar.src[1].ptr, 4097, 1, 0, ar.twin[1], 0, s1.cuda_stream))       # rank 0 holds 4096
    refused(lambda: c1.put_signal_raw(ar.src[1].ptr, 16, 1, 0, ar.twin[1], 4090, s1.cuda_stream))
    refused(lambda: c0.put_signal_raw(ar.src[0].ptr, 2, 7, 1, ar.twin[0], 12_284, s0.cuda_stream))     # rank 1 holds 12 288
    refused(lambda: c0.put_signal_raw(plain.ptr, 16, 1, 1, ar.twin[0], 0, s0.cuda_stream))
    refused(lambda: c0.put_signal_raw(ar.tgt[0].ptr, 16, 1, 1, ar.twin[0], 0, s0.cuda_stream))
    refused(lambda: c0.put_signal_raw(ar.src[0].ptr + (1 << 16) - 8, 16, 1, 1, ar.twin[0], 0, s0.cuda_stream))
    # within the peer's size: rank 0 writes the last bytes of rank 1's 12 KiB (beyond its own 4 KiB), rank 1 the last of
    # rank 0's 4 KiB
    errs = rma_phase(ar, [(0, 1, 8192 + 3, 3, 4096 - 3), (1, 0, 4096, 0, 0)], 1, "non-symmetric target")
    errs += rma_phase(ar, [(0, 1, 1, 0, 12_287, 1), (1, 0, 8, 0, 4088, 4)], 2, "non-symmetric target, last bytes")
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def _mp_worker(rank, nranks, uid, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ.update(CHUNK_ENV)
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(nranks, rank, uid)
        cs = [(comm, torch.cuda.Stream())]
        ar = Arenas(cs, BIG + 16, BIG + 64)
        errs = []
        stream = cs[0][1]
        nxt, prv = (rank + 1) % nranks, (rank - 1) % nranks
        for i, nbytes in enumerate((1000, 300_001, BIG)):
            puts = [(r, (r + 1) % nranks, nbytes, 3 * (i % 2), 5 * i) for r in range(nranks)]
            ph = Phase(ar, puts, 800 + i)               # (refills this rank's window)
            # A one-sided writer must know that its target may be overwritten: this rank tells its predecessor that
            # its window is ready for the phase, and puts only once its successor has said the same. Ready signals
            # come from the successor and data signals from the predecessor: different senders, different words.
            comm.signal(prv, stream=stream)
            comm.wait_signal([(nxt, 1)], stream=stream)
            ph.issue_puts(comm, stream)                 # put to the next rank ...
            ph.issue_wait(comm, stream)                 # ... and wait for the previous one's
            errs += ph.finish(f"mp ring bytes={nbytes}")
        ar.release()
        comm.destroy()
        q.put((rank, errs))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"rank {rank} exception: {e!r}\n{traceback.format_exc()}"]))


def test_multi_process(built):
    """Three processes on one GPU, each putting to the next rank and waiting for the previous in its natural order;
    each process checks its own window."""
    _torch()
    import nccl_amd
    nranks = 3
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


def test_put_runs_the_put_kernel(built):
    """The kernel log of a put + wait exchange names rmaPutKernel and rmaWaitKernel and no staged kernel."""
    errs, kernels = _spawn("kernels", {})
    assert not errs, "\n".join(errs[:20])
    assert any("rmaPutKernel" in k for k in kernels) and any("rmaWaitKernel" in k for k in kernels), kernels
    assert not any("p2pKernel" in k or "collKernel" in k or "llKernel" in k for k in kernels), kernels
    grids = {int(k.split("grid=")[1].split()[0]) for k in kernels if "rmaPutKernel" in k}
    assert grids == {1, 32}, kernels   # 17 bytes: one workgroup; 300 001 bytes in 4 KiB parts: NCCL_MAX_P2P_NCHANNELS
