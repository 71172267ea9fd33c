"""ncclAlltoAll / ncclGather with the sendbuff in an NCCL_WIN_COLL_SYMMETRIC window run zero-copy (kernels.h
symA2AKernel): every rank pulls its blocks straight out of the peers' windows. Results are compared
byte for byte with the permutation computed in numpy — nothing is folded, so there is no tolerance — and every case
compares the WHOLE of each rank's window and of an unregistered side buffer with their expected images, which checks
the bytes around the recv range, the sendbuffs and everything else no collective may touch. All ranks share the one
GPU (single process: init_all on a repeated device; multi-process: dma-buf mappings of the windows). Cases that read
the kernel log run in spawned workers (NCCL_AMD_KERNEL_LOG is read when the library loads)."""
import multiprocessing as mp
import os
import queue

import numpy as np
import pytest

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
pytestmark = pytest.mark.gpu

WIN_BYTES = 8 << 20           # per-rank window: sendbuffs from SEND_OFF, recvbuffs from HALF
HALF = WIN_BYTES // 2
EXT_BYTES = 4 << 20           # per-rank buffer outside any window, same layout at half the size
SEND_OFF = 4096
TYPE_SIZE = {0: 1, 2: 4, 6: 2, 7: 4, 8: 8}   # int8, int32, fp16, fp32, fp64
# (datatype, elements per rank pair): 1 byte; 7 fp32; 4101 fp16 = 8202 bytes, no multiple of 16, so most blocks are
# misaligned; 70 001 fp32 = several channels; fp64
PAYLOADS = [(0, 1), (7, 7), (6, 4101), (7, 70_001), (8, 1001)]
SETTINGS = {
    "default": {},
    # few channels, a ragged last part, and for the 1-byte payload a second channel with nothing to copy
    "few-channels": {"NCCL_AMD_MIN_CHANNEL_BYTES": "4096", "NCCL_MAX_CTAS": "3", "NCCL_MIN_CTAS": "2"},
    "elementwise": {"NCCL_AMD_FORCE_ELEMENTWISE": "1"},
}


class Rank:
    """One local rank: its communicator and stream, its registered window and a buffer outside any window."""

    def __init__(self, comm, stream):
        import torch
        self.comm, self.stream = comm, stream
        self.win = torch.empty(WIN_BYTES, dtype=torch.uint8, device="cuda")
        self.ext = torch.empty(EXT_BYTES, dtype=torch.uint8, device="cuda")
        self.handle = None

    def buf(self, outside):
        return self.ext if outside else self.win

    def recv_base(self, outside):
        return (EXT_BYTES if outside else WIN_BYTES) // 2


def _setup(n, env=None, flags=None):
    """n ranks on GPU 0 in this process, created under `env` (the knobs are read at communicator init), windows
    registered with `flags` (default symmetric)."""
    import torch
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
    ranks = [Rank(c, torch.cuda.Stream()) for c in comms]
    with nccl_amd.group():
        for r in ranks:
            r.handle = r.comm.register_window(r.win.data_ptr(), WIN_BYTES,
                                              nccl_amd.WIN_COLL_SYMMETRIC if flags is None else flags)
    assert all(r.handle.handle for r in ranks)
    return ranks


def _teardown(ranks):
    for r in ranks:
        r.comm.deregister_window(r.handle)
    for r in ranks:
        r.comm.destroy()


def _blocks(n, nbytes, seed):
    """Every rank's sendbuff contents (all n of them, whichever ranks are local): rank r's is row r."""
    return np.random.default_rng(seed).integers(0, 256, size=(n, nbytes), dtype=np.uint8)


def _diff(got, want, what):
    import torch
    if torch.equal(got, want):
        return []
    bad = torch.nonzero(got != want).flatten()
    return [f"{what}: {bad.numel()} bytes differ, first at {bad[:4].tolist()} got {got[bad[:4]].tolist()} "
            f"want {want[bad[:4]].tolist()}"]


def run_case(ranks, coll, dtype, count, off=0, seed=0, root=0, send_outside=False, recv_outside=False, inplace=False,
             launch=None):
    """One AlltoAll (`coll` "alltoall") or Gather over the local `ranks`. sendbuffs at the same offset on every rank
    (`off` elements past SEND_OFF; in the window unless send_outside), recvbuffs `off` elements past the buffer's
    middle; inplace (Gather): every sendbuff sits where the root's block of the root's recvbuff is, so that on the root
    sendbuff == recvbuff + root * count. Non-roots of a Gather pass no recvbuff."""
    import torch
    import nccl_amd
    n = ranks[0].comm.nranks
    es = TYPE_SIZE[dtype]
    B = count * es
    gather = coll == "gather"
    send = _blocks(n, B if gather else n * B, seed)
    images, places = [], []
    for rk in ranks:
        r = rk.comm.rank
        rk.win.fill_(0x5A)
        rk.ext.fill_(0xC3)
        recv_off = rk.recv_base(recv_outside) + off * es
        send_off = SEND_OFF + off * es
        if inplace:
            assert gather and not send_outside and not recv_outside
            send_off = recv_off + root * B
        sbuf, rbuf = rk.buf(send_outside), rk.buf(recv_outside)
        sbuf[send_off:send_off + send.shape[1]].copy_(torch.from_numpy(send[r]))
        places.append((sbuf.data_ptr() + send_off, rbuf.data_ptr() + recv_off))
    torch.cuda.synchronize()
    for rk in ranks:
        r = rk.comm.rank
        want_win, want_ext = rk.win.clone(), rk.ext.clone()
        if not gather or r == root:
            exp = send.reshape(n * B) if gather else np.concatenate([send[q, r * B:(r + 1) * B] for q in range(n)])
            recv_off = rk.recv_base(recv_outside) + off * es
            (want_ext if recv_outside else want_win)[recv_off:recv_off + n * B].copy_(torch.from_numpy(exp))
        images.append((want_win, want_ext))
    torch.cuda.synchronize()

    def issue():
        for rk, (sp, rp) in zip(ranks, places):
            if gather:
                rk.comm.gather_raw(sp, rp if rk.comm.rank == root else None, count, dtype, root, rk.stream.cuda_stream)
            else:
                rk.comm.alltoall_raw(sp, rp, count, dtype, rk.stream.cuda_stream)

    if launch is not None:
        launch(issue)
    else:
        with nccl_amd.group():
            issue()
    errs = []
    what = (f"{coll} n={n} dt={dtype} count={count} off={off} root={root} send_outside={send_outside} "
            f"recv_outside={recv_outside} inplace={inplace}")
    for rk, (want_win, want_ext) in zip(ranks, images):
        rk.stream.synchronize()
        if rk.comm.async_error():
            errs.append(f"rank {rk.comm.rank} {what}: async error {rk.comm.async_error()}")
            continue
        errs += _diff(rk.win, want_win, f"rank {rk.comm.rank} {what}: window")
        errs += _diff(rk.ext, want_ext, f"rank {rk.comm.rank} {what}: outside buffer")
    return errs


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("n", [2, 3, 5])
def test_alltoall_parity(built, n, setting):
    """recv[r][q] == send[q][r] for all r, q; the bytes on both sides of the recv range, every sendbuff and the rest of
    both buffers unchanged (the whole-buffer images of run_case); no async error."""
    ranks = _setup(n, SETTINGS[setting])
    errs = []
    for i, (dtype, count) in enumerate(PAYLOADS):
        for off in (0, 3):
            errs += run_case(ranks, "alltoall", dtype, count, off=off, seed=1000 * n + 10 * i + off)
        if errs:
            break
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 2. the path (spawned: kernel log)

def _job_path(scenario):
    """AlltoAll and a Gather with every root on n = 3; what differs per scenario is where the buffers lie."""
    import nccl_amd
    flags = nccl_amd.WIN_DEFAULT if scenario == "win-default" else None
    ranks = _setup(3, flags=flags)
    kw = {"send_outside": scenario == "send-outside", "recv_outside": scenario == "recv-outside"}
    errs = run_case(ranks, "alltoall", 7, 70_001, seed=1, **kw)
    errs += run_case(ranks, "alltoall", 6, 4101, off=3, seed=2, **kw)
    for root in range(3):
        errs += run_case(ranks, "gather", 7, 30_001, seed=3 + root, root=root, **kw)
    _teardown(ranks)
    return errs


def _worker_main(job, arg, env, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ.update(env)
        klog = f"/tmp/nccl_amd_sym_a2a_kernels_{os.getpid()}.log"
        dlog = f"/tmp/nccl_amd_sym_a2a_debug_{os.getpid()}.log"
        for f in (klog, dlog):
            if os.path.exists(f):
                os.remove(f)
        os.environ["NCCL_AMD_KERNEL_LOG"] = klog
        if "NCCL_DEBUG" in env:
            os.environ["NCCL_DEBUG_FILE"] = dlog
        import torch
        torch.cuda.set_device(0)
        errs = JOBS[job](arg)
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


def _spawn(job, arg, env):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_main, args=(job, arg, env, q))
    p.start()
    try:
        out = q.get(timeout=240)
    except queue.Empty:
        p.kill()
        raise AssertionError(f"worker {job} {arg} did not report")
    p.join(timeout=60)
    return out


@pytest.mark.parametrize("scenario,env,zero_copy", [
    ("window", {"NCCL_DEBUG": "TRACE"}, True),
    ("recv-outside", {}, True),              # only sendbuffs are read remotely: the recvbuff needs no window
    ("send-outside", {}, False),
    ("win-default", {}, False),              # a window registered without NCCL_WIN_COLL_SYMMETRIC
    ("window", {"NCCL_AMD_SYM_A2A": "0"}, False),
    ("window", {"NCCL_AMD_SYM_DISABLE": "1"}, False),
], ids=["window", "recv-outside", "send-outside", "win-default", "knob-off", "sym-disabled"])
def test_kernel_path(built, scenario, env, zero_copy):
    """With the sendbuff in a symmetric window the kernel log names symA2AKernel and no p2pKernel — AlltoAll, and Gather
    with every root; with the sendbuff outside any window, with NCCL_AMD_SYM_A2A=0, with NCCL_AMD_SYM_DISABLE=1 and with
    a window that is not symmetric, p2pKernel only. The same results in every case."""
    errs, kernels, log = _spawn("path", scenario, env)
    assert not errs, "\n".join(errs[:20])
    a2a = [k for k in kernels if "symA2AKernel" in k]
    p2p = [k for k in kernels if "p2pKernel" in k]
    if zero_copy:
        assert a2a and not p2p, kernels
    else:
        assert p2p and not a2a, kernels
    if "NCCL_DEBUG" in env:
        assert any("AlltoAll: symmetric nch " in ln and " part " in ln for ln in log.splitlines()), log[-2000:]
        assert any("Gather: symmetric nch " in ln and " part " in ln for ln in log.splitlines()), log[-2000:]


# ---------------------------------------------------------------- 3. Gather

def test_gather_every_root(built):
    """n = 3, every root: non-roots pass no recvbuff and nothing of theirs is written (their whole window and side
    buffer keep their images); in place at the root (sendbuff == recvbuff + root * count, both in the window);
    misaligned blocks; a one-byte payload; a root recvbuff outside any window."""
    ranks = _setup(3)
    errs = []
    for root in range(3):
        errs += run_case(ranks, "gather", 7, 70_001, seed=40 + root, root=root)
        errs += run_case(ranks, "gather", 6, 4101, off=3, seed=50 + root, root=root)
        errs += run_case(ranks, "gather", 0, 1, seed=60 + root, root=root)
        errs += run_case(ranks, "gather", 7, 30_001, seed=70 + root, root=root, inplace=True)
        errs += run_case(ranks, "gather", 8, 1001, seed=80 + root, root=root, recv_outside=True)
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 4. epoch sequence

def _i32(n, count, seed):
    return np.random.default_rng(seed).integers(-1000, 1000, size=(n, count), dtype=np.int32)


def _other_coll(ranks, kind, count, seed, outside=False):
    """One int32 collective of the other kinds over all ranks of this process (n = len(ranks)), checked exactly:
    allreduce / allgather / reducescatter with both buffers in the windows (symmetric kernels), broadcast and a
    send/recv ring on buffers outside them (staged)."""
    import torch
    import nccl_amd
    n = len(ranks)
    total = count * (n if kind == "reducescatter" else 1)
    data = _i32(n, total, seed)
    out_count = {"allreduce": count, "allgather": n * count, "reducescatter": count, "broadcast": count, "ring": count}[kind]
    for rk in ranks:
        b = rk.buf(outside)
        b[SEND_OFF:SEND_OFF + total * 4].copy_(torch.from_numpy(data[rk.comm.rank].view(np.uint8)))
        b[rk.recv_base(outside):rk.recv_base(outside) + out_count * 4].zero_()
    torch.cuda.synchronize()
    with nccl_amd.group():
        for rk in ranks:
            b, r, sid = rk.buf(outside), rk.comm.rank, rk.stream.cuda_stream
            sp, rp = b.data_ptr() + SEND_OFF, b.data_ptr() + rk.recv_base(outside)
            if kind == "allreduce":
                rk.comm.all_reduce_raw(sp, rp, count, 2, 0, sid)
            elif kind == "allgather":
                rk.comm.all_gather_raw(sp, rp, count, 2, sid)
            elif kind == "reducescatter":
                rk.comm.reduce_scatter_raw(sp, rp, count, 2, 0, sid)
            elif kind == "broadcast":
                rk.comm.broadcast_raw(sp, rp, count, 2, 1, sid)
            else:
                rk.comm.send_raw(sp, count, 2, (r + 1) % n, sid)
                rk.comm.recv_raw(rp, count, 2, (r - 1) % n, sid)
    errs = []
    for rk in ranks:
        rk.stream.synchronize()
        r = rk.comm.rank
        want = {"allreduce": lambda: data.sum(axis=0, dtype=np.int32), "allgather": lambda: data.reshape(-1),
                "reducescatter": lambda: data.sum(axis=0, dtype=np.int32)[r * count:(r + 1) * count],
                "broadcast": lambda: data[1], "ring": lambda: data[(r - 1) % n]}[kind]()
        base = rk.recv_base(outside)
        got = rk.buf(outside)[base:base + out_count * 4].cpu().numpy().view(np.int32)
        if rk.comm.async_error():
            errs.append(f"rank {r} {kind}: async error {rk.comm.async_error()}")
        elif not np.array_equal(got, want):
            errs.append(f"rank {r} {kind} count {count}: {(got != want).sum()} elements differ")
    return errs


def test_epoch_sequence(built):
    """One communicator, n = 3; twice over: symmetric AllReduce, zero-copy AlltoAll, staged AlltoAll, symmetric
    AllGather, zero-copy Gather, staged send/recv ring, symmetric ReduceScatter, zero-copy AlltoAll, staged Broadcast.
    The payloads differ, so consecutive launches use different channel counts: the zero-copy kernel leaves the channels'
    symmetric epochs and the staged sequences as every other kernel expects them."""
    ranks = _setup(3, {"NCCL_PROTO": "^LL"})
    errs = []
    for rnd in range(2):
        s = 100 * rnd
        errs += _other_coll(ranks, "allreduce", 100_003, s + 1)
        errs += run_case(ranks, "alltoall", 7, 70_001, seed=s + 2)
        errs += run_case(ranks, "alltoall", 7, 20_001, seed=s + 3, send_outside=True, recv_outside=True)
        errs += _other_coll(ranks, "allgather", 30_001, s + 4)
        errs += run_case(ranks, "gather", 2, 5000, seed=s + 5, root=rnd + 1)
        errs += _other_coll(ranks, "ring", 50_001, s + 6, outside=True)
        errs += _other_coll(ranks, "reducescatter", 40_003, s + 7)
        errs += run_case(ranks, "alltoall", 6, 4101, off=3, seed=s + 8)
        errs += _other_coll(ranks, "broadcast", 60_001, s + 9, outside=True)
        if errs:
            break
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 5. groups

def test_group_with_p2p_and_allreduce(built):
    """One group holding, per rank and in this order: a zero-copy AlltoAll, a send/recv exchange with the next rank, an
    AllReduce, a second zero-copy AlltoAll at other offsets. All exact; ncclGroupSimulateEnd on the same group succeeds
    with a positive time."""
    import torch
    import nccl_amd
    n = 3
    ranks = _setup(n, {"NCCL_PROTO": "^LL"})
    c1, c2, cx, car = 70_001, 4101, 9001, 50_003       # fp32 AlltoAll, fp16 AlltoAll, int32 exchange, int32 AllReduce
    a1, a2 = _blocks(n, n * c1 * 4, 1), _blocks(n, n * c2 * 2, 2)
    xs, ar = _i32(n, cx, 3), _i32(n, car, 4)
    # window: AlltoAll 1 send / recv, AlltoAll 2 send / recv (3 elements past), AllReduce in / out; outside: the exchange
    o_a1s, o_a2s, o_ars = SEND_OFF, SEND_OFF + (1 << 20) + 6, SEND_OFF + (2 << 20)
    o_a1r, o_a2r, o_arr = HALF, HALF + (1 << 20) + 6, HALF + (2 << 20)
    for rk in ranks:
        r = rk.comm.rank
        rk.win.zero_()
        rk.ext.zero_()
        rk.win[o_a1s:o_a1s + a1.shape[1]].copy_(torch.from_numpy(a1[r]))
        rk.win[o_a2s:o_a2s + a2.shape[1]].copy_(torch.from_numpy(a2[r]))
        rk.win[o_ars:o_ars + car * 4].copy_(torch.from_numpy(ar[r].view(np.uint8)))
        rk.ext[SEND_OFF:SEND_OFF + cx * 4].copy_(torch.from_numpy(xs[r].view(np.uint8)))
    torch.cuda.synchronize()

    def issue():
        for rk in ranks:
            r, w, e, sid = rk.comm.rank, rk.win.data_ptr(), rk.ext.data_ptr(), rk.stream.cuda_stream
            rk.comm.alltoall_raw(w + o_a1s, w + o_a1r, c1, 7, sid)
            rk.comm.send_raw(e + SEND_OFF, cx, 2, (r + 1) % n, sid)
            rk.comm.recv_raw(e + EXT_BYTES // 2, cx, 2, (r - 1) % n, sid)
            rk.comm.all_reduce_raw(w + o_ars, w + o_arr, car, 2, 0, sid)
            rk.comm.alltoall_raw(w + o_a2s, w + o_a2r, c2, 6, sid)

    nccl_amd.group_start()
    issue()
    sim = nccl_amd.group_end(simulate=True)
    assert sim.estimated_time > 0
    with nccl_amd.group():
        issue()
    errs = []
    for rk in ranks:
        rk.stream.synchronize()
        r = rk.comm.rank
        if rk.comm.async_error():
            errs.append(f"rank {r}: async error {rk.comm.async_error()}")
            continue
        for name, got, want in (
                ("AlltoAll 1", rk.win[o_a1r:o_a1r + n * c1 * 4],
                 np.concatenate([a1[q, r * c1 * 4:(r + 1) * c1 * 4] for q in range(n)])),
                ("AlltoAll 2", rk.win[o_a2r:o_a2r + n * c2 * 2],
                 np.concatenate([a2[q, r * c2 * 2:(r + 1) * c2 * 2] for q in range(n)])),
                ("exchange", rk.ext[EXT_BYTES // 2:EXT_BYTES // 2 + cx * 4], xs[(r - 1) % n].view(np.uint8)),
                ("AllReduce", rk.win[o_arr:o_arr + car * 4], ar.sum(axis=0, dtype=np.int32).view(np.uint8))):
            if not np.array_equal(got.cpu().numpy(), want):
                errs.append(f"rank {r}: {name} differs")
    _teardown(ranks)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------- 6. buffer reuse after return

def test_sendbuff_reusable_in_stream_order(built):
    """20 iterations without host synchronisation: AlltoAll, the output copied aside, then the sendbuff overwritten on
    the same stream with the next iteration's pattern. When the kernel has finished every peer has finished reading
    this rank's sendbuff (the DONE round), so every iteration's output is exact."""
    import torch
    import nccl_amd
    n, iters, count = 3, 20, 16_389          # int32: 65 556 bytes per block
    B = count * 4
    ranks = _setup(n)
    pats = [_blocks(n, n * B, 500 + it) for it in range(iters)]
    dev = [[torch.from_numpy(pats[it][rk.comm.rank]).cuda() for it in range(iters)] for rk in ranks]
    aside = [torch.zeros(iters, n * B, dtype=torch.uint8, device="cuda") for _ in ranks]
    for i, rk in enumerate(ranks):
        rk.win.zero_()
        rk.win[SEND_OFF:SEND_OFF + n * B].copy_(dev[i][0])
    torch.cuda.synchronize()
    for it in range(iters):
        with nccl_amd.group():
            for rk in ranks:
                w = rk.win.data_ptr()
                rk.comm.alltoall_raw(w + SEND_OFF, w + HALF, count, 2, rk.stream.cuda_stream)
        for i, rk in enumerate(ranks):
            with torch.cuda.stream(rk.stream):
                aside[i][it].copy_(rk.win[HALF:HALF + n * B])
                if it + 1 < iters:
                    rk.win[SEND_OFF:SEND_OFF + n * B].copy_(dev[i][it + 1])
    errs = []
    for i, rk in enumerate(ranks):
        rk.stream.synchronize()
        r = rk.comm.rank
        if rk.comm.async_error():
            errs.append(f"rank {r}: async error {rk.comm.async_error()}")
            continue
        got = aside[i].cpu().numpy()
        for it in range(iters):
            want = np.concatenate([pats[it][q, r * B:(r + 1) * B] for q in range(n)])
            if not np.array_equal(got[it], want):
                errs.append(f"rank {r} iteration {it}: {(got[it] != want).sum()} bytes differ")
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 7. stream capture

def test_graph_capture(built):
    """One zero-copy AlltoAll captured per rank, replayed three times with new sendbuff contents: all of the kernel's
    state is in device counters."""
    import torch
    import nccl_amd
    n, count = 2, 70_001
    B = count * 4
    ranks = _setup(n)
    streams = [nccl_amd.dedicated_stream(0) for _ in ranks]
    graphs = [torch.cuda.CUDAGraph() for _ in ranks]
    torch.cuda.synchronize()
    for rk, g, s in zip(ranks, graphs, streams):
        with torch.cuda.graph(g, stream=s):
            rk.comm.alltoall_raw(rk.win.data_ptr() + SEND_OFF, rk.win.data_ptr() + HALF, count, 7, s.cuda_stream)
    errs = []
    for it in range(3):
        send = _blocks(n, n * B, 900 + it)
        for rk in ranks:
            rk.win.zero_()
            rk.win[SEND_OFF:SEND_OFF + n * B].copy_(torch.from_numpy(send[rk.comm.rank]))
        torch.cuda.synchronize()
        for g, s in zip(graphs, streams):
            with torch.cuda.stream(s):
                g.replay()
        torch.cuda.synchronize()
        for rk in ranks:
            r = rk.comm.rank
            want = np.concatenate([send[q, r * B:(r + 1) * B] for q in range(n)])
            if rk.comm.async_error():
                errs.append(f"replay {it} rank {r}: async error {rk.comm.async_error()}")
            elif not np.array_equal(rk.win[HALF:HALF + n * B].cpu().numpy(), want):
                errs.append(f"replay {it} rank {r} differs")
    del graphs
    _teardown(ranks)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------- 8. multi-process

def _mp_worker(rank, nranks, uid, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        rk = Rank(nccl_amd.Communicator.init(nranks, rank, uid), torch.cuda.Stream())
        rk.handle = rk.comm.register_window(rk.win.data_ptr(), WIN_BYTES)
        errs = []
        for i, (dtype, count, off) in enumerate([(7, 7, 0), (6, 4101, 3), (7, 70_001, 0)]):
            errs += run_case([rk], "alltoall", dtype, count, off=off, seed=700 + i)
        errs += run_case([rk], "alltoall", 7, 70_001, seed=710, recv_outside=True)
        errs += run_case([rk], "gather", 7, 30_001, seed=720, root=1)
        _teardown([rk])
        q.put((rank, errs))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"rank {rank} exception: {e!r}\n{traceback.format_exc()}"]))


def test_multi_process(built):
    """Three processes on the GPU (the windows mapped into each other through dma-buf): a quick subset of the parity
    list and one Gather; each process checks its own rank."""
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


JOBS = {"path": _job_path}
