"""ncclBroadcast / ncclBcast with the recvbuff in an NCCL_WIN_COLL_SYMMETRIC window run zero-copy under
NCCL_AMD_SYM_BCAST=1 (kernels.h symBcastKernel): pulls only, owner blocks, a direct variant for small
payloads. Every case compares the WHOLE of each rank's window and of a side buffer outside any window, byte for byte,
with the image numpy predicts — nothing is folded, so there is no tolerance. All ranks share the one GPU; set-up,
teardown and the other collectives of the epoch test are tests/test_gpu_sym_alltoall.py's."""
import multiprocessing as mp
import os
import queue

import numpy as np
import pytest

from tests import test_gpu_sym_alltoall as A
from tests.test_gpu_sym_alltoall import SEND_OFF, WIN_BYTES, Rank, _diff, _setup, _teardown

pytestmark = pytest.mark.gpu

# ^LL: sizes the table would hand to the LL plan keep it (they are no zero-copy Broadcasts), so every size here is direct
BASE = {"NCCL_AMD_SYM_BCAST": "1", "NCCL_PROTO": "^LL"}
SETTINGS = {
    "default": (BASE, 16384),
    # few channels and ragged parts; the small minimum also makes the two-phase variant reachable at small sizes
    "few-channels": ({**BASE, "NCCL_AMD_MIN_CHANNEL_BYTES": "4096", "NCCL_MAX_CTAS": "3", "NCCL_MIN_CTAS": "2"}, 4096),
    "elementwise": ({**BASE, "NCCL_AMD_FORCE_ELEMENTWISE": "1"}, 16384),
}


def _issue(rk, nbytes, root, mode, off, sid):
    """mode: "win" root's sendbuff in the window; "ext" root's sendbuff outside any window and a garbage sendbuff
    pointer on non-roots; "inplace" ncclBcast; "staged" like "ext" with the recvbuff outside any window too."""
    rbuf = rk.ext if mode == "staged" else rk.win
    rp = rbuf.data_ptr() + rk.recv_base(mode == "staged") + off
    if mode == "inplace":
        rk.comm.bcast(rbuf[rp - rbuf.data_ptr():rp - rbuf.data_ptr() + nbytes], root, stream=sid)
    elif rk.comm.rank == root:
        rk.comm.broadcast_raw((rk.win if mode == "win" else rk.ext).data_ptr() + SEND_OFF + off, rp, nbytes, 0, root, sid)
    else:
        rk.comm.broadcast_raw(0xDEAD0 if mode == "ext" else None, rp, nbytes, 0, root, sid)


def run_bcast(ranks, nbytes, root, mode, seed, off=0, replay=None):
    """One Broadcast of `nbytes` over the local `ranks`; `replay`: (graph, stream) per rank that captured this call."""
    import torch
    import nccl_amd
    data = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8))
    images = []
    for rk in ranks:
        rk.win.fill_(0x5A)
        rk.ext.fill_(0xC3)
        outside = mode == "staged"
        lo = rk.recv_base(outside) + off
        if rk.comm.rank == root:
            src = rk.win if mode in ("win", "inplace") else rk.ext
            at = lo if mode == "inplace" else SEND_OFF + off
            src[at:at + nbytes].copy_(data)
        images.append((rk.win.clone(), rk.ext.clone()))
        images[-1][outside][lo:lo + nbytes].copy_(data)
    torch.cuda.synchronize()
    if replay:
        for g, s in replay:
            with torch.cuda.stream(s):
                g.replay()
        torch.cuda.synchronize()
    else:
        with nccl_amd.group():
            for rk in ranks:
                _issue(rk, nbytes, root, mode, off, rk.stream.cuda_stream)
    errs = []
    for rk, (want_win, want_ext) in zip(ranks, images):
        rk.stream.synchronize()
        what = f"rank {rk.comm.rank} bcast n={rk.comm.nranks} bytes={nbytes} root={root} mode={mode} off={off}"
        if rk.comm.async_error():
            errs.append(f"{what}: async error {rk.comm.async_error()}")
            continue
        errs += _diff(rk.win, want_win, what + ": window") + _diff(rk.ext, want_ext, what + ": outside buffer")
    return errs


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("n", [2, 3, 8])
def test_payloads(built, n, setting):
    env, min_chan = SETTINGS[setting]
    sw = (n - 1) * min_chan
    payloads = [1,          # trailing blocks empty (n >= 3: only the first owner holds bytes)
                8202,       # no multiple of 16: a byte tail, and the last block ends short
                sw - 1,     # the last size of the direct variant (at n = 2 every size is direct)
                sw + 1,     # the first two-phase size: blocks of one minimum part, the last one 1 byte over a 16-multiple
                300_001]    # several channels per block
    ranks = _setup(n, env)
    errs = []
    for root in (0, n - 1):
        for mode in ("win", "ext", "inplace"):
            for i, nbytes in enumerate(payloads):
                errs += run_bcast(ranks, nbytes, root, mode, seed=1000 * n + 10 * root + i)
    errs += run_bcast(ranks, 70_001, n - 1, "win", seed=7, off=3)  # recvbuff 3 bytes past the window offset: byte path
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


def _job_path(mode, zero_copy):
    klog = f"/tmp/nccl_amd_sym_bcast_kernels_{os.getpid()}.log"
    os.environ["NCCL_AMD_KERNEL_LOG"] = klog      # read when the library loads
    ranks = _setup(3, BASE)
    errs = run_bcast(ranks, 300_001, 2, mode, seed=1) + run_bcast(ranks, 8202, 0, mode, seed=2)
    _teardown(ranks)
    kernels = open(klog).read().splitlines()
    os.remove(klog)
    sym = [k for k in kernels if "symBcastKernel" in k]
    staged = [k for k in kernels if "collKernel<unsigned char, 0, 6>" in k]
    return errs if ((sym and not staged) if zero_copy else (staged and not sym)) else errs + [f"kernels: {kernels}"]


def _job_rank(rank, nranks, uid):
    import torch
    import nccl_amd
    rk = Rank(nccl_amd.Communicator.init(nranks, rank, uid), torch.cuda.Stream())
    rk.handle = rk.comm.register_window(rk.win.data_ptr(), WIN_BYTES)
    errs = run_bcast([rk], 300_001, 3, "ext", seed=1) + run_bcast([rk], 8202, 3, "inplace", seed=2)
    _teardown([rk])
    return errs


def _child(job, args, q):
    try:
        os.environ.update({"NCCL_AMD_SPIN_TIMEOUT_MS": "30000", **BASE})
        import torch
        torch.cuda.set_device(0)
        q.put(job(*args))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put([f"{args}: exception {e!r}\n{traceback.format_exc()}"])


def _spawn(job, arg_sets):
    """One spawned process per argument set (the knobs and the kernel log are read when the library loads); the errors
    they report."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_child, args=(job, a, q)) for a in arg_sets]
    for p in ps:
        p.start()
    errs = []
    try:
        for _ in ps:
            errs += q.get(timeout=240)
    except queue.Empty:
        errs.append("a worker did not report")
        for p in ps:
            p.kill()
    for p in ps:
        p.join(timeout=60)
    return errs


@pytest.mark.parametrize("mode,zero_copy", [("ext", True), ("staged", False)])
def test_kernel_path(built, mode, zero_copy):
    """Knob on and recvbuff in a symmetric window: the kernel log names symBcastKernel and no staged Broadcast kernel
    (the parent of this change ignores the knob and fails here); recvbuff outside any window: the staged kernel. Both
    exact."""
    errs = _spawn(_job_path, [(mode, zero_copy)])
    assert not errs, "\n".join(errs[:20])


def test_epochs_and_graph(built):
    """n = 3, one communicator and window set; twice over: Broadcasts of rotating roots and both variants between a
    symmetric AllReduce, AllGather and AlltoAll and a staged Broadcast. Then one two-phase Broadcast captured per rank
    and replayed three times with new payloads: the kernel's state is in device counters."""
    import torch
    import nccl_amd
    ranks = _setup(3, BASE)
    errs = []
    for rnd in range(2):
        s = 100 * rnd
        errs += run_bcast(ranks, 300_001, rnd, "win", seed=s + 1)                   # two-phase
        errs += A._other_coll(ranks, "allreduce", 100_003, s + 2)
        errs += run_bcast(ranks, 8202, rnd + 1, "inplace", seed=s + 3)              # direct
        errs += A._other_coll(ranks, "allgather", 30_001, s + 4)
        errs += run_bcast(ranks, 70_001, (rnd + 2) % 3, "ext", seed=s + 5)          # two-phase, fewer channels
        errs += A.run_case(ranks, "alltoall", 7, 20_001, seed=s + 6)
        errs += run_bcast(ranks, 100_001, rnd, "staged", seed=s + 7)                # recvbuff outside the window
        errs += run_bcast(ranks, 1, 2 - rnd, "win", seed=s + 8)                     # direct, one channel
    streams = [nccl_amd.dedicated_stream(0) for _ in ranks]
    graphs = [torch.cuda.CUDAGraph() for _ in ranks]
    torch.cuda.synchronize()
    for rk, g, st in zip(ranks, graphs, streams):
        with torch.cuda.graph(g, stream=st):
            _issue(rk, 300_001, 1, "win", 0, st.cuda_stream)
    for it in range(3):
        errs += run_bcast(ranks, 300_001, 1, "win", seed=900 + it, replay=list(zip(graphs, streams)))
    del graphs
    _teardown(ranks)
    assert not errs, "\n".join(errs[:20])


def test_multi_process(built):
    """Four processes on the GPU (the windows mapped into each other through dma-buf), root 3: a two-phase and a
    direct Broadcast; each process checks its own rank."""
    import nccl_amd
    uid = nccl_amd.get_unique_id()
    errs = _spawn(_job_rank, [(r, 4, uid) for r in range(4)])
    assert not errs, "\n".join(errs[:20])
