"""GPU tests of the LL protocol of ncclSend / ncclRecv: the payload itself, bit for bit, guard bytes
untouched. All ranks share GPU 0 under the tiny LL env: 128 payload bytes per channel and slot on two channels, so
messages of up to 256 bytes are LL and 257 bytes are staged."""
import multiprocessing as mp
import os
import queue

import numpy as np
import pytest

from tests.test_gpu_broadcast import CREDIT_ENVS, TYPE_SIZE, Buf, _comms, _destroy, _payload, _torch, bcast_case
from tests.test_gpu_p2p import _finish, coll_case, p2p_case

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
pytestmark = pytest.mark.gpu
LL_ENV = {"NCCL_AMD_P2P_LL_BYTES": "256", "NCCL_AMD_P2P_LL_LINE_BYTES": "256", "NCCL_AMD_P2P_LL_NCHANNELS": "2"}
DEPTH = 4   # kP2pLLDepth
# one unit, a ragged tail, one channel exactly, the spill into the second, the capacity; none; staged
SIZES = (1, 7, 8, 9, 127, 128, 129, 255, 256, 0, 257)


@pytest.fixture(scope="module")
def ll2(built):
    cs = _comms(2, LL_ENV)
    yield cs
    _destroy(cs)


def _typed(cs, sizes, seed):
    """Every size in every type that divides it, 0 -> 1 and 1 -> 0."""
    errs = []
    for nbytes in sizes:
        for dtype in (1, 7, 4):
            if nbytes % TYPE_SIZE[dtype] == 0:
                for src in (0, 1):
                    seed += 1
                    errs += p2p_case(cs, [(src, 1 - src, nbytes)], seed, dtype, "ll pair")
    return errs


@pytest.mark.parametrize("nbytes", SIZES)
def test_sizes_and_alignments(ll2, nbytes):
    errs = _typed(ll2, [nbytes], 100 * nbytes)
    for k, (smis, dmis) in enumerate((s, d) for s in (0, 1, 3) for d in (0, 1, 3)):
        errs += p2p_case(ll2, [(k % 2, 1 - k % 2, nbytes, smis, dmis)], 50 + k, 1, f"ll pair mis=({smis},{dmis})")
    assert not errs, "\n".join(errs[:20])


def test_slot_reuse_and_credit(built):
    """2 x depth + 1 messages of 129 bytes, each a group of its own, all issued before the receiver's one group: the
    fifth waits for the ack of the first. Then the mirror direction, the pair's sequences now uneven. The user streams
    have hardware queues of their own: a receiver's fork queued behind the waiting sender's join would never run."""
    import torch
    import nccl_amd
    cs = [(c, nccl_amd.dedicated_stream(0)) for c, _ in _comms(2, dict(LL_ENV, NCCL_AMD_NSLOTS="4"))]
    errs = []
    for src in (1, 0):
        (csend, ss), (cr, sr) = cs[src], cs[1 - src]
        wants = [_payload(129, 70 + 10 * src + k) for k in range(2 * DEPTH + 1)]
        sb = [Buf(129, 0, w) for w in wants]
        rb = [Buf(129) for _ in wants]
        torch.cuda.synchronize()
        for b in sb:
            csend.send_raw(b.ptr, 129, 1, 1 - src, ss.cuda_stream)
        with nccl_amd.group():
            for b in rb:
                cr.recv_raw(b.ptr, 129, 1, src, sr.cuda_stream)
        plan = [(src, 1 - src, 129, w, s, r) for w, s, r in zip(wants, sb, rb)]
        errs += _finish({0: cs[0], 1: cs[1]}, plan, f"nine messages from {src}")
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_mixed_streams(built):
    """LL and staged messages interleaved in one stream beside an all-pairs exchange at n = 3."""
    n, cs = 3, _comms(3, LL_ENV)
    stream = [(0, 1, b) for b in (5, 300_001, 0, 200, 4099, 256)]
    pairs = [(a, b, 100 * (a + 1) + 7 * b) for a in range(n) for b in range(n) if a != b]
    errs = p2p_case(cs, stream + pairs, 1, 1, "mixed stream")
    errs += p2p_case(cs, pairs + stream, 2, 1, "mixed stream, pairs first")
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_expanded_collectives(built, n):
    """ncclAlltoAll / ncclGather / ncclScatter with 129-byte blocks get the LL path through their expansion."""
    cs = _comms(n, LL_ENV)
    errs = coll_case(cs, "alltoall", 129, 10 * n)
    for root in range(n):
        errs += coll_case(cs, "gather", 129, 10 * n + 1 + root, root)
        errs += coll_case(cs, "scatter", 129, 10 * n + 20 + root, root)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("env", [CREDIT_ENVS[0], CREDIT_ENVS[3]], ids=["ag_pull", "push_tiny_slots"])
def test_sequences_survive(built, env):
    """LL p2p between ranks 0 and 2 alone and all pairs, between LL and staged AllReduces, a Broadcast and staged p2p."""
    from tests import gpu_cases as G
    n, cs = 3, _comms(3, dict(env, **LL_ENV))
    two = ("p2p", [(0, 2, 129), (2, 0, 65)])
    allp = ("p2p", [(a, b, 100 + 16 * a + b) for a in range(n) for b in range(n) if a != b])
    seq = [two, ("allreduce", 7, 0, 5, 0), allp, ("allreduce", 7, 0, 300_001, 0), two, ("broadcast", 70_001, 1),
           ("p2p", [(0, 2, 100_003), (1, 0, 4099)]), allp]
    errs = []
    for rep in range(2):
        for i, op in enumerate(seq):
            if op[0] == "p2p":
                errs += p2p_case(cs, op[1], 100 * rep + i, 1, f"rep {rep} op {i}")
            elif op[0] == "broadcast":
                errs += bcast_case(cs, op[1], 1, op[2], "oop", seed=2000 * rep + i)
            else:
                coll, dt, rop, count, root = op
                errs += G.run_case(cs, coll, dt, rop, count, 0, seed=1000 * rep + i, root=root)
    _destroy(cs)
    assert not errs, "\n".join(errs[:10])


def test_graph_capture(built):
    """An LL-sized exchange and an LL-sized ncclAlltoAll captured per rank, replayed three times with new contents."""
    import torch
    import nccl_amd
    cs = _comms(2, LL_ENV)
    comms = [c for c, _ in cs]
    streams = [nccl_amd.dedicated_stream(0), nccl_amd.dedicated_stream(0)]
    nb, blk = 200, 129
    x, y, a, b = [[torch.zeros(k, dtype=torch.uint8, device="cuda") for _ in range(2)] for k in (nb, nb, 2 * blk, 2 * blk)]
    graphs = [torch.cuda.CUDAGraph() for _ in range(2)]
    torch.cuda.synchronize()
    for r in range(2):
        with torch.cuda.graph(graphs[r], stream=streams[r]):
            with nccl_amd.group():
                comms[r].send_raw(x[r].data_ptr(), nb, 1, 1 - r, streams[r].cuda_stream)
                comms[r].recv_raw(y[r].data_ptr(), nb, 1, 1 - r, streams[r].cuda_stream)
            comms[r].alltoall_raw(a[r].data_ptr(), b[r].data_ptr(), blk, 1, streams[r].cuda_stream)
    errs = []
    for it in range(3):
        wx = [_payload(nb, 600 + 2 * it + r) for r in range(2)]
        wa = [_payload(2 * blk, 700 + 2 * it + r) for r in range(2)]
        for r in range(2):
            x[r].copy_(torch.from_numpy(wx[r]))
            a[r].copy_(torch.from_numpy(wa[r]))
            y[r].zero_()
            b[r].zero_()
        torch.cuda.synchronize()
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        torch.cuda.synchronize()
        for r in range(2):
            wb = np.concatenate([wa[i][r * blk:(r + 1) * blk] for i in range(2)])
            if comms[r].async_error():
                errs.append(f"replay {it} rank {r}: async error {comms[r].async_error()}")
            elif not (np.array_equal(y[r].cpu().numpy(), wx[1 - r]) and np.array_equal(b[r].cpu().numpy(), wb)):
                errs.append(f"replay {it} rank {r} differs")
    del graphs
    _destroy(cs)
    assert not errs, "\n".join(errs)


def _kernel_worker(q):
    """Communicators made before the knob was ever set, with it, and after it was unset; the kernel log names a kernel
    at its first launch, so the third's run comes first."""
    try:
        klog = os.environ["NCCL_AMD_KERNEL_LOG"] = f"/tmp/nccl_amd_p2p_ll_kernels_{os.getpid()}.log"
        before, on, after = _comms(2), _comms(2, LL_ENV), _comms(2)
        mem = [cs[0][0].mem_stats() for cs in (before, on, after)]
        errs = _typed(after, SIZES[:9], 0)
        off_names = open(klog).read().splitlines()
        errs += _typed(on, SIZES[:9], 500)
        on_names = open(klog).read().splitlines()[len(off_names):]
        os.remove(klog)
        _destroy(before + on + after)
        q.put((errs, mem, off_names, on_names))
    except Exception as e:  # report instead of hanging the parent
        q.put(([f"exception {e!r}"], [], [], []))


def test_which_kernel_ran(built):
    """LL sizes run p2pLLKernel under the LL env; without it p2pKernel alone, on exactly the memory held before."""
    _torch()
    q = (ctx := mp.get_context("spawn")).Queue()
    p = ctx.Process(target=_kernel_worker, args=(q,))
    p.start()
    try:
        errs, mem, off_names, on_names = q.get(timeout=240)
    except queue.Empty:
        p.kill()
        raise AssertionError("the worker did not report")
    p.join(timeout=60)
    assert not errs, "\n".join(errs[:20])
    assert any("p2pKernel" in k for k in off_names) and not any("p2pLLKernel" in k for k in off_names), off_names
    assert any("p2pLLKernel" in k for k in on_names) and not any("p2pKernel" in k for k in on_names), on_names
    assert mem[2] == mem[0] and mem[1] == mem[0] + 2 * DEPTH * 2 * 256, mem
