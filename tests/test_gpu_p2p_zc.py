"""GPU tests of the RDV (zero-copy rendezvous) protocol of ncclSend / ncclRecv: the payload bit for
bit in a recvbuff that lies in a registered window, every other byte of the window and around it untouched. All ranks
share GPU 0 under a tiny env: messages of 4096 bytes and more are RDV, 64 KiB spans four channels, and a message that
falls back walks its part in several staged slices."""
import multiprocessing as mp
import os
import queue

import numpy as np
import pytest

from tests.test_gpu_broadcast import CREDIT_ENVS, FILL, GUARD, Buf, _comms, _destroy, _payload, _torch, bcast_case
from tests.test_gpu_p2p import _finish, p2p_case
from tests.test_gpu_p2p_ll import LL_ENV

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
pytestmark = pytest.mark.gpu
ZC_ENV = {"NCCL_AMD_P2P_ZC_BYTES": "4096", "NCCL_AMD_P2P_CHUNK_BYTES": "16384", "NCCL_AMD_SLOT_BYTES": "4096"}
SIZES = (4095, 4096, 4097, 65536, 65537)   # staged; the threshold; a ragged tail; four full channels; a fifth of one byte
WIN, TAIL = 256 << 10, 128 << 10
SYM = 1   # NCCL_WIN_COLL_SYMMETRIC


class Arena:
    """Per rank a tensor of GUARD + WIN + TAIL bytes, FILL everywhere, whose bytes [GUARD, GUARD + WIN) are a window of
    the rank's communicator. take() places a recvbuff at a window offset (beyond WIN: outside the window) and notes
    what it must hold; check() compares every byte of every tensor with that image."""

    def __init__(self, cs, flags=0):
        import torch
        import nccl_amd
        self.cs = cs
        self.t = {c.rank: torch.full((GUARD + WIN + TAIL,), FILL, dtype=torch.uint8, device="cuda") for c, _ in cs}
        with nccl_amd.group():
            self.win = {c.rank: c.register_window(self.t[c.rank].data_ptr() + GUARD, WIN, flags) for c, _ in cs}
        self.reset()

    def reset(self):
        for t in self.t.values():
            t.fill_(FILL)
        self.want = {r: np.full(GUARD + WIN + TAIL, FILL, dtype=np.uint8) for r in self.t}
        self.top = {r: 0 for r in self.t}

    def take(self, r, want, at=None):
        """The address of want.size bytes at window offset `at` (None: the next free 16-byte boundary + GUARD)."""
        at = (self.top[r] + GUARD + 15) // 16 * 16 if at is None else at
        self.top[r] = max(self.top[r], at + want.size)
        self.want[r][GUARD + at: GUARD + at + want.size] = want
        return self.t[r].data_ptr() + GUARD + at

    def check(self, what):
        errs = []
        for r, t in self.t.items():
            bad = np.nonzero(t.cpu().numpy() != self.want[r])[0]
            if bad.size:
                errs.append(f"{what}: rank {r}'s window tensor differs at {bad.size} bytes, first {bad[:4].tolist()}")
        self.reset()
        return errs

    def release(self):
        for c, _ in self.cs:
            c.deregister_window(self.win[c.rank])


def zc_case(cs, ar, transfers, seed, what):
    """Like p2p_case: transfer (src, dst, nbytes, src_mis, at) is a send on src and a recv on dst, in list order; the
    recvbuff lies at window offset `at` of dst's arena tensor ("next": the next free place; None: in a plain Buf)."""
    import torch
    import nccl_amd
    mine = {c.rank: (c, s) for c, s in cs}
    plan, ptrs = [], []
    for k, (src, dst, nbytes, smis, at) in enumerate(transfers):
        want = _payload(nbytes, seed * 1000 + k)
        rb = Buf(nbytes) if at is None else None
        ptrs.append(rb.ptr if rb else ar.take(dst, want, None if at == "next" else at))
        plan.append((src, dst, nbytes, want, Buf(nbytes, smis, want), rb))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for r, (comm, stream) in mine.items():
            for (src, dst, nbytes, _, sb, _), rp in zip(plan, ptrs):
                if src == r:
                    comm.send_raw(sb.ptr, nbytes, 1, dst, stream.cuda_stream)
                if dst == r:
                    comm.recv_raw(rp, nbytes, 1, src, stream.cuda_stream)
    return _finish(mine, plan, what) + ar.check(what)


@pytest.fixture(scope="module")
def zc2(built):
    cs = _comms(2, ZC_ENV)
    arenas = {0: Arena(cs, 0), SYM: Arena(cs, SYM)}
    yield cs, arenas
    for a in arenas.values():
        a.release()
    _destroy(cs)


@pytest.mark.parametrize("nbytes", SIZES)
def test_sizes_offsets_and_windows(zc2, nbytes):
    cs, arenas = zc2
    errs, k = [], 0
    for flags, ar in arenas.items():
        for roff in (0, 16, 1, 3):
            for smis in (0, 1, 3):
                k += 1
                errs += zc_case(cs, ar, [(k % 2, 1 - k % 2, nbytes, smis, 4096 * (k % 3) + roff)], 100 + k,
                                f"flags={flags} roff={roff} smis={smis}")
        # fallback, not an error: the recvbuff in no window (behind this one's end), and straddling the window's end
        errs += zc_case(cs, ar, [(0, 1, nbytes, 0, WIN + 64), (1, 0, nbytes, 1, WIN - nbytes // 2)], 200 + flags, "fallback")
        errs += zc_case(cs, ar, [(1, 0, nbytes, 0, WIN - nbytes)], 300 + flags, "the window's last bytes")
    assert not errs, "\n".join(errs[:20])


def test_descriptor_line_reuse(built):
    """Nine RDV messages of one pair, each a group of its own, issued before the receiver's single group: the pair's
    one descriptor line carries them in turn. Then the mirror direction. Dedicated user streams, as in the LL test."""
    import torch
    import nccl_amd
    cs = [(c, nccl_amd.dedicated_stream(0)) for c, _ in _comms(2, ZC_ENV)]
    ar = Arena(cs)
    errs = []
    for src in (1, 0):
        (csend, ss), (cr, sr) = cs[src], cs[1 - src]
        wants = [_payload(4097 + 16 * k, 70 + 10 * src + k) for k in range(9)]
        sb = [Buf(w.size, k % 4, w) for k, w in enumerate(wants)]
        rp = [ar.take(1 - src, w) if k != 4 else None for k, w in enumerate(wants)]   # the fifth falls back
        rb = [None if p else Buf(w.size) for p, w in zip(rp, wants)]
        torch.cuda.synchronize()
        for b in sb:
            csend.send_raw(b.ptr, b.nbytes, 1, 1 - src, ss.cuda_stream)
        with nccl_amd.group():
            for p, b, w in zip(rp, rb, wants):
                cr.recv_raw(p or b.ptr, w.size, 1, src, sr.cuda_stream)
        plan = [(src, 1 - src, w.size, w, s, r) for w, s, r in zip(wants, sb, rb)]
        errs += _finish({0: cs[0], 1: cs[1]}, plan, f"nine messages from {src}") + ar.check(f"nine messages from {src}")
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_mixed_streams(built):
    """LL, staged, RDV-direct and RDV-fallback messages interleaved in one stream beside an all-pairs exchange, n = 3."""
    n, cs = 3, _comms(3, dict(LL_ENV, **ZC_ENV))
    ar = Arena(cs)
    stream = [(0, 1, b, k % 3, at) for k, (b, at) in enumerate([(5, "next"), (300_001 // 4, "next"), (2000, "next"), (200, None),
                                                               (4099, None), (65537, "next"), (256, "next"), (4096, "next")])]
    pairs = [(a, b, 100 * (a + 1) + 7 * b, 0, "next") for a in range(n) for b in range(n) if a != b]
    errs = zc_case(cs, ar, stream + pairs, 1, "mixed stream")
    errs += zc_case(cs, ar, pairs + stream, 2, "mixed stream, pairs first")
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_expanded_collectives(built, n):
    """ncclAlltoAll / ncclGather / ncclScatter with 4097-byte blocks, recvbuffs in windows, sendbuffs in plain memory."""
    import torch
    import nccl_amd
    cs, blk = _comms(n, ZC_ENV), 4097
    ar = Arena(cs)
    errs = []
    for kind, root in [("alltoall", 0)] + [(k, r) for r in range(n) for k in ("gather", "scatter")]:
        ins = {r: _payload(blk if kind == "gather" else n * blk, 50 * n + 7 * root + r) for r in range(n)}
        if kind == "alltoall":
            wants = {r: np.concatenate([ins[i][r * blk:(r + 1) * blk] for i in range(n)]) for r in range(n)}
        elif kind == "gather":
            wants = {root: np.concatenate([ins[i] for i in range(n)])}
        else:
            wants = {r: ins[root][r * blk:(r + 1) * blk] for r in range(n)}
        sb = {r: Buf(ins[r].size, 0, ins[r]) for r in range(n)}
        rp = {r: ar.take(r, wants[r]) if r in wants else None for r in range(n)}
        torch.cuda.synchronize()
        with nccl_amd.group():
            for comm, stream in cs:
                r, call = comm.rank, {"alltoall": comm.alltoall_raw, "gather": comm.gather_raw, "scatter": comm.scatter_raw}[kind]
                call(sb[r].ptr, rp[r], blk, 1, *(() if kind == "alltoall" else (root,)), stream.cuda_stream)
        what = f"{kind} n={n} root={root}"
        errs += _finish({c.rank: (c, s) for c, s in cs}, [(r, r, 0, ins[r], sb[r], None) for r in range(n)], what) + ar.check(what)
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("env", [CREDIT_ENVS[0], CREDIT_ENVS[3]], ids=["ag_pull", "push_tiny_slots"])
def test_sequences_survive(built, env):
    """RDV p2p, direct and fallen back, between staged and LL AllReduces, a Broadcast and staged p2p, twice through."""
    from tests import gpu_cases as G
    n, cs = 3, _comms(3, dict(env, **ZC_ENV))
    ar = Arena(cs)
    two = ("zc", [(0, 2, 4097, 1, "next"), (2, 0, 65537, 0, None), (0, 2, 20_001, 0, "next")])
    allp = ("zc", [(a, b, 5000 + 16 * a + b, 0, "next") for a in range(n) for b in range(n) if a != b])
    seq = [two, ("allreduce", 7, 0, 5, 0), allp, ("allreduce", 7, 0, 300_001, 0), two, ("broadcast", 70_001, 1),
           ("p2p", [(0, 2, 3001), (1, 0, 4095)]), allp]
    errs = []
    for rep in range(2):
        for i, op in enumerate(seq):
            if op[0] == "zc":
                errs += zc_case(cs, ar, op[1], 100 * rep + i, f"rep {rep} op {i}")
            elif op[0] == "p2p":
                errs += p2p_case(cs, op[1], 100 * rep + i, 1, f"rep {rep} op {i}")
            elif op[0] == "broadcast":
                errs += bcast_case(cs, op[1], 1, op[2], "oop", seed=2000 * rep + i)
            else:
                coll, dt, rop, count, root = op
                errs += G.run_case(cs, coll, dt, rop, count, 0, seed=1000 * rep + i, root=root)
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs[:10])


def test_graph_capture(built):
    """An RDV exchange captured per rank (the descriptor is baked into the kernel's arguments), replayed three times."""
    import torch
    import nccl_amd
    cs, nb = _comms(2, ZC_ENV), 20_001
    ar = Arena(cs)
    streams = [nccl_amd.dedicated_stream(0), nccl_amd.dedicated_stream(0)]
    x = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    y = [ar.take(r, np.zeros(nb, dtype=np.uint8), 48 + r) for r in range(2)]
    graphs = [torch.cuda.CUDAGraph() for _ in range(2)]
    torch.cuda.synchronize()
    for r, (comm, _) in enumerate(cs):
        with torch.cuda.graph(graphs[r], stream=streams[r]), nccl_amd.group():
            comm.send_raw(x[r].data_ptr(), nb, 1, 1 - r, streams[r].cuda_stream)
            comm.recv_raw(y[r], nb, 1, 1 - r, streams[r].cuda_stream)
    errs = []
    for it in range(3):
        for r in range(2):
            want = _payload(nb, 600 + 2 * it + r)
            x[r].copy_(torch.from_numpy(want))
            ar.take(1 - r, want, 48 + 1 - r)
        torch.cuda.synchronize()
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        torch.cuda.synchronize()
        errs += [f"replay {it} rank {c.rank}: async error {c.async_error()}" for c, _ in cs if c.async_error()]
        errs += ar.check(f"replay {it}")
    del graphs
    ar.release()
    _destroy(cs)
    assert not errs, "\n".join(errs)


def _kernel_worker(q):
    """Communicators made before the knob was ever set, with it, and after it was unset; the kernel log names a kernel
    at its first launch, so the third's run comes first. The knob alone here: the memory figures are compared."""
    try:
        klog = os.environ["NCCL_AMD_KERNEL_LOG"] = f"/tmp/nccl_amd_p2p_zc_kernels_{os.getpid()}.log"
        dlog = os.environ["NCCL_DEBUG_FILE"] = f"/tmp/nccl_amd_p2p_zc_debug_{os.getpid()}.log"
        os.environ["NCCL_DEBUG"] = "TRACE"
        before, on, after = _comms(2), _comms(2, {"NCCL_AMD_P2P_ZC_BYTES": "4096"}), _comms(2)
        mem = [cs[0][0].mem_stats() for cs in (before, on, after)]
        ar_off, ar_on = Arena(after), Arena(on)
        errs = []
        for k, nbytes in enumerate(SIZES):
            errs += zc_case(after, ar_off, [(k % 2, 1 - k % 2, nbytes, 0, 32)], k, "knob unset")
        off_names = open(klog).read().splitlines()
        for k, nbytes in enumerate(SIZES[1:]):
            errs += zc_case(on, ar_on, [(k % 2, 1 - k % 2, nbytes, 0, 32)], 10 + k, "knob set")
        on_names = open(klog).read().splitlines()[len(off_names):]
        trace = [ln.split("rdv messages")[1].strip() for ln in open(dlog).read().splitlines() if "rdv messages" in ln]
        os.remove(klog)
        os.remove(dlog)
        ar_off.release()
        ar_on.release()
        _destroy(before + on + after)
        q.put((errs, mem, off_names, on_names, trace))
    except Exception as e:  # report instead of hanging the parent
        q.put(([f"exception {e!r}"], [], [], [], []))


def test_which_kernel_ran(built):
    """RDV sizes run p2pZcKernel under the knob, every recvbuff in the window served direct (the TRACE line); without
    the knob p2pKernel alone, on exactly the memory held before."""
    _torch()
    q = (ctx := mp.get_context("spawn")).Queue()
    p = ctx.Process(target=_kernel_worker, args=(q,))
    p.start()
    try:
        errs, mem, off_names, on_names, trace = q.get(timeout=240)
    except queue.Empty:
        p.kill()
        raise AssertionError("the worker did not report")
    p.join(timeout=60)
    assert not errs, "\n".join(errs[:20])
    off_p2p, on_p2p = [[k for k in names if "p2p" in k] for names in (off_names, on_names)]
    assert off_p2p and all("p2pKernel" in k for k in off_p2p), off_names
    assert on_p2p and all("p2pZcKernel" in k for k in on_p2p), on_names
    # one line per launch: the sender's counts no received message, the receiver's its one, direct
    assert sorted(trace) == 4 * ["1 (received: 0 direct, 0 fell back)"] + 4 * ["1 (received: 1 direct, 0 fell back)"], trace
    # the RDV area and counter rows: at most 256 channels x (16 lines + 16 done words + 2 x 16 counters), rounded up
    assert mem[2] == mem[0] and mem[0] < mem[1] <= mem[0] + 256 * (384 + 256) + 512, mem
