"""GPU tests of ncclLLA2ASession (include/nccl_device_ll_a2a.h) through tests/native/devapi_lla2a_kernels.hip: every
received word against the exact pattern, the fused AllReduce bit for bit against a numpy fold in rank order, the epoch
wrap over stale flagged lines. Ranks share the one GPU: up to 3 in this process, one spawned process each above. Every
case has a DevComm of its own with one zero-filled session block per CTA (grid 2)."""
import ctypes
import multiprocessing as mp
import os
import traceback

import numpy as np
import pytest

from tests.test_gpu_device_api import ROOT, _cs, _grouped, _torch

pytestmark = pytest.mark.gpu
M, EPOCHS, K, GRID = 3, 5, 70, 2            # values per peer; epochs per launch; AllReduce elements per CTA; CTAs
COOPS = {"thread": 0, "warp": 1, "cta128": 2}
WORDS = {"4B": 1, "8B": 2, "12B": 3, "16B": 4, "24B": 6}
_K = []


def _k():
    if not _K:
        import nccl_amd
        nccl_amd.load()
        _K.append(ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libdevapi_lla2a_kernels.so")))
        P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        _K[0].lla2a_exchange.argtypes = [P, U, U, I, I, I, I, U, P, P]
        _K[0].lla2a_allreduce.argtypes = [P, U, U, I, P, P, I, I, P]
        _K[0].lla2a_block.argtypes = [P, U, U, U, I, U, U, U, U, P, P]
    return _K[0]


def exchange(rs, n, ns, coop, words, stored=0, launches=((0, EPOCHS, M), (EPOCHS, EPOCHS, M))):
    """`launches` (first round, epochs, values per peer) of the exchange kernel on every rank of this process."""
    torch, k = _torch(), _k()
    outs = [[torch.zeros(GRID * ep * n * m * words, dtype=torch.int32, device="cuda") for _, ep, m in launches] for _ in rs]
    word = torch.zeros(GRID, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for li, (seq0, ep, m) in enumerate(launches):
        for (dc, s), out in zip(rs, outs):
            assert k.lla2a_exchange(dc.ptr, dc.buffer_handles[0], ns, coop, words, m, ep, seq0, out[li].data_ptr(), s.cuda_stream) == 0
    for _ in range(sum(ep for _, ep, _ in launches)):    # ncclLLA2ANextEpoch on stored + 2, minus 2
        stored = (stored + (1 if stored != 0xFFFFFFFD else 3)) & 0xFFFFFFFF
    for (dc, s), out in zip(rs, outs):
        for b in range(GRID):
            assert k.lla2a_block(dc.ptr, dc.buffer_handles[0], ns, b, 0, 0, 0, 0, 0, word.data_ptr() + 4 * b, s.cuda_stream) == 0
        s.synchronize()
        for li, (seq0, ep, m) in enumerate(launches):   # [block][epoch][from][j][word], as the kernel's comment has it
            b, e, f, j, w = np.ix_(*(np.arange(x, dtype=np.uint32) for x in (GRID, ep, n, m, words)))
            want = b << 31 | f << 27 | np.uint32(dc.comm.rank) << 23 | ((seq0 + e) & 0xff) << 15 | j << 8 | w
            got = out[li].cpu().numpy().view(np.uint32).reshape(want.shape)
            bad = np.argwhere(got != want)
            assert not len(bad), (dc.comm.rank, li, len(bad), bad[0].tolist(), hex(got[tuple(bad[0])]))
        assert word.cpu().numpy().view(np.uint32).tolist() == [stored] * GRID and not dc.comm.async_error(), dc.comm.rank


def wrap(rs, n, ns):
    """Every slot of both parities holds a stale line flagged 2 (even) or 3 (odd), the stored epoch is 0xFFFFFFFA. One
    launch of one value per peer runs the epochs ...FC to ...FF and overwrites only the first 2n lines of each parity;
    the next, of three values per peer, runs 2 to 5 and polls 6n lines, 4n of them stale unless endEpoch cleared them."""
    torch, word = _torch(), _torch().zeros(1, dtype=_torch().int32, device="cuda")
    for dc, s in rs:
        for b in range(GRID):
            assert _k().lla2a_block(dc.ptr, dc.buffer_handles[0], ns, b, 1, 0xFFFFFFFA, 2, 3, 0xDEADBEEF, word.data_ptr(), s.cuda_stream) == 0
    torch.cuda.synchronize()                            # every rank's lines are prepared before any kernel starts
    exchange(rs, n, ns, COOPS["cta128"], WORDS["16B"], 0xFFFFFFFA, ((252, 4, 1), (0, 4, M)))


def allreduce(rs, n, ns, kind, graph=False):
    torch, k = _torch(), _k()
    dt, tdt = (np.float32, torch.float32) if kind == "f32" else (np.float64, torch.float64)
    ins = [torch.zeros(GRID * K, dtype=tdt, device="cuda") for _ in rs]
    outs = [torch.zeros(GRID * K, dtype=tdt, device="cuda") for _ in rs]
    launch = lambda dc, stream, i, o: k.lla2a_allreduce(dc.ptr, dc.buffer_handles[0], ns, kind == "f64", i.data_ptr(),
                                                        o.data_ptr(), K, GRID, stream)
    if graph:       # one rank per process: captured once, replayed with new inputs
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            assert launch(rs[0][0], torch.cuda.current_stream().cuda_stream, ins[0], outs[0]) == 0
    for rep in range(3 if graph else 2):
        xs = []
        for r in range(n):                  # mixed magnitudes; the fold rounds per add, in rank order 0 .. n-1
            rng = np.random.default_rng(1000 * n + 10 * rep + r)
            xs.append((rng.standard_normal(GRID * K) * 10.0 ** rng.integers(-3, 4, GRID * K)).astype(dt))
        want = xs[0]
        for x in xs[1:]:
            want = (want + x).astype(dt)
        for (dc, _), i, o in zip(rs, ins, outs):
            i.copy_(torch.from_numpy(xs[dc.comm.rank]))
            o.fill_(float("nan"))
        torch.cuda.synchronize()
        if graph:
            g.replay()
        for (dc, s), i, o in zip(rs, ins, outs):
            assert graph or launch(dc, s.cuda_stream, i, o) == 0
        for (dc, s), o in zip(rs, outs):
            s.synchronize()
            torch.cuda.synchronize()
            assert o.cpu().numpy().tobytes() == want.tobytes() and not dc.comm.async_error(), (dc.comm.rank, kind, rep)


def _job(cs, n, job, args):
    import nccl_amd
    ns = n * K                              # >= ncclLLA2ACalcSlots(n * M, 24) = 3 * n * M lines, too
    dcs = _grouped(cs, lambda c, s: c.dev_comm_create(0, [nccl_amd.lla2a_requirement(GRID, ns)]))
    try:
        globals()[job]([(dc, s) for dc, (_, s) in zip(dcs, cs)], n, ns, *args)
    finally:
        _torch().cuda.synchronize()
        for dc in dcs:
            dc.comm.dev_comm_destroy(dc)


def _rank_main(rank, n, uid, job, args, q):
    try:
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(n, rank, uid)
        _job([(comm, torch.cuda.Stream())], n, job, args)
        comm.destroy()
        q.put("")
    except Exception:  # report instead of hanging the parent
        q.put(f"rank {rank}: {traceback.format_exc()}")


def _run(n, job, *args):
    """One case on n ranks: in this process up to 3 (dedicated streams), one spawned process per rank above."""
    if n <= 3:
        cs = _cs(n)
        try:
            return _job(cs, n, job, args)
        finally:
            for c, _ in cs:
                c.destroy()
    import nccl_amd
    uid, ctx = nccl_amd.get_unique_id(), mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rank_main, args=(r, n, uid, job, args, q)) for r in range(n)]
    for p in ps:
        p.start()
    try:
        errs = [e for e in (q.get(timeout=240) for _ in ps) if e]
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("words", list(WORDS))
@pytest.mark.parametrize("coop", list(COOPS))
@pytest.mark.parametrize("n", [2, 3, 8])
def test_exchange(built, n, coop, words):
    _run(n, "exchange", COOPS[coop], WORDS[words])


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("n", [2, 3, 5, 8])     # recvReduce<4>: a remainder of 2 alone, of 3 alone, 4 + 1, 4 + 4
def test_allreduce_recv_reduce(built, n, kind):
    _run(n, "allreduce", kind)


def test_allreduce_graph_replay(built):
    _run(5, "allreduce", "f32", True)


@pytest.mark.parametrize("n", [2, 3])
def test_epoch_wrap(built, n):
    _run(n, "wrap")
