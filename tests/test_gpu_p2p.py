"""GPU tests of ncclSend / ncclRecv and of ncclAlltoAll / ncclGather / ncclScatter: payloads are random bytes from a
seed, the expected outputs plain numpy slicing, compared bit for bit.

Ranks share the box's one GPU (ncclCommInitAll with a repeated device, NCCL_MULTI_RANK_GPU_ENABLE=1) or run as spawned
processes; cases that read the kernel log or the debug log run in a spawned worker, as in tests/test_gpu_broadcast.py,
whose buffer helper (guard bytes in front and behind, checked unchanged) is used here too."""
import multiprocessing as mp
import os
import queue
import subprocess

import numpy as np

import pytest

from tests.test_gpu_broadcast import CREDIT_ENVS, TYPE_SIZE, Buf, _comms, _destroy, _payload, _torch, bcast_case

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_ENV = {"NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2", "NCCL_MAX_CTAS": "7"}
BIG = (4 << 20) + 64


def p2p_case(cs, transfers, seed, dtype=1, what="", recv_streams=None):
    """One group per rank of this process: every transfer (src, dst, nbytes[, src_mis, dst_mis]) is a send on rank src
    and a recv on rank dst, issued in list order. Only the ranks in `cs` are driven and checked (one per process in
    the multi-process test); payloads depend on the seed and the transfer's index alone. recv_streams: rank -> the
    stream its recvs are issued on instead of its own. Returns error strings."""
    import torch
    import nccl_amd
    ts = TYPE_SIZE[dtype]
    mine = {comm.rank: (comm, stream) for comm, stream in cs}
    plan = []
    for k, t in enumerate(transfers):
        src, dst, nbytes = t[:3]
        smis, dmis = (t[3], t[4]) if len(t) > 3 else (0, 0)
        assert nbytes % ts == 0
        want = _payload(nbytes, seed * 1000 + k)
        sb = Buf(nbytes, smis, want) if src in mine else None
        rb = Buf(nbytes, dmis) if dst in mine else None
        plan.append((src, dst, nbytes, want, sb, rb))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for r, (comm, stream) in mine.items():
            for src, dst, nbytes, _, sb, rb in plan:
                if src == r:
                    comm.send_raw(sb.ptr, nbytes // ts, dtype, dst, stream.cuda_stream)
                if dst == r:
                    rs = recv_streams[r] if recv_streams else stream
                    comm.recv_raw(rb.ptr, nbytes // ts, dtype, src, rs.cuda_stream)
    for rs in (recv_streams or {}).values():
        rs.synchronize()
    return _finish(mine, plan, f"{what} seed={seed} dt={dtype}")


def _finish(mine, plan, what):
    errs = []
    for r, (comm, stream) in mine.items():
        stream.synchronize()
        if comm.async_error():
            errs.append(f"rank {r} {what}: async error {comm.async_error()}")
    if errs:
        return errs
    for k, (src, dst, nbytes, want, sb, rb) in enumerate(plan):
        if rb is not None:
            errs += rb.check(want, f"{what} transfer {k} ({src}->{dst}, {nbytes} bytes) recv")
        if sb is not None:  # the input is untouched
            errs += sb.check(want, f"{what} transfer {k} ({src}->{dst}, {nbytes} bytes) send")
    return errs


def coll_case(cs, kind, block, seed, root=0, dtype=1):
    """ncclAlltoAll / ncclGather / ncclScatter with blocks of `block` bytes on every rank of this process."""
    import torch
    import nccl_amd
    n = cs[0][0].nranks
    ts = TYPE_SIZE[dtype]
    assert block % ts == 0
    ins, wants = {}, {}
    if kind == "alltoall":
        for r in range(n):
            ins[r] = _payload(n * block, seed * 100 + r)
        for r in range(n):
            wants[r] = np.concatenate([ins[i][r * block:(r + 1) * block] for i in range(n)])
    elif kind == "gather":
        for r in range(n):
            ins[r] = _payload(block, seed * 100 + r)
        wants[root] = np.concatenate([ins[i] for i in range(n)])
    else:
        ins[root] = _payload(n * block, seed * 100)
        for r in range(n):
            wants[r] = ins[root][r * block:(r + 1) * block]
    bufs = {}
    for comm, _ in cs:
        r = comm.rank
        sb = Buf(ins[r].size, 0, ins[r]) if r in ins else None
        rb = Buf(wants[r].size) if r in wants else None
        bufs[r] = (sb, rb)
    torch.cuda.synchronize()
    with nccl_amd.group():
        for comm, stream in cs:
            sb, rb = bufs[comm.rank]
            sp, rp = (sb.ptr if sb else None), (rb.ptr if rb else None)
            if kind == "alltoall":
                comm.alltoall_raw(sp, rp, block // ts, dtype, stream.cuda_stream)
            elif kind == "gather":
                comm.gather_raw(sp, rp, block // ts, dtype, root, stream.cuda_stream)
            else:
                comm.scatter_raw(sp, rp, block // ts, dtype, root, stream.cuda_stream)
    errs = []
    what = f"{kind} n={n} block={block} root={root} seed={seed}"
    for comm, stream in cs:
        stream.synchronize()
        if comm.async_error():
            errs.append(f"rank {comm.rank} {what}: async error {comm.async_error()}")
    if errs:
        return errs
    for comm, _ in cs:
        sb, rb = bufs[comm.rank]
        if rb is not None:
            errs += rb.check(wants[comm.rank], f"rank {comm.rank} {what} recv")
        if sb is not None:
            errs += sb.check(ins[comm.rank], f"rank {comm.rank} {what} send")
    return errs


def ring_shift(n, nbytes):
    return [(r, (r + 1) % n, nbytes) for r in range(n)]


# ---------------------------------------------------------------- spawned workers (kernel log / debug log)

def _job_pairs():
    """n = 2 under the tiny-slot env: every size in every type that divides it, both directions; then every source x
    destination misalignment at every size, as bytes."""
    cs = _comms(2)
    errs, seed = [], 0
    sizes = (0, 1, 15, 16, 17, 4095, 4096, 4097, 70_001, 300_001 * 4, BIG)
    for nbytes in sizes:
        for dtype in (1, 6, 7, 4):
            if nbytes % TYPE_SIZE[dtype]:
                continue
            for src in (0, 1):
                seed += 1
                errs += p2p_case(cs, [(src, 1 - src, nbytes)], seed, dtype, "pair")
        if errs:
            break
    for nbytes in sizes:
        for smis in (0, 1, 3):
            for dmis in (0, 1, 3):
                seed += 1
                errs += p2p_case(cs, [(seed % 2, 1 - seed % 2, nbytes, smis, dmis)], seed, 1, f"pair mis=({smis},{dmis})")
        if errs:
            break
    _destroy(cs)
    return errs


def _job_mixed():
    """One group per rank: an AllReduce, a Broadcast and a ring shift."""
    import torch
    import nccl_amd
    import oracle
    n = 3
    cs = _comms(n)
    count, nb, ns = 50_001, 300_001, 70_001
    ins = [oracle.fill(7, 77 + r, count) for r in range(n)]
    wb = _payload(nb, 5)
    ws = [_payload(ns, 10 + r) for r in range(n)]
    bufs = {}
    for comm, _ in cs:
        r = comm.rank
        bufs[r] = (torch.from_numpy(ins[r]).cuda(), torch.zeros(count, device="cuda"), Buf(nb, 0, wb if r == 1 else None),
                   Buf(ns, 0, ws[r]), Buf(ns))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for comm, stream in cs:
            r = comm.rank
            x, y, bb, sb, rb = bufs[r]
            comm.allreduce(x, y, nccl_amd.SUM, stream=stream)
            comm.broadcast_raw(bb.ptr, bb.ptr, nb, 1, 1, stream.cuda_stream)
            comm.send_raw(sb.ptr, ns, 1, (r + 1) % n, stream.cuda_stream)
            comm.recv_raw(rb.ptr, ns, 1, (r - 1) % n, stream.cuda_stream)
    errs = []
    want_ar = oracle.all_reduce(ins, 7, 0)
    for comm, stream in cs:
        stream.synchronize()
        r = comm.rank
        if comm.async_error():
            errs.append(f"rank {r}: async error {comm.async_error()}")
            continue
        _, y, bb, sb, rb = bufs[r]
        if not np.array_equal(y.cpu().numpy(), want_ar):
            errs.append(f"mixed group AllReduce rank {r} differs")
        errs += bb.check(wb, f"mixed group Broadcast rank {r}")
        errs += rb.check(ws[(r - 1) % n], f"mixed group ring shift rank {r}")
    errs += p2p_case(cs, ring_shift(n, 1000), 3, 1, "after the mixed group")
    _destroy(cs)
    return errs


def _job_split():
    cs = _comms(5)
    errs = coll_case(cs, "alltoall", 300_001, seed=8)
    errs += coll_case(cs, "alltoall", 4099, seed=9)
    _destroy(cs)
    return errs


JOBS = {"pairs": _job_pairs, "mixed": _job_mixed, "split": _job_split}


def _worker_main(job, env, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
        os.environ.update(env)
        klog = f"/tmp/nccl_amd_p2p_kernels_{os.getpid()}.log"
        dlog = f"/tmp/nccl_amd_p2p_debug_{os.getpid()}.log"
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


# ---------------------------------------------------------------- tests

@pytest.mark.parametrize("extra", [{}, {"NCCL_MAX_P2P_NCHANNELS": "1"}], ids=["channels", "one-channel"])
def test_pair_sizes(built, extra):
    """n = 2, 4 KiB slots, 2 slots, 7 workgroups per launch (so 3 channels per direction; many steps, slot reuse):
    0 .. 4 MiB + 64 bytes as uint8 / fp16 / fp32 / int64 where the size divides, 0 -> 1 and 1 -> 0, source and
    destination misaligned by {0, 1, 3} independently; once more on one channel. Staged kernel only."""
    errs, kernels, _ = _spawn("pairs", dict(TINY_ENV, **extra))
    assert not errs, "\n".join(errs[:20])
    assert any("p2pKernel" in k for k in kernels), kernels
    assert not any("llKernel" in k for k in kernels), kernels
    grids = {int(k.split("grid=")[1].split()[0]) for k in kernels if "p2pKernel" in k}
    # one stream per launch here: one channel up to 128 KiB, three (half of 7 workgroups) for the two large sizes
    assert grids == ({1} if extra else {1, 3}), kernels


def test_exchange(built):
    """Both ranks send and recv 4 MiB + 64 in one group: more than channels x nSlots x slotBytes under the tiny-slot
    env, so credits and acks flow both ways at once."""
    cs = _comms(2, TINY_ENV)
    errs = p2p_case(cs, [(0, 1, BIG), (1, 0, BIG)], 1, 1, "exchange")
    errs += p2p_case(cs, [(1, 0, BIG, 1, 3), (0, 1, BIG, 3, 0)], 2, 1, "exchange misaligned")
    # each rank's recv named on a second stream: the group's p2p work launches on the first, the other is joined to it
    other = {r: _torch().cuda.Stream() for r in range(2)}
    errs += p2p_case(cs, [(0, 1, 300_001), (1, 0, 70_001)], 3, 1, "exchange on two streams", recv_streams=other)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_patterns(built, n):
    """A ring shift, an all-pairs exchange with per-pair sizes 1000 (a + 1) + 7 b bytes, ncclAlltoAll, and ncclGather /
    ncclScatter with every root: at an odd byte count with tiny slots and at 70 001 bytes with default slots."""
    errs = []
    for env, nbytes in ((TINY_ENV, 4099), ({}, 70_001)):
        cs = _comms(n, env)
        seed = 10 * n
        errs += p2p_case(cs, ring_shift(n, nbytes), seed, 1, f"ring n={n}")
        pairs = [(a, b, 1000 * (a + 1) + 7 * b) for a in range(n) for b in range(n) if a != b]
        errs += p2p_case(cs, pairs, seed + 1, 1, f"all pairs n={n}")
        errs += coll_case(cs, "alltoall", nbytes, seed + 2)
        errs += coll_case(cs, "alltoall", (nbytes // 4) * 4, seed + 3, dtype=7)
        for root in range(n):
            errs += coll_case(cs, "gather", nbytes, seed + 4 + root, root)
            errs += coll_case(cs, "scatter", nbytes, seed + 20 + root, root)
        _destroy(cs)
        if errs:
            break
    assert not errs, "\n".join(errs[:20])


def test_several_messages_per_pair(built):
    """One group sends four messages of 5, 0, 300 001 and 16 bytes to the same peer, which receives them into four
    buffers in that order; then with the sender's group split in two (matching across group boundaries)."""
    import torch
    import nccl_amd
    # Four slots: channel 0 carries three slices (5 bytes, the first part of 300 001, 16 bytes), and in the second half
    # the sender's groups must complete before the receiver's group is even issued — one thread drives both ranks, and a
    # group's join on the sender's stream may hold the receiver's fork behind it when the two user streams share a
    # hardware queue (group.cc collFork). With the default two slots the third slice would wait for an ack.
    cs = _comms(2, {"NCCL_AMD_NSLOTS": "4"})
    sizes = (5, 0, 300_001, 16)
    errs = p2p_case(cs, [(0, 1, b) for b in sizes], 1, 1, "four messages")
    (c0, s0), (c1, s1) = cs
    wants = [_payload(b, 70 + k) for k, b in enumerate(sizes)]
    sb = [Buf(b, 0, w) for b, w in zip(sizes, wants)]
    rb = [Buf(b) for b in sizes]
    torch.cuda.synchronize()
    for half in (sb[:2], sb[2:]):
        with nccl_amd.group():
            for b in half:
                c1.send_raw(b.ptr, b.nbytes, 1, 0, s1.cuda_stream)
    with nccl_amd.group():
        for b in rb:
            c0.recv_raw(b.ptr, b.nbytes, 1, 1, s0.cuda_stream)
    plan = [(1, 0, b, w, s, r) for b, w, s, r in zip(sizes, wants, sb, rb)]
    errs += _finish({0: cs[0], 1: cs[1]}, plan, "sender's group split")
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_self_and_one_rank(built):
    """peer == rank inside a group (a local copy) beside a ring shift at n = 3; a one-rank communicator."""
    cs = _comms(3)
    errs = p2p_case(cs, [(1, 1, 70_001)] + ring_shift(3, 4099) + [(2, 2, 16), (0, 0, 0)], 1, 1, "self n=3")
    _destroy(cs)
    cs = _comms(1)
    errs += p2p_case(cs, [(0, 0, 300_001), (0, 0, 5, 1, 3)], 2, 1, "one rank")
    errs += coll_case(cs, "alltoall", 4099, 3)
    errs += coll_case(cs, "gather", 4099, 4)
    errs += coll_case(cs, "scatter", 4099, 5)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("env", CREDIT_ENVS,
                         ids=["ag_pull", "both_pulls", "ag_pull_tiny_slots", "push_tiny_slots", "rs_pull_push"])
def test_credit_sequences_survive(built, env):
    """p2p traffic between ranks 0 and 2 alone (rank 1 issues nothing) and all-pairs traffic, interleaved with
    AllReduce, ReduceScatter, AllGather, Reduce and Broadcast on one communicator under both gathers and both
    scatters: the pairs' RS slots, credits and counters stay in step (the collectives against the oracle)."""
    from tests import gpu_cases as G
    n = 3
    cs = _comms(n, env)
    two = lambda nbytes: ("p2p", [(0, 2, nbytes), (2, 0, nbytes // 2 + 1)])  # noqa: E731
    allp = lambda nbytes: ("p2p", [(a, b, nbytes + 16 * a + b) for a in range(n) for b in range(n) if a != b])  # noqa: E731
    seq = [two(100_003), ("allgather", 7, 0, 70_001, 0), allp(300_001), ("allreduce", 7, 0, 300_001, 0),
           ("reduce", 7, 0, 100_003, 1), two(5), ("broadcast", 300_001 * 4, 2), ("reducescatter", 7, 0, 3 * 40_000, 0),
           allp(4099), ("allreduce", 6, 2, 1_000_003, 0), ("p2p", [(0, 2, 1 << 20)]), ("allgather", 2, 0, 5, 0),
           ("alltoall", 70_001)]
    errs = []
    for rep in range(2):
        for i, op in enumerate(seq):
            if op[0] == "p2p":
                errs += p2p_case(cs, op[1], 100 * rep + i, 1, f"rep {rep} op {i}")
            elif op[0] == "alltoall":
                errs += coll_case(cs, "alltoall", op[1], 100 * rep + i)
            elif op[0] == "broadcast":
                errs += bcast_case(cs, op[1], 1, op[2], "oop" if rep == 0 else "inplace", seed=2000 * rep + i)
            else:
                coll, dt, rop, count, root = op
                errs += G.run_case(cs, coll, dt, rop, count, 0, seed=1000 * rep + i, root=root)
            if errs:
                break
    _destroy(cs)
    assert not errs, "\n".join(errs[:10])


def test_mixed_group(built):
    """One group holds an AllReduce, a Broadcast and a ring shift: all correct, and every rank's p2p launch follows the
    group's collectives."""
    errs, kernels, log = _spawn("mixed", {"NCCL_DEBUG": "TRACE"})
    assert not errs, "\n".join(errs[:20])
    lines = log.splitlines()
    p2p = [i for i, ln in enumerate(lines) if "p2p launch: rank" in ln]
    colls = [i for i, ln in enumerate(lines) if "AllReduce: count" in ln or "Broadcast: count" in ln]
    assert len(colls) == 6, [lines[i] for i in colls]
    first_group = p2p[:3]   # (the ring shift after the mixed group launches three more)
    assert len(p2p) == 6 and sorted({lines[i].split("p2p launch: rank ")[1].split()[0] for i in first_group}) == ["0", "1", "2"]
    assert min(first_group) > max(colls), "a p2p launch precedes a collective of its group"
    assert any("p2pKernel" in k for k in kernels), kernels


def test_round_split(built):
    """n = 5 ncclAlltoAll with 4 workgroups per launch: two channels per stream, so one round per launch and four
    launches per rank at 300 001 bytes, two rounds per launch at 4099."""
    errs, kernels, log = _spawn("split", {"NCCL_MAX_CTAS": "4", "NCCL_DEBUG": "TRACE"})
    assert not errs, "\n".join(errs[:20])
    per_rank = [sum("p2p launch: rank %d " % r in ln for ln in log.splitlines()) for r in range(5)]
    assert per_rank == [4 + 2] * 5, per_rank
    assert all(int(k.split("grid=")[1].split()[0]) <= 4 for k in kernels if "p2pKernel" in k), kernels


def test_graph_capture(built):
    """A send / recv exchange and an ncclAlltoAll captured per rank, replayed three times with new contents."""
    import torch
    import nccl_amd
    cs = _comms(2)
    comms = [c for c, _ in cs]
    streams = [nccl_amd.dedicated_stream(0), nccl_amd.dedicated_stream(0)]
    nb, blk = 300_001, 70_001
    x = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    y = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    a = [torch.zeros(2 * blk, dtype=torch.uint8, device="cuda") for _ in range(2)]
    b = [torch.zeros(2 * blk, dtype=torch.uint8, device="cuda") for _ in range(2)]
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


def _mp_worker(rank, nranks, uid, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(nranks, rank, uid)
        cs = [(comm, torch.cuda.Stream())]
        errs = []
        for i, nbytes in enumerate((1000, 300_001 * 4)):
            errs += p2p_case(cs, ring_shift(nranks, nbytes), 800 + i, 1, "ring")
            errs += coll_case(cs, "alltoall", nbytes, 900 + i)
        comm.destroy()
        q.put((rank, errs))
    except Exception as e:  # report instead of hanging the parent
        q.put((rank, [f"rank {rank} exception: {e!r}"]))


def test_multi_process(built):
    """Four processes on one GPU: a ring shift and an ncclAlltoAll at 1000 bytes and 300 001 x 4 bytes; each process
    checks its own rank."""
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


def test_arguments(built):
    """A peer or root outside 0 .. n-1 is ncclInvalidArgument; a send to self without its recv is ncclInvalidUsage
    from the group end; the communicator then still runs a ring shift."""
    import nccl_amd
    cs = _comms(3)
    (c0, s0) = cs[0]
    b = Buf(4096)
    for peer in (3, -1):
        with pytest.raises(nccl_amd.NcclError) as ei:
            c0.send_raw(b.ptr, 1024, 7, peer, s0.cuda_stream)
        assert ei.value.code == nccl_amd.Result.InvalidArgument
        with pytest.raises(nccl_amd.NcclError) as ei:
            c0.recv_raw(b.ptr, 1024, 7, peer, s0.cuda_stream)
        assert ei.value.code == nccl_amd.Result.InvalidArgument
        with pytest.raises(nccl_amd.NcclError) as ei:
            c0.gather_raw(b.ptr, b.ptr, 16, 7, peer, s0.cuda_stream)
        assert ei.value.code == nccl_amd.Result.InvalidArgument
        with pytest.raises(nccl_amd.NcclError) as ei:
            c0.scatter_raw(b.ptr, b.ptr, 16, 7, peer, s0.cuda_stream)
        assert ei.value.code == nccl_amd.Result.InvalidArgument
    nccl_amd.group_start()
    c0.send_raw(b.ptr, 1024, 7, 0, s0.cuda_stream)          # to itself, no recv in the group
    with pytest.raises(nccl_amd.NcclError) as ei:
        nccl_amd.group_end()
    assert ei.value.code == nccl_amd.Result.InvalidUsage
    errs = p2p_case(cs, ring_shift(3, 4099), 1, 1, "after the refused calls")
    _destroy(cs)
    assert not errs, "\n".join(errs)


def test_group_simulate(built):
    """ncclGroupSimulateEnd accepts p2p ops, launches nothing and prices them: more bytes cost more, and the pairs'
    sequences are where they were (a real exchange afterwards is correct)."""
    import torch
    import nccl_amd
    cs = _comms(2)
    est = []
    for nbytes in (70_001, 64 << 20):
        bufs = [(Buf(nbytes, 0, _payload(nbytes, 40 + r)), Buf(nbytes)) for r in range(2)]
        torch.cuda.synchronize()
        nccl_amd.group_start()
        for (comm, stream), (sb, rb) in zip(cs, bufs):
            comm.send_raw(sb.ptr, nbytes, 1, 1 - comm.rank, stream.cuda_stream)
            comm.recv_raw(rb.ptr, nbytes, 1, 1 - comm.rank, stream.cuda_stream)
        est.append(nccl_amd.group_end(simulate=True).estimated_time)
        torch.cuda.synchronize()
        for r, (_, rb) in enumerate(bufs):   # nothing ran: the recv buffers still hold their fill
            assert bool((rb.store == 0x5A).all()), f"rank {r}: a simulated group wrote its recv buffer"
    assert 0 < est[0] < est[1], est
    assert est[1] > (64 << 20) / 50e9, est   # at least one link's worth of the bytes at the model's 50 GB/s
    errs = p2p_case(cs, [(0, 1, 300_001), (1, 0, 4099)], 5, 1, "after the simulated groups")
    _destroy(cs)
    assert not errs, "\n".join(errs)


def test_python_tensors(built):
    """Communicator.send / recv on torch tensors: a small Linear's weight from rank 0 to rank 1; alltoall on fp16."""
    import torch
    import nccl_amd
    cs = _comms(2)
    (c0, s0), (c1, s1) = cs
    torch.manual_seed(11)
    models = [torch.nn.Linear(37, 19).cuda(), torch.nn.Linear(37, 19).cuda()]
    assert not torch.equal(models[0].weight, models[1].weight)
    ref = models[0].weight.detach().clone()
    src = [torch.randn(2 * 501, device="cuda").half() for _ in range(2)]
    out = [torch.zeros(2 * 501, dtype=torch.float16, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with torch.no_grad():
        c0.send(models[0].weight.data, 1, stream=s0)
        c1.recv(models[1].weight.data, 0, stream=s1)
        with nccl_amd.group():
            c0.alltoall(src[0], out[0], stream=s0)
            c1.alltoall(src[1], out[1], stream=s1)
    torch.cuda.synchronize()
    assert all(c.async_error() == 0 for c, _ in cs)
    assert torch.equal(models[0].weight, ref) and torch.equal(models[1].weight, ref)
    for r in range(2):
        assert torch.equal(out[r], torch.cat([src[i][r * 501:(r + 1) * 501] for i in range(2)]))
    with pytest.raises(ValueError):
        c0.alltoall(src[0][:501], out[0][:501])   # 501 elements are not two equal blocks
    with pytest.raises(ValueError):
        c0.send(src[0][::2], 1)                   # not contiguous
    _destroy(cs)


def test_native_sendrecv_example(built):
    """The C caller of ncclSend / ncclRecv / ncclAlltoAll (tests/native/sendrecv_example.cc) verifies its own output."""
    exe = os.path.join(ROOT, "tests", "native", "sendrecv_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "sendrecv-example"], cwd=ROOT)
    env = dict(os.environ, NCCL_MULTI_RANK_GPU_ENABLE="1", NCCL_AMD_SPIN_TIMEOUT_MS="20000")
    for n in (2, 4):
        out = subprocess.run([exe, str(n)], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
