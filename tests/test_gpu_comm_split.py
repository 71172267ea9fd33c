"""GPU tests of ncclCommSplit / ncclCommShrink: no kernel is new, so what is tested is that every
existing kernel runs on communicators whose rank numbering, peer table, slot size and channel cap differ from their
parent's, side by side with their siblings. Every result is compared bit for bit with the oracle (reductions, folded in
CHILD rank order) or with numpy slicing (everything that only moves bytes).

Ranks share the box's one GPU: in one process (ncclCommInitAll on a repeated device, one thread splitting every
communicator of the clique inside a group) under the tiny-slot environment of tests/test_gpu_p2p.py (4 KiB slots, 2
slots, 7 channels), or as four spawned processes over ncclCommInitRank. Sizes: one element; 4099 bytes (the LL path;
4100 for fp32); 300 KiB + 4 bytes (the staged path, many slot reuses at 4 KiB). At most 8 communicators that share the
GPU are alive in the process at any time."""
import contextlib
import ctypes
import multiprocessing as mp
import os
import queue

import numpy as np

import pytest

from tests import gpu_cases as G
from tests.test_gpu_broadcast import Buf, _comms, _destroy, _payload, _torch, bcast_case
from tests.test_gpu_p2p import TINY_ENV, coll_case, p2p_case

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu

BYTES = (4, 4099, (300 << 10) + 4)
COUNTS = (1, 1025, (300 << 10) // 4 + 1)   # the same sizes in whole fp32 elements


@contextlib.contextmanager
def _env(env):
    """A child reads the environment's knobs when it is created, like any communicator."""
    env = dict(env, NCCL_MULTI_RANK_GPU_ENABLE="1")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _split(cs, colors, keys, env=TINY_ENV):
    """One thread splits every communicator of the clique inside one group. Returns {color: [(child, stream), ...] in
    child rank order} (each child on its parent rank's stream) and the children in parent rank order (None: NOCOLOR)."""
    import nccl_amd
    with _env(env):
        with nccl_amd.group():
            kids = [c.split(colors[c.rank], keys[c.rank]) for c, _ in cs]
    out = {}
    for (c, s), k in zip(cs, kids):
        assert (k is None) == (colors[c.rank] == nccl_amd.SPLIT_NOCOLOR)
        if k is not None:
            assert k.ptr, "the child's handle is filled in when the group ends"
            out.setdefault(colors[c.rank], []).append((k, s))
    for color in out:
        out[color].sort(key=lambda ks: ks[0].rank)
    return out, kids


def _shrink(cs, exclude, flags=0, env=TINY_ENV):
    """The ranks that are not excluded call ncclCommShrink in one group; [(child, stream), ...] in child rank order."""
    import nccl_amd
    with _env(env):
        with nccl_amd.group():
            kids = [(c.shrink(exclude, flags), s) for c, s in cs if c.rank not in exclude]
    assert all(k.ptr for k, _ in kids)
    return sorted(kids, key=lambda ks: ks[0].rank)


def _members(colors, keys, color):
    """The reference's rule (src/init.cc:1789-1799): ascending key, ties by parent rank."""
    return sorted((r for r in range(len(colors)) if colors[r] == color), key=lambda r: (keys[r], r))


def _check_numbering(cs, kids, colors, keys):
    for (c, _), k in zip(cs, kids):
        if k is None:
            continue
        mem = _members(colors, keys, colors[c.rank])
        assert (k.nranks, k.rank, k.device) == (len(mem), mem.index(c.rank), c.device), (c.rank, k.nranks, k.rank)


def _six_ops(cs, nbytes, seed):
    """AllReduce, AllGather and ReduceScatter (fp32 sum), a Broadcast from child root 1, an AlltoAll and a send / recv
    pair between child ranks 0 and 1 on the local ranks `cs` of one communicator. Returns (issue, check): issue is a
    list of calls, op by op and rank by rank, to be made inside a group; check() returns error strings."""
    n = cs[0][0].nranks
    cnt = max(1, nbytes // 4)
    root = min(1, n - 1)
    issue, checks = [], []
    tag = f"n={n} bytes={nbytes} seed={seed}"
    for coll, count in (("allreduce", cnt), ("allgather", cnt), ("reducescatter", max(1, cnt // n) * n)):
        ins = G.make_inputs(n, 7, count, seed)
        exp = G.expected(coll, ins, 7, 0)
        for c, s in cs:
            keep, sv = G.to_device(ins[c.rank], "cuda:0")
            keep2, rv = G.to_device(np.zeros(G.out_count(coll, n, count), np.float32), "cuda:0")
            issue.append(lambda c=c, s=s, sv=sv, rv=rv, coll=coll, count=count:
                         G.launch(c, coll, sv, rv, count, 7, 0, 0, s.cuda_stream))
            checks.append(lambda rv=rv, want=exp[c.rank], what=f"rank {c.rank} {coll} {tag}", keep=(keep, keep2):
                          [] if G.same_bits(G.from_device(rv, np.float32), want, 7) else [what + " differs"])
    want_b = _payload(nbytes, seed + 1)
    for c, s in cs:
        b = Buf(nbytes, 0, want_b if c.rank == root else None)
        issue.append(lambda c=c, s=s, b=b: c.broadcast_raw(b.ptr, b.ptr, nbytes, 1, root, s.cuda_stream))
        checks.append(lambda b=b, what=f"rank {c.rank} broadcast {tag}": b.check(want_b, what))
    a2a = [_payload(n * nbytes, seed * 100 + 2 + r) for r in range(n)]
    for c, s in cs:
        r = c.rank
        sb, rb = Buf(n * nbytes, 0, a2a[r]), Buf(n * nbytes)
        want = np.concatenate([a2a[i][r * nbytes:(r + 1) * nbytes] for i in range(n)])
        issue.append(lambda c=c, s=s, sb=sb, rb=rb: c.alltoall_raw(sb.ptr, rb.ptr, nbytes, 1, s.cuda_stream))
        checks.append(lambda rb=rb, want=want, what=f"rank {r} alltoall {tag}": rb.check(want, what))
    if n >= 2:
        pair = [_payload(nbytes, seed * 100 + 50 + r) for r in range(2)]
        for c, s in cs:
            r = c.rank
            if r > 1:
                continue
            sb, rb = Buf(nbytes, 0, pair[r]), Buf(nbytes)
            issue.append(lambda c=c, s=s, sb=sb, r=r: c.send_raw(sb.ptr, nbytes, 1, 1 - r, s.cuda_stream))
            issue.append(lambda c=c, s=s, rb=rb, r=r: c.recv_raw(rb.ptr, nbytes, 1, 1 - r, s.cuda_stream))
            checks.append(lambda rb=rb, want=pair[1 - r], what=f"rank {r} recv {tag}": rb.check(want, what))
    return issue, lambda: [e for f in checks for e in f()]


def _together(groups, nbytes, seed):
    """The six operations on several communicators at once: every call of every communicator in ONE group."""
    torch = _torch()
    import nccl_amd
    plans = [_six_ops(cs, nbytes, seed + 7 * i) for i, cs in enumerate(groups)]
    torch.cuda.synchronize()
    with nccl_amd.group():
        for issue, _ in plans:
            for call in issue:
                call()
    errs = []
    for cs in groups:
        for c, s in cs:
            s.synchronize()
            if c.async_error():
                errs.append(f"child rank {c.rank} of {c.nranks}: async error {c.async_error()}")
    if errs:
        return errs
    return [e for _, check in plans for e in check()]


def _order_sensitive(n, count, perm, seed):
    """fp32 inputs in child rank order whose sum folded in child order differs, in at least one element, from the fold
    with the ranks in `perm` order (perm[p] = the child rank held by the p-th member in PARENT order): the seed is
    chosen on the CPU, before anything runs, so that the GPU result can tell the two orders apart. The oracle's fill
    gives multiples of 2^-23 below 1, whose sums of three are exact in any order, so rank r's values are scaled by
    1 + 0.37 r: the partial sums then round."""
    import oracle
    for s in range(seed, seed + 2000):
        ins = [(x * np.float32(1 + 0.37 * r)).astype(np.float32) for r, x in enumerate(G.make_inputs(n, 7, count, s))]
        child = oracle.all_reduce(ins, 7, 0)
        parent = oracle.all_reduce([ins[q] for q in perm], 7, 0)
        if not np.array_equal(child.view(np.uint32), parent.view(np.uint32)):
            return ins, s
    raise AssertionError(f"no seed tells child order from parent order at n={n} count={count}")


# ---------------------------------------------------------------- 1. numbering

def test_numbering_and_concurrent_children(built):
    """Parent n = 4, colour r % 2, key -r: two children of 2, each numbered against its parent's order, both running
    all six operations at once at the three sizes."""
    cs = _comms(4, TINY_ENV)
    colors, keys = [r % 2 for r in range(4)], [-r for r in range(4)]
    groups, kids = _split(cs, colors, keys)
    _check_numbering(cs, kids, colors, keys)
    assert [k.rank for k in kids] == [1, 1, 0, 0] and all(k.nranks == 2 for k in kids)
    # each child owns its memory: its own staging slab, sized for its own rank count (same slot size here)
    assert 0 < kids[0].mem_stats() < cs[0][0].mem_stats()
    errs = []
    for i, nbytes in enumerate(BYTES):
        errs += _together([groups[0], groups[1]], nbytes, 100 + i)
    for g in groups.values():
        _destroy(g)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 2. fold order

@pytest.mark.parametrize("colors,keys", [((0, 0, 0, 0), (0, -1, -2, -3)), ((0, 0, 0, 1), (2, 0, 1, 0))])
def test_fold_order_is_the_childs(built, colors, keys):
    """A child of 4 in reversed order, and a child of 3 in rotated order (parent ranks 1, 2, 0) beside a child of 1: an
    fp32 sum must be folded in child rank order. The inputs are picked so that parent order gives another result. (The
    3-rank child is rotated, not reversed: a reversal of three ranks swaps the two ends and keeps the middle, and the one
    element of the smallest size is folded as (end + end) + middle, which commutes — no input could tell the orders
    apart there.)"""
    cs = _comms(4, TINY_ENV)
    groups, kids = _split(cs, list(colors), list(keys))
    _check_numbering(cs, kids, list(colors), list(keys))
    errs = []
    for color, g in groups.items():
        n = g[0][0].nranks
        mem = _members(colors, keys, color)                # parent ranks in child order
        perm = [mem.index(p) for p in sorted(mem)]         # child rank of each member, in parent order
        for i, count in enumerate(COUNTS):
            if n >= 3:
                ins, seed = _order_sensitive(n, count, perm, 1000 * (i + 1))
            else:
                ins, seed = G.make_inputs(n, 7, count, 77 + i), 77 + i
            errs += G.run_case(g, "allreduce", 7, 0, count, 0, seed, inputs=ins)
    for g in groups.values():
        _destroy(g)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 3. NOCOLOR

def test_nocolor(built):
    import nccl_amd
    cs = _comms(4, TINY_ENV)
    colors, keys = [0, 0, 0, nccl_amd.SPLIT_NOCOLOR], [0, 0, 0, 0]
    groups, kids = _split(cs, colors, keys)
    assert kids[3] is None and list(groups) == [0]
    _check_numbering(cs, kids, colors, keys)
    g = groups[0]
    assert [k.rank for k, _ in g] == [0, 1, 2] and g[0][0].nranks == 3
    errs = []
    for i, (nbytes, count) in enumerate(zip(BYTES, COUNTS)):
        errs += G.run_case(g, "allreduce", 7, 0, count, 0, seed=30 + i)
        errs += bcast_case(g, nbytes, 1, 2, "oop", seed=40 + i)
    errs += G.run_case(cs, "allreduce", 7, 0, COUNTS[1], 0, seed=50)   # the parent, rank 3 included, is as it was
    _destroy(g)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 4. coexistence and lifetime

def test_parent_and_children_coexist_then_outlive(built):
    """Parent, children and parent again on the same streams; then the parent is destroyed first and the children go
    on; then they are destroyed."""
    cs = _comms(4, TINY_ENV)
    colors, keys = [0, 1, 1, 0], [0, 0, 0, 0]
    groups, kids = _split(cs, colors, keys)
    _check_numbering(cs, kids, colors, keys)
    errs = []
    for i, (nbytes, count) in enumerate(zip(BYTES, COUNTS)):
        errs += G.run_case(cs, "allreduce", 7, 0, count, 0, seed=60 + i)
        errs += _together([groups[0], groups[1]], nbytes, 200 + i)
        errs += G.run_case(cs, "reducescatter", 7, 0, 4 * count, 0, seed=70 + i)
        errs += p2p_case(cs, [(0, 3, nbytes), (2, 1, nbytes)], 80 + i, 1, "parent after its children")
    _destroy(cs)
    for i, nbytes in enumerate(BYTES):
        errs += _together([groups[1], groups[0]], nbytes, 300 + i)
        errs += coll_case(groups[0], "gather", nbytes, 90 + i, root=1)
        errs += coll_case(groups[1], "scatter", nbytes, 95 + i, root=0)
    for g in groups.values():
        _destroy(g)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 5. grandchildren

def test_grandchildren(built):
    """A reversed child of 4 split again 2 + 2: the grandchildren, siblings on one GPU, run at once — the channel cap
    they inherited through two generations is the 4-ranks-per-GPU one (8 communicators alive: the child and they)."""
    cs = _comms(4, TINY_ENV)
    groups, kids = _split(cs, [0] * 4, [-r for r in range(4)])
    child = groups[0]
    assert [k.rank for k in kids] == [3, 2, 1, 0]
    _destroy(cs)
    colors, keys = [r // 2 for r in range(4)], [-r for r in range(4)]   # by child rank
    grand, gk = _split(child, colors, keys)
    _check_numbering(child, gk, colors, keys)
    errs = []
    for i, nbytes in enumerate(BYTES):
        errs += _together([grand[0], grand[1]], nbytes, 400 + i)
    errs += G.run_case(child, "allreduce", 7, 0, COUNTS[2], 0, seed=99)
    for g in grand.values():
        _destroy(g)
    _destroy(child)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 6. every path on a child of 3

def test_every_path_on_a_child_of_three(built):
    """The quick case list (every collective, type and operator), a symmetric window registered on the child with a
    zero-copy AllReduce and AlltoAll, a put / signal / wait phase, and a captured AllReduce replayed twice."""
    torch = _torch()
    import nccl_amd
    from tests.test_gpu_rma import Arenas, rma_phase
    from tests.test_gpu_sym_alltoall import Rank, run_case as a2a_case
    from tests.test_gpu_windows import _run as win_case
    cs = _comms(4, TINY_ENV)
    groups, kids = _split(cs, [0, 0, 0, nccl_amd.SPLIT_NOCOLOR], [-r for r in range(4)])
    _destroy(cs)
    g = groups[0]
    assert [k.rank for k in kids[:3]] == [2, 1, 0]
    errs = []
    for i, (coll, dtype, op, count, mis) in enumerate(G.case_list(3, quick=True)):
        errs += G.run_case(g, coll, dtype, op, count, mis, seed=500 + i)
        if len(errs) > 10:
            break
    # a symmetric window on the child: zero-copy AllReduce and AlltoAll
    ranks = [Rank(c, s) for c, s in g]
    with nccl_amd.group():
        for rk in ranks:
            rk.handle = rk.comm.register_window(rk.win.data_ptr(), rk.win.numel(), nccl_amd.WIN_COLL_SYMMETRIC)
    assert all(rk.handle.handle for rk in ranks)
    bases = [(rk.win, rk.win.data_ptr()) for rk in ranks]
    for i, count in enumerate(COUNTS):
        errs += win_case(g, bases, "allreduce", 7, 0, count, 0, False, seed=600 + i)
        errs += a2a_case(ranks, "alltoall", 7, count, seed=610 + i)
    for rk in ranks:
        rk.comm.deregister_window(rk.handle)
    # put / signal / wait
    ar = Arenas(g, 1 << 20, 1 << 20)
    for i, nbytes in enumerate(BYTES):
        errs += rma_phase(ar, [(0, 1, nbytes, 0, 0), (1, 2, nbytes, 1, 16), (2, 0, nbytes, 3, 5), (2, 1, 4, 0, nbytes + 64)],
                          700 + i, "child of 3", signals=[(0, 2)])
    ar.release()
    # one capture per rank, replayed twice
    comms = [c for c, _ in g]
    streams = [nccl_amd.dedicated_stream(0) for _ in comms]
    count = COUNTS[2]
    x = [torch.empty(count, device="cuda") for _ in comms]
    y = [torch.empty(count, device="cuda") for _ in comms]
    graphs = [torch.cuda.CUDAGraph() for _ in comms]
    torch.cuda.synchronize()
    for r, c in enumerate(comms):
        with torch.cuda.graph(graphs[r], stream=streams[r]):
            c.all_reduce_raw(x[r].data_ptr(), y[r].data_ptr(), count, 7, 0, streams[r].cuda_stream)
    for it in range(2):
        ins = G.make_inputs(3, 7, count, 800 + it)
        for r, c in enumerate(comms):
            x[r].copy_(torch.from_numpy(ins[c.rank]))
        torch.cuda.synchronize()
        for r in range(3):
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        torch.cuda.synchronize()
        want = G.expected("allreduce", ins, 7, 0)[0]
        for r, c in enumerate(comms):
            if c.async_error():
                errs.append(f"replay {it} rank {c.rank}: async error {c.async_error()}")
            elif not G.same_bits(y[r].cpu().numpy(), want, 7):
                errs.append(f"replay {it} rank {c.rank} differs")
    del graphs
    _destroy(g)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 7. shrink in one process

def test_shrink(built):
    """n = 4 without rank 2, then a fresh parent without ranks 3 and 1 (listed unsorted), then NCCL_SHRINK_ABORT on an
    idle parent: the mapping (parent order, the excluded removed), the collectives, and the parent left as it was."""
    import nccl_amd
    errs = []
    for exclude, flags in (([2], nccl_amd.SHRINK_DEFAULT), ([3, 1], nccl_amd.SHRINK_DEFAULT), ([1], nccl_amd.SHRINK_ABORT)):
        cs = _comms(4, TINY_ENV)
        g = _shrink(cs, exclude, flags)
        kept = [r for r in range(4) if r not in exclude]
        assert [k.rank for k, _ in g] == list(range(len(kept))) and all(k.nranks == len(kept) for k, _ in g)
        # the child on parent rank p's stream is child rank kept.index(p)
        for (c, s) in cs:
            if c.rank in kept:
                mine = [k for k, ks in g if ks is s]
                assert len(mine) == 1 and mine[0].rank == kept.index(c.rank) and mine[0].device == c.device
        assert all(c.async_error() == 0 for c, _ in cs), "the parent's async error stays at success"
        for i, (nbytes, count) in enumerate(zip(BYTES, COUNTS)):
            n = len(kept)
            perm = [2, 0, 1]   # any order that is no reversal (test_fold_order_is_the_childs)
            ins = _order_sensitive(n, count, perm, 2000 + 100 * i)[0] if n >= 3 else G.make_inputs(n, 7, count, 21 + i)
            errs += G.run_case(g, "allreduce", 7, 0, count, 0, 0, inputs=ins)
            errs += bcast_case(g, nbytes, 1, len(kept) - 1, "bcast", seed=900 + i)
            errs += p2p_case(g, [(0, len(kept) - 1, nbytes), (len(kept) - 1, 0, nbytes)], 910 + i, 1, f"shrink {exclude}")
        errs += G.run_case(cs, "allreduce", 7, 0, COUNTS[2], 0, seed=920)   # the parent still works, all 4 ranks
        assert all(c.async_error() == 0 for c, _ in cs)
        _destroy(g)
        _destroy(cs)
        if errs:
            break
    assert not errs, "\n".join(errs[:20])


def test_arguments(built):
    """The checks before any rendezvous, on a real communicator: a NULL newcomm, the shrink list, the config."""
    import nccl_amd
    lib = nccl_amd.load()
    cs = _comms(2, TINY_ENV)
    c = cs[0][0]
    P, I = ctypes.c_void_p, ctypes.c_int
    out = P(0x1234)
    assert lib.ncclCommSplit(c.ptr, 0, 0, None, None) == 4
    assert lib.ncclCommShrink(c.ptr, (I * 1)(1), 1, None, None, 0) == 4
    assert lib.ncclCommShrink(c.ptr, None, 1, ctypes.byref(out), None, 0) == 4          # no list
    assert lib.ncclCommShrink(c.ptr, (I * 1)(1), 0, ctypes.byref(out), None, 0) == 4    # count <= 0
    assert lib.ncclCommShrink(c.ptr, (I * 1)(2), 1, ctypes.byref(out), None, 0) == 4    # outside [0, nRanks)
    assert lib.ncclCommShrink(c.ptr, (I * 1)(-1), 1, ctypes.byref(out), None, 0) == 4
    assert lib.ncclCommShrink(c.ptr, (I * 1)(0), 1, ctypes.byref(out), None, 0) == 4    # the caller itself
    bad = nccl_amd.Config.default()
    bad.magic = 0
    assert lib.ncclCommSplit(c.ptr, 0, 0, ctypes.byref(out), ctypes.byref(bad)) == 4
    assert out.value == 0x1234, "newcomm is untouched by a call that fails its checks"
    # a child of one rank is legal, and a given config applies to it
    with _env(TINY_ENV):
        with nccl_amd.group():
            kids = [k.split(k.rank, 0, nccl_amd.Config.default(maxCTAs=3, commName="solo")) for k, _ in cs]
    assert all(k.nranks == 1 and k.rank == 0 for k in kids)
    errs = []
    for k, (_, s) in zip(kids, cs):
        errs += G.run_case([(k, s)], "allreduce", 7, 0, COUNTS[1], 0, seed=5)
    errs += G.run_case(cs, "allreduce", 7, 0, COUNTS[1], 0, seed=6)
    for k in kids:
        k.destroy()
    _destroy(cs)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------- 8. four processes

def _mp_worker(rank, nranks, uid, q, finish):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ.update(TINY_ENV)   # 300 KiB on 4 KiB slots: the staged path
        import torch
        import nccl_amd
        torch.cuda.set_device(0)
        comm = nccl_amd.Communicator.init(nranks, rank, uid)
        s = torch.cuda.Stream()
        errs = []
        # 2 + 2 with reversed keys: parent ranks (2, 0) and (3, 1)
        color = rank % 2
        kid = comm.split(color, -rank)
        if (kid.nranks, kid.rank) != (2, 0 if rank >= 2 else 1):
            errs.append(f"rank {rank}: child rank {kid.rank} of {kid.nranks}")
        g = [(kid, s)]
        errs += G.run_case(g, "allreduce", 7, 0, COUNTS[1], 0, seed=10 + color)
        errs += G.run_case(g, "allreduce", 7, 0, COUNTS[2], 0, seed=20 + color)
        errs += bcast_case(g, BYTES[2], 1, 1, "oop", seed=30 + color)
        errs += p2p_case(g, [(0, 1, BYTES[1]), (1, 0, BYTES[2])], 40 + color, 1, "split child")
        kid.destroy()
        # shrink without rank 1, which stays alive and idle
        if rank != 1:
            kid = comm.shrink([1])
            kept = [0, 2, 3]
            if (kid.nranks, kid.rank) != (3, kept.index(rank)):
                errs.append(f"rank {rank}: shrunk rank {kid.rank} of {kid.nranks}")
            for i, count in enumerate(COUNTS):
                ins, seed = _order_sensitive(3, count, [2, 0, 1], 1000 * (i + 1))
                errs += G.run_case([(kid, s)], "allreduce", 7, 0, count, 0, seed, inputs=ins)
            kid.destroy()
        q.put((rank, errs))
        finish.wait(timeout=240)   # rank 1 (and everyone) keeps its parent until every rank has reported
        comm.destroy()
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"rank {rank} exception: {e!r}\n{traceback.format_exc()}"]))


def test_multi_process(built):
    """Four processes on the one GPU over ncclCommInitRank: ncclCommSplit 2 + 2 with reversed keys (an LL and a staged
    AllReduce, a Broadcast, a send / recv pair), then ncclCommShrink without rank 1 and the order-sensitive fp32
    AllReduce on the 3-rank child. Each process checks its own rank; the root thread lives in this process."""
    _torch()
    import nccl_amd
    nranks = 4
    uid = nccl_amd.get_unique_id()
    ctx = mp.get_context("spawn")
    q, finish = ctx.Queue(), ctx.Event()
    ps = [ctx.Process(target=_mp_worker, args=(r, nranks, uid, q, finish)) for r in range(nranks)]
    for p in ps:
        p.start()
    results = {}
    try:
        while len(results) < nranks:
            r, errs = q.get(timeout=240)
            results[r] = errs
    except queue.Empty:
        pass
    finish.set()
    for p in ps:
        if p.is_alive() and len(results) < nranks:
            p.kill()
        p.join(timeout=60)
    assert len(results) == nranks, f"only {len(results)} of {nranks} ranks reported"
    bad = [e for r in sorted(results) for e in results[r]]
    assert not bad, "\n".join(bad[:20])
