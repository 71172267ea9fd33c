"""GPU tests of the device API's reduce-copy family (include/nccl_device_reduce_copy.h): ncclLocal* forms in one
process without a communicator, a user RedOp, the ncclLsa* forms across ranks (in one process on dedicated streams, and
as spawned processes), the in-place AllReduce, a child communicator and a captured graph. The kernels are
tests/native/devapi_rc_kernels.hip (libdevapi_rc_kernels.so, launched through ctypes); expected values come from numpy
(torch on the CPU for bf16), folded in source order with fp32 accumulation and one final rounding for the 2-byte floats,
and are compared bit for bit. Every sweep takes its counts from the header's per-round element count P. The numerics
of the fold on edge values, NaNs and source order are tests/test_gpu_device_rc_edge.py, which drives lsa_case and
inplace_case with its own inputs, reference and comparison."""
import ctypes
import multiprocessing as mp
import os
import queue
import subprocess

import numpy as np

import pytest

from tests.test_gpu_broadcast import FILL, _destroy, _torch
from tests.test_gpu_device_api import (RECV_OFF, SEND_OFF, _cs, _fill, _grouped, _setup, _teardown)

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLIB = os.path.join(ROOT, "tests", "native", "libdevapi_rc_kernels.so")

# name -> (the kernels' type code, element bytes)
TYPES = {"int8": (0, 1), "uint8": (1, 1), "int32": (2, 4), "uint32": (3, 4), "int64": (4, 8), "uint64": (5, 8),
         "float": (6, 4), "double": (7, 8), "half": (8, 2), "bfloat16": (9, 2)}
NP = {"int8": np.int8, "uint8": np.uint8, "int32": np.int32, "uint32": np.uint32, "int64": np.int64,
      "uint64": np.uint64, "float": np.float32, "double": np.float64, "half": np.float16, "bfloat16": np.uint16}
COOPS = ((0, 1), (1, 64), (2, 256))      # (the kernels' coop code, threads of the coop): thread, warp, CTA
NSRC = (1, 2, 3, 4, 5, 8, 16)
NDST = (1, 3)
GUARD = 64

_K = None


def _kernels():
    global _K
    if _K is None:
        import nccl_amd
        nccl_amd.load()
        assert os.path.exists(KLIB), f"{KLIB} missing: make devapi-rc-kernels"
        k = ctypes.CDLL(KLIB)
        P, S, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        k.rc_round_elts.argtypes, k.rc_round_elts.restype = [S, I], S
        k.rc_local.argtypes = [I, I, I, I, P, P, P, S, P, S, I, I, S, P]
        k.rc_max.argtypes = [I, P, I, P, I, S, P]
        k.rc_usersum.argtypes = [I, P, I, P, I, S, P]
        k.rc_lsa.argtypes = [I, P, P, S, P, S, S, I, I, I, P]
        _K = k
    return _K


def _counts(elt, coop_size):
    p = _kernels().rc_round_elts(elt, coop_size)
    assert p == coop_size * (1 if coop_size == 1 else 4) * (16 // elt)      # the header's P, restated
    return sorted({0, 1, 16 // elt - 1, p - 1, p, p + 1, 2 * p + p // 2 + 3})


# ---------------------------------------------------------------- inputs and the expected fold

def _values(kind, n, rng):
    """n elements of `kind` as its numpy type (bfloat16: its bits as uint16): integers over the whole range; floats with
    magnitudes over 1e-3..1e3 and both signs, every 11th or so replaced by +-0, a denormal or +-max. No NaN."""
    dt = NP[kind]
    if kind in ("int8", "uint8", "int32", "uint32", "int64", "uint64"):
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    special = rng.random(n) < 0.09
    pick = rng.integers(0, 6, n)
    if kind == "bfloat16":
        bits = (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        table = np.array([0x0000, 0x8000, 0x0001, 0x807f, 0x7f7f, 0xff7f], dtype=np.uint16)
        return np.where(special, table[pick], bits)
    with np.errstate(over="ignore"):
        v = x.astype(dt)
    fi = np.finfo(dt)
    tiny = fi.smallest_subnormal
    table = np.array([0.0, -0.0, tiny, -3 * tiny, fi.max, -fi.max], dtype=dt)
    v = np.where(special, table[pick], v)
    assert not np.isnan(v).any() and np.isfinite(v).all()
    return v


def _fold(kind, srcs, upto=None):
    """{k: the fold of srcs[0..k) in source order} for every k in `upto` (default: only len(srcs)), as arrays of the
    element type. Integers wrap; float and double round per step; half and bfloat16 accumulate in fp32 and round once."""
    upto = set(upto or [len(srcs)])
    out = {}
    if 1 in upto:
        out[1] = srcs[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "bfloat16":
            import torch
            up = lambda a: torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float()
            acc = up(srcs[0])
            for i in range(1, len(srcs)):
                acc = acc + up(srcs[i])
                if i + 1 in upto:
                    out[i + 1] = acc.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
        elif kind == "half":
            acc = srcs[0].astype(np.float32)
            for i in range(1, len(srcs)):
                acc = acc + srcs[i].astype(np.float32)
                if i + 1 in upto:
                    out[i + 1] = acc.astype(np.float16)
        else:
            acc = srcs[0].copy()
            for i in range(1, len(srcs)):
                acc = (acc + srcs[i]).astype(srcs[0].dtype)
                if i + 1 in upto:
                    out[i + 1] = acc.copy()
    return out


def _align_cases(elt):
    """(source shift, destination shift) in bytes: all 16-byte aligned; all shifted by one element (a common prefix);
    the destinations 4 bytes off the sources (4-byte packs; one element off for 8-byte types: the scalar path); for 1-
    and 2-byte types the destinations one element off (the scalar path)."""
    cases = [(0, 0), (elt, elt), (0, 4 if elt <= 4 else 8)]
    if elt < 4:
        cases.append((0, elt))
    return cases


# ---------------------------------------------------------------- 1. local forms

def _local_sweep(kind, coops, nsrcs):
    """Every local form x alignment case x count x IntCount for the coops and source counts given; error strings."""
    torch = _torch()
    k = _kernels()
    code, elt = TYPES[kind]
    maxcount = max(max(_counts(elt, size)) for _, size in coops)
    displ = (maxcount * elt + 32 + 15) // 16 * 16 // elt                 # elements between two sources / destinations
    rng = np.random.default_rng(1000 + code)
    vals = _values(kind, 16 * displ + 16, rng)
    raw = np.full(GUARD + vals.nbytes + GUARD, FILL, dtype=np.uint8)
    raw[GUARD:GUARD + vals.nbytes] = vals.view(np.uint8)
    src = torch.from_numpy(raw).cuda()
    src_orig = src.clone()
    fill = torch.full((GUARD + 3 * displ * elt + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    dst = fill.clone()
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    flags, what = [], []
    launches = 0
    for sshift, dshift in _align_cases(elt):
        s0 = sshift // elt
        srcs = [vals[s0 + i * displ: s0 + i * displ + maxcount] for i in range(16)]
        want = {n: torch.from_numpy(v.view(np.uint8).copy()).cuda() for n, v in _fold(kind, srcs, nsrcs).items()}
        sbase = src.data_ptr() + GUARD + sshift
        dbase = dst.data_ptr() + GUARD + dshift
        stab = torch.tensor([sbase + i * displ * elt for i in range(16)], dtype=torch.int64, device="cuda")
        dtab = torch.tensor([dbase + i * displ * elt for i in range(3)] + [0] * 13, dtype=torch.int64, device="cuda")
        for coop, size in coops:
            for wide in (0, 1):
                for count in _counts(elt, size):
                    forms = ([(f, n, 1) for f in (0, 1) for n in nsrcs] + [(f, 1, d) for f in (2, 3) for d in NDST]
                             + [(4, n, d) for n in nsrcs for d in NDST])
                    for form, nsrc, ndst in forms:
                        rc = k.rc_local(code, coop, wide, form, stab.data_ptr(), dtab.data_ptr(), sbase, displ, dbase,
                                        displ, nsrc, ndst, count, stream)
                        assert rc == 0, f"launch failed: {rc}"
                        launches += 1
                        expect = fill.clone()
                        for d in range(ndst):
                            at = GUARD + dshift + d * displ * elt
                            expect[at:at + count * elt] = want[nsrc][:count * elt]
                        flags.append((dst == expect).all())
                        what.append(f"{kind} shifts=({sshift},{dshift}) coop={coop} wide={wide} count={count} "
                                    f"form={form} nSrc={nsrc} nDst={ndst}")
                        dst.copy_(fill)
    ok = torch.stack(flags).cpu().numpy()
    bad = [w for w, o in zip(what, ok) if not o]
    if bad:
        bad = [f"{len(bad)} of {launches} cases differ (destinations or the bytes around them)"] + bad
    if not bool((src == src_orig).all()):
        bad.append(f"{kind}: a source was written")
    return bad


@pytest.mark.parametrize("kind", list(TYPES))
def test_local_forms(built, kind):
    errs = _local_sweep(kind, COOPS, NSRC)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("kind", ["int8", "half", "float", "double"])
def test_local_forms_cta_with_partial_wave(built, kind):
    """A CTA of 72 threads: its last wave has 8 lanes, too few to keep 16 pointers one per lane."""
    errs = _local_sweep(kind, ((3, 72),), (1, 2, 5, 16))
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("kind", ["float", "half"])
def test_more_pointers_than_registers(built, kind):
    """17 sources (ncclLocalReduceSum, lambda) and 17 destinations (ncclLocalCopy, lambda): the element-at-a-time loop
    that asks the lambdas again; same fold, same rounding."""
    torch = _torch()
    k = _kernels()
    code, elt = TYPES[kind]
    n = 17
    stream = torch.cuda.current_stream().cuda_stream
    bad = []
    for coop, size in ((0, 1), (2, 256)):
        counts = _counts(elt, size)
        maxcount = max(counts)
        rng = np.random.default_rng(4242 + code + coop)
        srcs = [_values(kind, maxcount, rng) for _ in range(n)]
        dev = [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in srcs]
        want = {m: torch.from_numpy(v.view(np.uint8).copy()).cuda() for m, v in _fold(kind, srcs, (1, n)).items()}
        fill = torch.full((GUARD + maxcount * elt + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        dsts = [fill.clone() for _ in range(n)]
        stab = torch.tensor([d.data_ptr() for d in dev], dtype=torch.int64, device="cuda")
        dtab = torch.tensor([d.data_ptr() + GUARD for d in dsts], dtype=torch.int64, device="cuda")
        for form, nsrc, ndst in ((0, n, 1), (2, 1, n)):
            for count in counts:
                rc = k.rc_local(code, coop, 1, form, stab.data_ptr(), dtab.data_ptr(), dev[0].data_ptr(), 0,
                                dsts[0].data_ptr() + GUARD, 0, nsrc, ndst, count, stream)
                assert rc == 0
                expect = fill.clone()
                expect[GUARD:GUARD + count * elt] = want[nsrc][:count * elt]
                for d in range(n):
                    if not bool((dsts[d] == (expect if d < ndst else fill)).all()):
                        bad.append(f"{kind} coop={coop} form={form} count={count} destination {d}")
                    dsts[d].copy_(fill)
        for d, x in zip(dev, srcs):
            if not bool((d == torch.from_numpy(x.view(np.uint8).copy()).cuda()).all()):
                bad.append(f"{kind} coop={coop}: a source was written")
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------- 2. a user RedOp

@pytest.mark.parametrize("kind", ["int32", "float"])
def test_user_redop_max(built, kind):
    """ncclLsaReduceLsaCopy with a max functor (a < b ? b : a): folded in T, in source order (+-0 tell the order)."""
    torch = _torch()
    k = _kernels()
    code, elt = TYPES[kind]
    counts = _counts(elt, 256)
    maxcount = max(counts)
    rng = np.random.default_rng(77 + code)
    srcs = [_values(kind, maxcount, rng) for _ in range(5)]
    if kind == "float":
        srcs[1][:64] = np.where(np.arange(64) % 2 == 0, 0.0, -0.0)     # zeros of both signs against each other
        srcs[0][:64] = -srcs[1][:64]
    dev = [torch.from_numpy(s.view(np.uint8).copy()).cuda() for s in srcs]
    fill = torch.full((GUARD + maxcount * elt + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    dsts = [fill.clone(), fill.clone()]
    stab = torch.tensor([d.data_ptr() for d in dev], dtype=torch.int64, device="cuda")
    dtab = torch.tensor([d.data_ptr() + GUARD for d in dsts], dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    bad = []
    for nsrc in (1, 2, 5):
        acc = srcs[0].copy()
        for s in srcs[1:nsrc]:
            acc = np.where(acc < s, s, acc)
        want = torch.from_numpy(acc.view(np.uint8).copy()).cuda()
        for ndst in (1, 2):
            for count in counts:
                assert k.rc_max(code, stab.data_ptr(), nsrc, dtab.data_ptr(), ndst, count, stream) == 0
                expect = fill.clone()
                expect[GUARD:GUARD + count * elt] = want[:count * elt]
                for d in range(2):
                    if not bool((dsts[d] == (expect if d < ndst else fill)).all()):
                        bad.append(f"{kind} max nSrc={nsrc} nDst={ndst} count={count} destination {d}")
                    dsts[d].copy_(fill)
    assert not bad, "\n".join(bad[:20])
    assert all(bool((d == torch.from_numpy(s.view(np.uint8).copy()).cuda()).all()) for d, s in zip(dev, srcs))


# ---------------------------------------------------------------- 3. LSA forms across ranks

LSA_KINDS = ("float", "half", "bfloat16", "uint32")
GRIDS = (1, 4)
REDUCE_FORMS, COPY_FORMS, ALLREDUCE_FORMS, TWO_TEAM_FORM = (0, 1, 2, 3, 4), (5, 6, 7, 8, 9), (10, 11, 12, 13, 15), 14
INNER = 2


def _lsa_inputs(kind, count, n, seed):
    return [_values(kind, count, np.random.default_rng(seed * 131 + r)) for r in range(n)]


def _lsa_want(kind, xs, n, form, grid, fold=None):
    """The payload every rank's receive window must hold after `form`; `fold` (kind, sources) -> their sum replaces
    _fold for the forms that reduce all ranks."""
    count = xs[0].size
    if form in COPY_FORMS:
        return np.concatenate(xs)
    if form != TWO_TEAM_FORM:
        return fold(kind, xs) if fold else _fold(kind, xs)[n]
    assert fold is None
    want = np.zeros(count, dtype=xs[0].dtype)
    per = (count + n * grid - 1) // (n * grid)
    for r in range(n):      # part r: the sum over r's run of INNER consecutive ranks
        lo, hi = min(r * grid * per, count), min((r + 1) * grid * per, count)
        run = [xs[p][lo:hi] for p in range(r // INNER * INNER, r // INNER * INNER + INNER)]
        want[lo:hi] = _fold(kind, run)[INNER]
    return want


def _payload(nbytes, off, arr):
    want = np.full(nbytes, FILL, dtype=np.uint8)
    want[off:off + arr.nbytes] = arr.view(np.uint8)
    return want


def _launch(rs, code, swin, soff, rwin, roff, count, form, grid):
    k = _kernels()
    for r in rs:
        rc = k.rc_lsa(code, r.dc.ptr, getattr(r, swin).handle, soff, getattr(r, rwin).handle, roff, count, form, INNER,
                      grid, r.stream.cuda_stream)
        assert rc == 0, f"launch failed: {rc}"
    for r in rs:
        r.stream.synchronize()


def _async_errors(rs, what):
    return [f"rank {r.comm.rank} {what}: async error {r.comm.async_error()}" for r in rs if r.comm.async_error()]


def _check_window(buf, off, want, what, check=None):
    """Errors of a window's buffer against the payload `want` at byte `off`, fill everywhere else: bit for bit, or
    with check(got, want, what) -> errors on the payload's elements and the rest against the fill."""
    if check is None:
        return buf.check(_payload(buf.nbytes, off, want), what)
    raw = buf.store.cpu().numpy()
    lo, hi = buf.lo + off, buf.lo + off + want.nbytes
    errs = check(raw[lo:hi].view(want.dtype), want, what)
    if not (np.all(raw[:lo] == FILL) and np.all(raw[hi:] == FILL)):
        errs.append(f"{what}: bytes outside the payload were written")
    return errs


def lsa_case(rs, n, kind, count, forms, grids, seed, soff=SEND_OFF, roff=RECV_OFF, inputs=None, fold=None, check=None):
    """Every form x grid on one set of inputs; the ranks `rs` of this process, of n in all. Returns error strings.
    inputs: every rank's `count` elements in place of the seeded ones, with fold (kind, sources) -> the expected sum and
    check (got, want, what) -> errors in place of _fold and the bit-for-bit comparison."""
    torch = _torch()
    code, _ = TYPES[kind]
    xs = _lsa_inputs(kind, count, n, seed) if inputs is None else inputs
    assert len(xs) == n and all(x.size == count for x in xs)
    for r in rs:
        _fill(r.send, soff, xs[r.comm.rank])
    errs = []
    for form in forms:
        if form == TWO_TEAM_FORM and n % INNER:
            continue
        for grid in grids:
            for r in rs:
                r.recv.view.fill_(FILL)
            torch.cuda.synchronize()
            _launch(rs, code, "swin", soff, "rwin", roff, count, form, grid)
            what = f"{kind} n={n} count={count} form={form} grid={grid} offsets=({soff},{roff})"
            errs += _async_errors(rs, what)
            want = _lsa_want(kind, xs, n, form, grid, fold)
            for r in rs:
                errs += _check_window(r.recv, roff, want, f"rank {r.comm.rank} {what}", check)
            if errs:
                return errs
    for r in rs:
        errs += r.send.check(_payload(r.send.nbytes, soff, xs[r.comm.rank]), f"rank {r.comm.rank} {kind} send window")
    return errs


def inplace_case(rs, n, kind, count, grid, seed, forms=(10, 13), inputs=None, fold=None, check=None):
    """ncclLsaReduceSumCopy with the send window as source and destination, at one offset; inputs, fold and check as
    in lsa_case."""
    torch = _torch()
    code, _ = TYPES[kind]
    xs = _lsa_inputs(kind, count, n, seed) if inputs is None else inputs
    assert len(xs) == n and all(x.size == count for x in xs)
    errs = []
    for form in forms:
        for r in rs:
            _fill(r.send, SEND_OFF, xs[r.comm.rank])
            r.recv.view.fill_(FILL)
        torch.cuda.synchronize()
        _launch(rs, code, "swin", SEND_OFF, "swin", SEND_OFF, count, form, grid)
        what = f"in place {kind} n={n} count={count} form={form} grid={grid}"
        errs += _async_errors(rs, what)
        want = fold(kind, xs) if fold else _fold(kind, xs)[n]
        for r in rs:
            errs += _check_window(r.send, SEND_OFF, want, f"rank {r.comm.rank} {what}", check)
            errs += r.recv.check(np.full(r.recv.nbytes, FILL, dtype=np.uint8), f"rank {r.comm.rank} {what}: recv window")
    return errs


def lsa_matrix(cs, n):
    """All forms x grids x types x counts at the usual offsets; the 4-byte-relative offsets once per type; in place."""
    maxcount = max(_counts(2, 256))
    rs = _setup(cs, n * maxcount * 4, max(GRIDS))
    errs, seed = [], 0
    every = REDUCE_FORMS + COPY_FORMS + ALLREDUCE_FORMS + (TWO_TEAM_FORM,)
    for kind in LSA_KINDS:
        counts = _counts(TYPES[kind][1], 256)
        for count in counts:
            seed += 1
            errs += lsa_case(rs, n, kind, count, every, GRIDS, seed)
            if errs:
                break
        # the send payload 4 bytes into the window against 32: 4-byte packs for the 2-byte types, the scalar loop else
        for count in counts:
            seed += 1
            errs += lsa_case(rs, n, kind, count, (1, 6, 10), (4,), seed, soff=4, roff=32)
        if kind in ("float", "bfloat16"):
            for count in counts:
                for grid in GRIDS:
                    seed += 1
                    errs += inplace_case(rs, n, kind, count, grid, seed)
        if errs:
            break
    _teardown(rs, destroy_comms=False)
    return errs


def graph_case(cs, n):
    """The float AllReduce kernel (form 10) captured once and replayed 3 times with fresh inputs; one rank per process."""
    torch = _torch()
    k = _kernels()
    code, elt = TYPES["float"]
    count, grid = max(_counts(elt, 256)), 4
    rs = _setup(cs, 4 * count, grid)
    (r,) = rs
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    xs = _lsa_inputs("float", count, n, 900)
    _fill(r.send, SEND_OFF, xs[r.comm.rank])
    r.recv.view.fill_(FILL)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        rc = k.rc_lsa(code, r.dc.ptr, r.swin.handle, SEND_OFF, r.rwin.handle, RECV_OFF, count, 10, INNER, grid,
                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    errs = []
    for rep in range(3):
        xs = _lsa_inputs("float", count, n, 901 + rep)
        _fill(r.send, SEND_OFF, xs[r.comm.rank])
        r.recv.view.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        errs += r.recv.check(_payload(r.recv.nbytes, RECV_OFF, _fold("float", xs)[n]),
                             f"rank {r.comm.rank} graph replay {rep}")
    errs += _async_errors(rs, "graph replay")
    del g
    _teardown(rs, destroy_comms=False)
    return errs


# ---------------------------------------------------------------- spawned ranks (one process each)

RANK_JOBS = {"lsa": lsa_matrix, "graph": graph_case}


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


def _spawned(nranks, jobs):
    """Run `jobs` on nranks spawned processes; {job: error strings of every rank}."""
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
    return {job: [e for r in sorted(results) for e in results[r][job]] for job in jobs}


@pytest.mark.parametrize("n", [2, 3, 4])
def test_lsa_forms_in_process(built, n):
    cs = _cs(n)
    errs = lsa_matrix(cs, n)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


def test_lsa_forms_spawned_8(built):
    errs = _spawned(8, ("lsa",))["lsa"]
    assert not errs, "\n".join(errs[:20])


def test_child_communicator(built):
    """2 of 4 ranks: each pair of an ncclCommSplit runs the float AllReduce on its own DevComm."""
    import nccl_amd
    cs = _cs(4)
    with nccl_amd.group():
        kids = [c.split(c.rank // 2, c.rank) for c, _ in cs]
    flat = [(kids[i], cs[i][1]) for i in range(4)]
    count = max(_counts(4, 256))
    rs = _setup(flat, 2 * count * 4, 4)
    errs = []
    for i, pair in enumerate((rs[:2], rs[2:])):
        errs += lsa_case(pair, 2, "float", count, (10, 12), (4,), 600 + i)
    _teardown(rs)
    _destroy(cs)
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 4. graph replay

def test_graph_replay_spawned(built):
    errs = _spawned(2, ("graph",))["graph"]
    assert not errs, "\n".join(errs[:20])


# ---------------------------------------------------------------- 5. the native example

@pytest.mark.parametrize("n", [2, 4])
def test_native_rc_example(built, n):
    """tests/native/devapi_rc_example: the AllReduce written with ncclLsaReduceSumCopy, send -> recv and in place."""
    exe = os.path.join(ROOT, "tests", "native", "devapi_rc_example")
    assert os.path.exists(exe), f"{exe} missing: make devapi-rc-example"
    env = dict(os.environ, NCCL_AMD_SPIN_TIMEOUT_MS="30000")
    r = subprocess.run([exe, str(n)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and f"OK n={n}" in r.stdout, r.stdout + r.stderr
