"""GPU tests of the wide-accumulator fold of the zero-copy kernels (NCCL_AMD_SYM_WIDE_ACC=1, kernels.h foldRangeWide,
DESIGN.md §2.8): fp16 / bf16 / fp8 Sum and Avg on symmetric windows and registered buffers decode to f32, add in f32
in the fold order (ranks owner+1, ..., owner) and round once. The reference is plain torch on the CPU; results must
equal it bit for bit (any NaN code equals any NaN code). All ranks share the one GPU (single process)."""
import os

import numpy as np
import pytest

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
pytestmark = pytest.mark.gpu

WIN, HALF = 4 << 20, 2 << 20  # per-rank window: send at [0, HALF), recv at [HALF, WIN)
SUM, AVG = 0, 4
BATCH = 16384                 # elements a thread block folds per batch: 512 threads x 4 packs x 8 (2-byte) = x 2 x 16 (fp8)


def _tt(dtype):
    import torch
    # torch type, pack elements, max finite (fp8: the clamp), 2^significand bits (big + 1 rounds back to big in T)
    return {6: (torch.float16, 8, None, 2048.0), 9: (torch.bfloat16, 8, None, 256.0),
            10: (torch.float8_e4m3fn, 16, 448.0, 16.0), 11: (torch.float8_e5m2, 16, 57344.0, 8.0)}[dtype]


def _inputs(n, dtype, count, seed):
    """Rank r's input in T: random normal values of magnitude 2^-6 .. 2^6; at the head (block 0, folded in the order
    1, 2, ..., 0) and again at the end: big, 1, 1, ... / a sum beyond +max / beyond -max / one Inf / one NaN."""
    import torch
    T, _, mx, big = _tt(dtype)
    g = torch.Generator().manual_seed(seed)
    top = mx if mx else float(torch.finfo(T).max)
    out = []
    for r in range(n):
        x = torch.exp2(torch.rand(count, generator=g) * 12 - 6) * (torch.randint(0, 2, (count,), generator=g) * 2 - 1)
        fixed = torch.tensor([big if r == 1 else 1.0, top if r else 16.0, -top if r else -16.0,
                              float("inf") if r == 2 and dtype != 10 else 1.0, float("nan") if r == 0 else 1.0])
        x[:5] = fixed[:count]
        if count >= 10:
            x[-5:] = fixed
        out.append(x.to(T))
    return out


def _reference(ins, dtype, op, chunk):
    """Block q = [q * chunk, (q + 1) * chunk) folds in f32 in the order q+1, ..., q; one multiply for avg; fp8 clamps;
    one conversion to T."""
    import torch
    T, _, mx, _ = _tt(dtype)
    n, f = len(ins), [x.to(torch.float32) for x in ins]
    acc = torch.empty_like(f[0])
    for q in range(n):
        s = slice(q * chunk, (q + 1) * chunk)
        a = f[(q + 1) % n][s].clone()
        for k in range(1, n):
            a = f[(q + 1 + k) % n][s] + a
        acc[s] = a
    if op == AVG:
        acc = acc * (torch.tensor(1.0, dtype=torch.float32) / n)
    if mx:
        acc = acc.clamp(-mx, mx)
    return acc.to(T)


def _differ(got, want):
    """Indices where the raw codes differ; any NaN code equals any NaN code."""
    import torch
    gn, wn = got.to(torch.float32).isnan(), want.to(torch.float32).isnan()
    raw = (got.view(torch.uint8).reshape(got.numel(), -1) != want.view(torch.uint8).reshape(got.numel(), -1)).any(1)
    return ((raw & ~(gn & wn)) | (gn != wn)).nonzero().flatten()


def _run(comms, streams, bufs, coll, dtype, op, count, off=0, inplace=False, seed=1):
    """One collective on every rank; `count` = AllReduce elements / ReduceScatter recvcount. Returns error strings."""
    import torch
    import nccl_amd
    T, epp, _, big = _tt(dtype)
    n, es = len(comms), 16 // epp
    total = count * n if coll == "rs" else count
    ins = _inputs(n, dtype, total, seed)
    chunk = count if coll == "rs" else -(-(-(-count // n)) // epp) * epp  # AllReduce block: divUp(count, n) in whole packs
    want = _reference(ins, dtype, op, chunk)
    so, ro = off * es, (off * es if inplace else HALF + off * es)
    for b, x in zip(bufs, ins):
        b[ro:ro + total * es].zero_()
        b[so:so + total * es].copy_(x.view(torch.uint8))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for c, s, b in zip(comms, streams, bufs):
            p = b.data_ptr()
            if coll == "rs":
                c.reduce_scatter_raw(p + so, p + ro, count, dtype, op, s.cuda_stream)
            else:
                c.all_reduce_raw(p + so, p + ro, count, dtype, op, s.cuda_stream)
    errs = []
    for c, s, b in zip(comms, streams, bufs):
        s.synchronize()
        r = c.rank
        exp = want[r * count:(r + 1) * count] if coll == "rs" else want
        got = b[ro:ro + exp.numel() * es].cpu().view(T)
        tag = f"rank {r} {coll} dt {dtype} op {op} count {count} off {off} inplace {inplace}"
        bad = _differ(got, exp)
        if c.async_error() or bad.numel():
            errs.append(f"{tag}: async {c.async_error()}, {bad.numel()} differ, first {bad[:4].tolist()} got "
                        f"{got[bad[:4]].float().tolist()} want {exp[bad[:4]].float().tolist()}")
        # (b) the fixed element: per-hop rounding in T loses every 1 added to `big`, the wide fold keeps them
        if op == SUM and (coll == "ar" or r == 0):
            hop = ins[1][0]
            for k in (*range(2, n), 0):
                hop = (ins[k][0].float() + hop.float()).to(T)
            wide = float(torch.tensor(big + n - 1).to(T))
            if float(hop) != big or float(got[0]) != wide:
                errs.append(f"{tag}: fixed element {float(got[0])}, per-hop fold {float(hop)}, wide {wide}")
    return errs


def _comms(n, monkeypatch, dtype, oneshot=False, register=False):
    import torch
    import nccl_amd
    os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
    monkeypatch.setenv("NCCL_PROTO", "^LL")  # (small messages take LL, which needs no window and stays narrow)
    monkeypatch.setenv("NCCL_AMD_SYM_WIDE_ACC", "1")
    monkeypatch.setenv("NCCL_AMD_SYM_ONESHOT", "1" if oneshot else "0")
    # a channel part of one batch and two packs: counts below put one batch, and a batch plus a ragged rest, on a channel
    monkeypatch.setenv("NCCL_AMD_MIN_CHANNEL_BYTES", str((BATCH + 2 * _tt(dtype)[1]) * 16 // _tt(dtype)[1]))
    torch.cuda.set_device(0)
    comms = nccl_amd.Communicator.init_all([0] * n)
    bufs = [torch.empty(WIN, dtype=torch.uint8, device="cuda") for _ in comms]
    if register:
        hs = [c.register_buffer(b.data_ptr(), WIN) for c, b in zip(comms, bufs)]
    else:
        with nccl_amd.group():
            hs = [c.register_window(b.data_ptr(), WIN) for c, b in zip(comms, bufs)]

    def close():
        for c, h in zip(comms, hs):
            c.deregister_buffer(h) if register else c.deregister_window(h)
        for c in comms:
            c.destroy()
    return comms, [torch.cuda.Stream() for _ in comms], bufs, close


@pytest.mark.parametrize("dtype", [6, 9, 10, 11])
@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("oneshot", [False, True])
def test_wide_fold_equals_f32_reference(built, monkeypatch, n, dtype, oneshot):
    comms, streams, bufs, close = _comms(n, monkeypatch, dtype, oneshot)
    # AllReduce counts: less than a pack; one batch per thread (one channel); two channels of a batch and two packs;
    # that with the last rank's block short by a pack and three elements (a ragged < 16-byte tail)
    span, errs = 2 * BATCH + 4 * _tt(dtype)[1], []
    for op in (SUM, AVG):
        for i, count in enumerate([5, n * BATCH, n * span, n * span - _tt(dtype)[1] - 3]):
            errs += _run(comms, streams, bufs, "ar", dtype, op, count, seed=10 * i + op)  # out of place (one-shot when promised)
            if not oneshot:
                errs += _run(comms, streams, bufs, "ar", dtype, op, count, inplace=True, seed=10 * i + op + 1)
                errs += _run(comms, streams, bufs, "rs", dtype, op, -(-count // n), seed=10 * i + op + 2)
        if not oneshot:  # a window offset of one element: the element-wise path
            errs += _run(comms, streams, bufs, "ar", dtype, op, n * BATCH + 11, off=1, seed=77 + op)
    close()
    assert not errs, "\n".join(errs[:10])


def test_wide_fold_registered_buffers(built, monkeypatch):
    comms, streams, bufs, close = _comms(3, monkeypatch, 9, register=True)
    errs = [e for op in (SUM, AVG) for e in _run(comms, streams, bufs, "ar", 9, op, 3 * (2 * BATCH + 32) - 11, seed=5 + op)]
    close()
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("dtype,op,premul", [(9, 2, None), (2, 0, None), (9, 0, 0x3F00)])
def test_other_ops_keep_the_narrow_fold_under_the_knob(built, monkeypatch, dtype, op, premul):
    """(c) bf16 Max, int32 Sum and a user PreMulSum (bf16, scalar 0.5) on the same windows: the oracle's bits as before."""
    import torch
    import nccl_amd
    import oracle
    from tests import gpu_cases as G
    comms, streams, bufs, close = _comms(3, monkeypatch, 9)
    count, ins = 3 * BATCH + 5, G.make_inputs(3, dtype, 3 * BATCH + 5, 42)
    want = oracle.all_reduce(ins, dtype, op, premul)
    ops = [c.create_pre_mul_sum(premul, dtype) if premul is not None else op for c in comms]
    for b, x in zip(bufs, ins):
        b[:x.nbytes].copy_(torch.from_numpy(x.view(np.uint8).copy()))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for c, s, b, o in zip(comms, streams, bufs, ops):
            c.all_reduce_raw(b.data_ptr(), b.data_ptr() + HALF, count, dtype, o, s.cuda_stream)
    torch.cuda.synchronize()
    ok = [not c.async_error() and G.same_bits(b[HALF:HALF + want.nbytes].cpu().numpy().view(want.dtype), want, dtype)
          for c, b in zip(comms, bufs)]
    close()
    assert all(ok), ok
