"""GPU tests of the bf16 wire of the fp32 direct plan (NCCL_AMD_WIRE_BF16=1): an fp32 Sum / Avg
AllReduce or ReduceScatter rounds every contribution to bf16 once, adds the n rounded values in f32, multiplies an Avg
once by float32(1 / n); ReduceScatter stores that f32 value, AllReduce rounds it once to bf16 and stores it widened on
every rank. The reference is plain torch on the CPU, bit for bit (any NaN code equals any NaN code): the inputs'
rounded contributions are multiples of 2^-13 below 2^7, so their sum is exact in f32 in any order (asserted in
_reference). All ranks share the one GPU (single process); geometry: 4096-byte slots, 2 slots, 3 channels."""
import pytest

from tests import gpu_cases as G
from tests.test_gpu_sym_wide import AVG, SUM, _differ
from tests.test_gpu_wide_staged import HALF, _comms

pytestmark = pytest.mark.gpu

F32 = 7
BLOCK = 3 * 3 * (4096 // 2)  # a rank block of 3 channels x 3 steps of a slot at the wire's slice: slotBytes / 2 elements


def _inputs(n, count, seed):
    """Per rank `count` fp32 values: random signs and mantissas, magnitudes in [2^-6, 2^6). At both ends (where they
    fit) the edge elements: +0 and -0 on every rank, +inf, -inf and a NaN on one rank each, the largest finite fp32
    (it rounds to inf) on rank 0 over zeros."""
    import torch
    g = torch.Generator().manual_seed(seed)
    r = lambda hi: torch.randint(0, hi, (n, count), generator=g, dtype=torch.int64)
    x = ((r(2) << 31) | ((121 + r(12)) << 23) | r(1 << 23)).to(torch.int32).view(torch.float32)
    edges = [[0.0] * n, [-0.0] * n, [float("inf")], [None, float("-inf")], [None] * (n - 1) + [float("nan")],
             [torch.finfo(torch.float32).max] + [0.0] * (n - 1)]
    for base in {0, max(0, count - len(edges))}:
        for k, col in enumerate(edges):
            for rank, v in enumerate(col):
                if base + k < count and v is not None:
                    x[rank, base + k] = v
    return list(x)


def _reference(ins, op, allreduce):
    import torch
    s = ins[0].to(torch.bfloat16).double()
    for x in ins[1:]:  # (not sum(): its start value 0 would turn a sum of -0 into +0)
        s = s + x.to(torch.bfloat16).double()
    fin = s.isfinite()
    assert (s.float().double() == s)[fin].all() and s[fin].abs().max() < 1024  # exact in f32: order-free
    out = s.float() * torch.tensor(1.0 / len(ins), dtype=torch.float32) if op == AVG else s.float()
    return out.to(torch.bfloat16).float() if allreduce else out


def _run(ctx, op, coll, count, off=0, inplace=False):
    """One call on every rank. `count`: elements of an AllReduce, recvcount of a ReduceScatter; `off`: elements the
    sendbuff is misaligned by."""
    import torch
    import nccl_amd
    comms, streams, bufs = ctx
    n = len(comms)
    total = count * n if coll == "rs" else count
    ins = _inputs(n, total, 7 * count + op)
    want = _reference(ins, op, coll == "ar")
    so = 4 * off
    ro = so if inplace else HALF
    for b, x in zip(bufs, ins):
        b[HALF:HALF + 4 * total].zero_()
        b[so:so + 4 * total].copy_(x.view(torch.uint8))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for c, s, b in zip(comms, streams, bufs):
            (c.reduce_scatter_raw if coll == "rs" else c.all_reduce_raw)(b.data_ptr() + so, b.data_ptr() + ro, count, F32, op, s.cuda_stream)
    torch.cuda.synchronize()
    errs = []
    for c, b in zip(comms, bufs):
        exp = want[c.rank * count:(c.rank + 1) * count] if coll == "rs" else want
        got = b[ro:ro + 4 * exp.numel()].cpu().view(torch.float32)
        bad = _differ(got, exp)
        if c.async_error() or bad.numel():
            errs.append(f"rank {c.rank} {coll} op {op} count {count} off {off} inplace {inplace}: async {c.async_error()}, "
                        f"{bad.numel()} differ, first {bad[:4].tolist()} got {got[bad[:4]].tolist()} want {exp[bad[:4]].tolist()}")
    return errs


@pytest.mark.parametrize("op", [SUM, AVG])
@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("path", ["DIRECT", "PULLS_AG0", "PULLS_AG1"])
def test_wire_bf16_equals_rounded_f32_reference(built, monkeypatch, path, n, op):
    """Less than a wire pack; 3 channels x 3 steps over 2 slots (reuse, credits); that short by a pack and 3 elements
    (a ragged tail; the ReduceScatter's odd recvcount also goes element-wise); 1011 elements from an odd element (the
    element-wise path); in place. Without the bf16 wire the results are the unrounded fp32 sums."""
    ctx = _comms(n, monkeypatch, path, knob="NCCL_AMD_WIRE_BF16")
    errs = []
    for count, rs in ((5, 5), (n * BLOCK, BLOCK), (n * BLOCK - 8 - 3, BLOCK - 8 - 3)):
        errs += _run(ctx, op, "ar", count) + _run(ctx, op, "rs", rs)
    errs += _run(ctx, op, "ar", 1011, off=1) + _run(ctx, op, "ar", n * BLOCK - 8 - 3, inplace=True)
    for c in ctx[0]:
        c.destroy()
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("path,dtype,op,count", [("DIRECT", 9, SUM, 40001), ("DIRECT", 2, SUM, 40001), ("DIRECT", F32, 2, 40001),
                                                 ("LL", F32, SUM, 499), ("RING", F32, SUM, 40001)])
def test_everything_else_keeps_the_full_width_wire(built, monkeypatch, path, dtype, op, count):
    """A bf16 Sum, an int32 Sum and an fp32 Max on the direct plan, an fp32 Sum at an LL size and on the ring: the
    oracle's bits under the knob."""
    comms, streams, _ = _comms(3, monkeypatch, path, knob="NCCL_AMD_WIRE_BF16")
    errs = G.run_case(list(zip(comms, streams)), "allreduce", dtype, op, count, 0, seed=42)
    for c in comms:
        c.destroy()
    assert not errs, "\n".join(errs[:10])
