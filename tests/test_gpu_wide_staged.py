"""GPU tests of the wide-accumulator fold on the staged and LL plans (NCCL_AMD_WIDE_ACC=1): fp16 /
bf16 / fp8 Sum and Avg on plain buffers — the direct kernel's phase B, one-shot B, LL / LL64 pass 2 and their group
batches — decode to f32, add in f32 in the fold order (ranks owner+1, ..., owner; Reduce: root+1, ..., root) and round
once. The reference is plain torch on the CPU, bit for bit (any NaN code equals any NaN code); inputs, reference and
comparison are those of the zero-copy kernels' test. All ranks share the one GPU (single process)."""
import multiprocessing as mp
import os

import pytest

from tests import gpu_cases as G
from tests.test_gpu_sym_wide import AVG, BATCH, SUM, _differ, _inputs, _reference, _tt

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
pytestmark = pytest.mark.gpu

HALF = 2 << 20  # per-rank buffer: inputs from 0, outputs from HALF; the calls of one group side by side in both
ENVS = dict(G.BOUNDARY_ENVS, DEFAULT_SLOTS={"NCCL_ALGO": "DIRECT", "NCCL_PROTO": "Simple"})


def _comms(n, monkeypatch, path, knob="NCCL_AMD_WIDE_ACC", **extra):
    import torch
    import nccl_amd
    os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
    for k, v in {**ENVS[path], knob: "1", **extra}.items():
        monkeypatch.setenv(k, v)
    torch.cuda.set_device(0)
    comms = nccl_amd.Communicator.init_all([0] * n)
    return comms, [torch.cuda.Stream() for _ in comms], [torch.empty(2 * HALF, dtype=torch.uint8, device="cuda") for _ in comms]


def _run(ctx, dtype, op, calls, seed):
    """The calls [(coll, count, off, inplace), ...] of every rank in ONE group (two calls: a batch). `count`: elements
    of an AllReduce / a Reduce to root 1, recvcount of a ReduceScatter; `off`: elements the sendbuff is misaligned by."""
    import torch
    import nccl_amd
    comms, streams, bufs = ctx
    T, epp, _, big = _tt(dtype)
    n, es, plan, at, errs = len(comms), 16 // epp, [], 0, []
    for i, (coll, count, off, inplace) in enumerate(calls):
        total = count * n if coll == "rs" else count
        ins = _inputs(n, dtype, total, seed + i)
        # Reduce: every element in the root's order — one block, the ranks renumbered from the root; AllReduce: rank
        # blocks of divUp(count, n) in whole packs
        src, chunk = (ins[1:] + ins[:1], total) if coll == "reduce" else (ins, count if coll == "rs" else -(-(-(-count // n)) // epp) * epp)
        so = at + off * es
        ro = so if inplace else HALF + at
        for b, x in zip(bufs, ins):
            b[HALF + at:HALF + at + total * es].zero_()
            b[so:so + total * es].copy_(x.view(torch.uint8))
        plan.append((coll, count, so, ro, ins, _reference(src, dtype, op, chunk)))
        at += -(-(total + off) * es // 256) * 256
    torch.cuda.synchronize()
    with nccl_amd.group():
        for coll, count, so, ro, _, _ in plan:
            for c, s, b in zip(comms, streams, bufs):
                args = (b.data_ptr() + so, b.data_ptr() + ro, count, dtype, op)
                if coll == "reduce":
                    c.reduce_raw(*args, 1, s.cuda_stream)
                else:
                    (c.reduce_scatter_raw if coll == "rs" else c.all_reduce_raw)(*args, s.cuda_stream)
    torch.cuda.synchronize()
    for coll, count, so, ro, ins, want in plan:
        for c, b in zip(comms, bufs):
            r = c.rank
            if coll == "reduce" and r != 1:
                continue
            exp = want[r * count:(r + 1) * count] if coll == "rs" else want
            got = b[ro:ro + exp.numel() * es].cpu().view(T)
            tag, bad = f"rank {r} {coll} dt {dtype} op {op} count {count} at {so} -> {ro}", _differ(got, exp)
            if c.async_error() or bad.numel():
                errs.append(f"{tag}: async {c.async_error()}, {bad.numel()} differ, first {bad[:4].tolist()} got "
                            f"{got[bad[:4]].float().tolist()} want {exp[bad[:4]].float().tolist()}")
            # the fixed element: per-hop rounding in T loses every 1 added to `big`, the wide fold keeps them
            if op == SUM and (coll == "ar" or (coll == "rs" and r == 0)):
                hop = ins[1][0]
                for k in (*range(2, n), 0):
                    hop = (ins[k][0].float() + hop.float()).to(T)
                wide = float(torch.tensor(big + n - 1).to(T))
                if float(hop) != big or float(got[0]) != wide:
                    errs.append(f"{tag}: fixed element {float(got[0])}, per-hop fold {float(hop)}, wide {wide}")
    return errs


def _calls(path, n, epp):
    """The groups of calls of one path, each group one _run."""
    es, one = 16 // epp, lambda coll, count, off=0, inplace=False: [(coll, count, off, inplace)]
    if path == "DIRECT":
        # 5: less than a pack. A rank block of 27008 bytes: 3 channels x 3 steps of a 4096-byte slot (2 slots: reuse,
        # credits), the last block short by a pack and 3 elements (a ragged tail). 1011 from an odd element: the
        # element-wise path. Two AllReduces in one group: the batch kernel
        blk, big = 27008 // es, n * (27008 // es) - epp - 3
        return [one("ar", 5), one("ar", big), one("ar", 5, 0, True), one("ar", big, 0, True), one("rs", 5), one("rs", blk),
                one("reduce", 5), one("reduce", big), one("ar", 1011, 1), one("ar", big) + one("ar", 777)]
    if path == "DEFAULT_SLOTS":  # two channels of one full batch and two packs each; the last block a ragged rest
        return [one("ar", n * (2 * BATCH + 4 * epp)), one("ar", n * (2 * BATCH + 4 * epp) - epp - 3)]
    if path == "ONESHOT":  # below a pack; ~1000 bytes on 2 channels: a channel's portion spans two rank blocks
        return [one("ar", 5), one("ar", 1000 // es - 3)]
    # LL / LL64: below 8 bytes; ~1000 bytes on all 4 channels, no multiple of 8 or 56 (a ReduceScatter's rank blocks
    # are whole payloads on these plans: 8 and 992 bytes); two AllReduces in one group: the batch kernels
    few, many = 6 // es, 1000 // es - 1
    return [one("ar", few), one("ar", many), one("reduce", few), one("reduce", many), one("rs", 8 // es),
            one("rs", 992 // es), one("ar", many) + one("ar", few)]


@pytest.mark.parametrize("dtype", [6, 9, 10, 11])
@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("path", ["DIRECT", "DEFAULT_SLOTS", "ONESHOT", "LL", "LL128"])
def test_wide_fold_equals_f32_reference(built, monkeypatch, path, n, dtype):
    epp = _tt(dtype)[1]
    # DEFAULT_SLOTS: a channel part of exactly one wide batch (512 threads x packs per thread) and two packs
    ctx = _comms(n, monkeypatch, path, **({"NCCL_AMD_MIN_CHANNEL_BYTES": str((BATCH + 2 * epp) * 16 // epp)} if path == "DEFAULT_SLOTS" else {}))
    errs = [e for op in (SUM, AVG) for i, calls in enumerate(_calls(path, n, epp)) for e in _run(ctx, dtype, op, calls, 20 * i + op)]
    for c in ctx[0]:
        c.destroy()
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("path,dtype,op,premul", [(p, *c) for p in ("DIRECT", "LL") for c in ((9, 2, None), (2, 0, None), (9, 0, 0x3F00))]
                         + [("RING", 9, 0, None)])
def test_other_plans_and_ops_keep_the_narrow_fold(built, monkeypatch, path, dtype, op, premul):
    """bf16 Max, int32 Sum and a user PreMulSum (bf16, 0.5) on the direct and LL plans, a bf16 Sum on the ring: the
    oracle's per-hop bits under the knob."""
    comms, streams, _ = _comms(3, monkeypatch, path)
    ops = {c.rank: c.create_pre_mul_sum(premul, dtype) for c in comms} if premul is not None else None
    errs = G.run_case(list(zip(comms, streams)), "allreduce", dtype, op, 499 if path == "LL" else 40001, 0, seed=42,
                      user_ops=ops, premul=premul)
    for c in comms:
        c.destroy()
    assert not errs, "\n".join(errs[:10])


def _identity_worker(q):
    """Per datatype one path, a Sum on plain buffers under each knob: the kernels the log names (bits: the tests above)."""
    klog = os.environ["NCCL_AMD_KERNEL_LOG"] = f"/tmp/nccl_amd_wide_staged_kernels_{os.getpid()}.log"  # read at load
    out = {}
    for dtype, path in ((6, "DIRECT"), (9, "ONESHOT"), (10, "LL"), (11, "LL128")):
        for knob in ("NCCL_AMD_WIDE_ACC", "NCCL_AMD_SYM_WIDE_ACC"):
            with pytest.MonkeyPatch.context() as mpatch:
                comms, streams, _ = _comms(3, mpatch, path, knob)
                G.run_case(list(zip(comms, streams)), "allreduce", dtype, 0, 499, 0, seed=8)
                for c in comms:
                    c.destroy()
            out[dtype, knob] = open(klog).read().splitlines()
            os.remove(klog)
    q.put(out)


def test_kernel_log_names_the_wide_kernels(built):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_identity_worker, args=(q,))
    p.start()
    p.join(timeout=240)
    assert p.exitcode == 0, f"the worker ended with {p.exitcode}"
    out = q.get(timeout=10)
    for (dtype, knob), lines in out.items():
        wide = [ln for ln in lines if ("collKernel<" in ln or "llKernel<" in ln) and (", 16, " in ln or ", 17, " in ln)]
        assert bool(wide) == (knob == "NCCL_AMD_WIDE_ACC"), f"dt {dtype} under {knob}: launched {lines}"
