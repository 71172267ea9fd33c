#!/usr/bin/env python3
"""One-GPU probe of the wide-accumulator fold of the zero-copy AllReduce (NCCL_AMD_SYM_WIDE_ACC=1, kernels.h
foldRangeWide) beside the default per-hop fold of the same data.

  sym_wide_probe.py [--mode sym|staged] [--warmup 5] [--iters 10] [--rounds 3] [--step-timeout 300] [--out FILE.json]

Two communicators of 4 ranks each in one process on GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1), one created with the knob and
one without (it is read at communicator init). bf16 and e4m3 AllReduce Sum of 64 MiB per rank, out of place, on
symmetric windows; the two communicators alternate inside every round; a call's time is the slowest rank's HIP event
pair around it. The measurement runs in a child process started with a time limit. Both folds read the same bytes and
write the same bytes; they differ in the ALU work per element. No byte crosses an xGMI link here: the figures are
HBM-bound rehearsal records and say nothing about link speed. No default and no threshold is derived from them.

--mode staged: the same method on the staged direct AllReduce (NCCL_AMD_WIDE_ACC=1 beside the per-hop fold): plain
buffers in no window, NCCL_PROTO=^LL, the size far above the one-shot range, so collKernel's phase B folds. The scatter
and the gather around the fold are the same copies in both communicators."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"

N_RANKS, NBYTES = 4, 64 << 20  # ranks per communicator, bytes each rank reduces
KINDS = ("wide", "narrow")
TYPES = {"bf16": 9, "e4m3": 10}


def run_step(a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, nbytes = N_RANKS, NBYTES
    comms, wins, handles, streams = {}, {}, {}, {}
    staged = a.mode == "staged"
    if staged:
        os.environ["NCCL_PROTO"] = "^LL"
    for kind in KINDS:
        os.environ["NCCL_AMD_WIDE_ACC" if staged else "NCCL_AMD_SYM_WIDE_ACC"] = "1" if kind == "wide" else "0"
        comms[kind] = nccl_amd.Communicator.init_all([0] * n)
        streams[kind] = [torch.cuda.Stream() for _ in range(n)]
        wins[kind] = [torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]  # [send | recv]
        if staged:  # plain buffers: no window, no registration
            continue
        with nccl_amd.group():
            handles[kind] = [c.register_window(w.data_ptr(), 2 * nbytes) for c, w in zip(comms[kind], wins[kind])]

    def fill(name):  # the same normal values of magnitude 2^-6 .. 2^6 in both communicators' windows
        T = torch.bfloat16 if name == "bf16" else torch.float8_e4m3fn
        g = torch.Generator().manual_seed(7)
        cnt = nbytes // (2 if name == "bf16" else 1)
        for r in range(n):  # (4 Mi values made on the CPU, tiled)
            x = torch.exp2(torch.rand(cnt // 16, generator=g) * 12 - 6)
            x = (x * (torch.randint(0, 2, (cnt // 16,), generator=g) * 2 - 1)).to(T).view(torch.uint8).repeat(16).cuda()
            for kind in KINDS:
                wins[kind][r][:nbytes].copy_(x)
        torch.cuda.synchronize()
        return cnt

    def call(kind, dtype, cnt):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for r in range(n):
            ev[r][0].record(streams[kind][r])
        with nccl_amd.group():
            for r in range(n):
                p = wins[kind][r].data_ptr()
                comms[kind][r].all_reduce_raw(p, p + nbytes, cnt, dtype, 0, streams[kind][r].cuda_stream)
        for r in range(n):
            ev[r][1].record(streams[kind][r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    out = {}
    for name, dtype in TYPES.items():
        cnt = fill(name)
        for _ in range(a.warmup):
            for kind in KINDS:
                call(kind, dtype, cnt)
        rounds = []
        for _ in range(a.rounds):
            t = {k: [] for k in KINDS}
            for _ in range(a.iters):
                for kind in KINDS:
                    t[kind].append(call(kind, dtype, cnt))
            rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                               "max_ms": round(max(v), 4)} for k, v in t.items()})
        med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in KINDS}
        ratios = [r["wide"]["median_ms"] / r["narrow"]["median_ms"] for r in rounds]
        differ = int((wins["wide"][0][nbytes:] != wins["narrow"][0][nbytes:]).sum())
        out[name] = {"rounds": rounds, "wide_median_ms": med["wide"], "narrow_median_ms": med["narrow"],
                     "wide_over_narrow": round(med["wide"] / med["narrow"], 3),
                     "wide_over_narrow_per_round": [round(x, 3) for x in ratios],
                     "result_bytes_that_differ_rank0": differ}
    errs = [c.async_error() for k in KINDS for c in comms[k]]
    for kind in KINDS:
        for c, h in zip(comms[kind], handles.get(kind, [])):
            c.deregister_window(h)
        for c in comms[kind]:
            c.destroy()
    what = ("staged direct AllReduce Sum on plain buffers (NCCL_PROTO=^LL) with the wide-accumulator fold (NCCL_AMD_WIDE_ACC=1) "
            if staged else
            "zero-copy AllReduce Sum on symmetric windows with the wide-accumulator fold (NCCL_AMD_SYM_WIDE_ACC=1) ")
    res = {"what": what + "beside the per-hop fold, two communicators of one process on one GPU (no xGMI link is crossed)",
           "n_ranks": n, "bytes_per_rank": nbytes, "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank; the two communicators alternate",
           "types": out, "async_errors": errs, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return 0 if not any(errs) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("sym", "staged"), default="sym")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return run_step(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mode", a.mode, "--warmup", str(a.warmup), "--iters", str(a.iters),
           "--rounds", str(a.rounds)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.step_timeout} s", file=sys.stderr)
        return 1
    if out.returncode != 0:
        print(f"the measurement failed ({out.returncode})\n{out.stdout[-2000:]}{out.stderr[-2000:]}", file=sys.stderr)
        return 1
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
