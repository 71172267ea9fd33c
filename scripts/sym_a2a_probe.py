#!/usr/bin/env python3
"""One-GPU probe of the zero-copy ncclAlltoAll (sendbuff in a symmetric window, kernels.h symA2AKernel) beside the
staged ncclAlltoAll of the same data on the same communicator and a device-to-device hipMemcpyAsync of the same bytes.

  sym_a2a_probe.py [--warmup 5] [--iters 10] [--rounds 3] [--step-timeout 240] [--out FILE.json]

4 ranks of one process on GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1), 64 MiB per rank (16 MiB per pair). Every rank holds
its data twice: in a window registered with NCCL_WIN_COLL_SYMMETRIC (the zero-copy call) and in a buffer outside any
window (the staged call: the send / recv expansion through the staging slots, which is what every AlltoAll ran before
the zero-copy kernel existed). The three calls alternate inside every round; a call's time is the slowest rank's HIP
event pair around it. The measurement runs in a child process started with a time limit. The zero-copy path copies
every byte once (2 S of HBM traffic for S bytes), the staged path twice (4 S), the yardstick once. No byte crosses an
xGMI link here: the figures are HBM-bound rehearsal records and say nothing about link speed."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"

N_RANKS, NBYTES = 4, 64 << 20  # ranks, bytes each rank sends
KINDS = ("zero_copy", "staged", "memcpy")


def run_step(a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, nbytes = N_RANKS, NBYTES
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    comms = nccl_amd.Communicator.init_all([0] * n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    g = torch.Generator(device="cuda").manual_seed(1)
    # window: [sendbuff | recvbuff]; outside: the same data and a recvbuff of its own
    win = [torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
    with nccl_amd.group():
        handles = [c.register_window(w.data_ptr(), 2 * nbytes) for c, w in zip(comms, win)]
    send = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    recv = {k: ([w[nbytes:] for w in win] if k == "zero_copy" else
                [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]) for k in KINDS}
    for r in range(n):
        win[r][:nbytes].copy_(send[r])
    torch.cuda.synchronize()

    def call(kind):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for r in range(n):
            ev[r][0].record(streams[r])
        if kind == "memcpy":
            for r in range(n):
                rc = hip.hipMemcpyAsync(recv[kind][r].data_ptr(), send[r].data_ptr(), nbytes, 3, streams[r].cuda_stream)
                assert rc == 0, f"hipMemcpyAsync returned {rc}"
        else:
            with nccl_amd.group():
                for r in range(n):
                    src = win[r][:nbytes] if kind == "zero_copy" else send[r]
                    comms[r].alltoall(src, recv[kind][r], stream=streams[r])
        for r in range(n):
            ev[r][1].record(streams[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    for _ in range(a.warmup):
        for kind in KINDS:
            call(kind)
    blk = nbytes // n
    want = [torch.cat([send[i][r * blk:(r + 1) * blk] for i in range(n)]) for r in range(n)]
    ok = all(torch.equal(recv[k][r], want[r]) for k in ("zero_copy", "staged") for r in range(n))
    rounds = []
    for _ in range(a.rounds):
        t = {k: [] for k in KINDS}
        for _ in range(a.iters):
            for kind in KINDS:
                t[kind].append(call(kind))
        rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for k, v in t.items()})
    errs = [c.async_error() for c in comms]
    for c, h in zip(comms, handles):
        c.deregister_window(h)
    for c in comms:
        c.destroy()
    med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in KINDS}
    res = {"what": "zero-copy all-to-all (sendbuff in a symmetric window) beside the staged all-to-all of the same data on "
                   "the same communicator and hipMemcpyAsync of the same bytes, ranks of one process on one GPU (no xGMI "
                   "link is crossed)",
           "n_ranks": n, "bytes_sent_per_rank": nbytes, "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank; the three calls alternate",
           "rounds": rounds, "zero_copy_median_ms": med["zero_copy"], "staged_median_ms": med["staged"],
           "memcpy_median_ms": med["memcpy"], "zero_copy_over_staged": round(med["zero_copy"] / med["staged"], 3),
           "zero_copy_over_memcpy": round(med["zero_copy"] / med["memcpy"], 3),
           "staged_over_memcpy": round(med["staged"] / med["memcpy"], 3),
           "outputs_match": bool(ok), "async_errors": errs, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return 0 if ok and not any(errs) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return run_step(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(a.warmup), "--iters", str(a.iters),
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
