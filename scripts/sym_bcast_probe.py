#!/usr/bin/env python3
"""One-GPU probe of the zero-copy Broadcast (NCCL_AMD_SYM_BCAST=1, recvbuff in a symmetric window, kernels.h
symBcastKernel) beside the staged Broadcast of the same payload on the same communicator.

  sym_bcast_probe.py [--warmup 3] [--iters 10] [--rounds 3] [--step-timeout 300] [--out FILE.json]

Per case (4 ranks x 64 MiB, 8 ranks x 256 MiB; out of place and in place) one communicator of n ranks in one process on
GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1), created with the knob. Every rank holds a registered window and a buffer outside
any window, each [send | recv]: a Broadcast into the window runs the zero-copy kernel, one into the outside buffer the
staged kernel. The two alternate inside every round; a call's time is the slowest rank's HIP event pair around it; the
root rotates with the iteration. Every case runs in a child process of its own, started with a time limit. No byte
crosses an xGMI link here: the figures are HBM-bound rehearsal records and say nothing about link speed. No default and
no threshold is derived from them."""
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
os.environ["NCCL_AMD_SYM_BCAST"] = "1"

CASES = [(4, 64 << 20), (8, 256 << 20)]
KINDS = ("zero_copy", "staged")


def run_step(a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, nbytes = a.ranks, a.bytes
    comms = nccl_amd.Communicator.init_all([0] * n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    bufs = {k: [torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)] for k in KINDS}
    with nccl_amd.group():
        handles = [c.register_window(w.data_ptr(), 2 * nbytes) for c, w in zip(comms, bufs["zero_copy"])]
    g = torch.Generator().manual_seed(11)
    pattern = torch.randint(0, 256, (nbytes // 64,), generator=g, dtype=torch.uint8).repeat(64).cuda()

    def call(kind, inplace, root):
        for r in range(n):  # the root's payload, marked with the root; every output cleared
            b = bufs[kind][r]
            b.zero_()
            if r == root:
                b[nbytes if inplace else 0:][:nbytes].copy_(pattern).add_(root)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for r in range(n):
            ev[r][0].record(streams[r])
        with nccl_amd.group():
            for r in range(n):
                p = bufs[kind][r].data_ptr()
                comms[r].broadcast_raw(p + nbytes if inplace else p, p + nbytes, nbytes, 0, root, streams[r].cuda_stream)
        for r in range(n):
            ev[r][1].record(streams[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    out = {}
    for place in ("out_of_place", "in_place"):
        inplace = place == "in_place"
        for i in range(a.warmup):
            for kind in KINDS:
                call(kind, inplace, i % n)
        rounds = []
        for _ in range(a.rounds):
            t = {k: [] for k in KINDS}
            for i in range(a.iters):
                for kind in KINDS:
                    t[kind].append(call(kind, inplace, i % n))
            rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                               "max_ms": round(max(v), 4)} for k, v in t.items()})
        root = (a.iters - 1) % n
        wrong = sum(int((bufs[k][r][nbytes:] != pattern + root).sum()) for k in KINDS for r in range(n))
        med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in KINDS}
        out[place] = {"rounds": rounds, "zero_copy_median_ms": med["zero_copy"], "staged_median_ms": med["staged"],
                      "zero_copy_over_staged": round(med["zero_copy"] / med["staged"], 3),
                      "zero_copy_over_staged_per_round": [round(r["zero_copy"]["median_ms"] / r["staged"]["median_ms"], 3)
                                                          for r in rounds],
                      "wrong_bytes_last_call": wrong}
    errs = [c.async_error() for c in comms]
    for c, h in zip(comms, handles):
        c.deregister_window(h)
    for c in comms:
        c.destroy()
    print(json.dumps({"n_ranks": n, "bytes": nbytes, "places": out, "async_errors": errs,
                      "device": torch.cuda.get_device_name(0)}))
    return 0 if not any(errs) and not any(p["wrong_bytes_last_call"] for p in out.values()) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--bytes", type=int, default=64 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return run_step(a)
    res = {"what": "ncclBroadcast with the recvbuff in a symmetric window under NCCL_AMD_SYM_BCAST=1 (zero-copy, "
                   "symBcastKernel) beside the same Broadcast with the recvbuff outside any window (staged), alternating "
                   "on one communicator of one process on one GPU (no xGMI link is crossed)",
           "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank; the root rotates", "cases": []}
    for n, nbytes in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(a.warmup), "--iters", str(a.iters),
               "--rounds", str(a.rounds), "--ranks", str(n), "--bytes", str(nbytes)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{n} ranks x {nbytes} bytes: no result within {a.step_timeout} s", file=sys.stderr)
            return 1  # nothing more is started on this GPU
        if out.returncode != 0:
            print(f"{n} ranks x {nbytes} bytes failed ({out.returncode})\n{out.stdout[-2000:]}{out.stderr[-2000:]}",
                  file=sys.stderr)
            return 1
        res["cases"].append(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
