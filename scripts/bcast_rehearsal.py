#!/usr/bin/env python3
"""One-GPU rehearsal of the staged Broadcast beside an AllGather of the same total output bytes, on the same
communicator and build: N ranks of one process on GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1), HIP-event time per call.

  bcast_rehearsal.py [--n 2] [--mib 256] [--warmup 5] [--iters 20] [--rounds 3] [--root 0] [--out FILE.json]

Each round times `iters` Broadcasts and `iters` AllGathers, alternating one of each; a call's time is the slowest
rank's event pair around it. Reported: median / min / max of the per-call times per round, and the ratio of the
medians. No byte crosses an xGMI link here (every rank shares the one GPU): the figures are HBM-bound rehearsal
records, not link measurements. Under rocprofv3 --kernel-trace --stats, use --rounds 1 --iters 5."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")
os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, total = a.n, a.mib << 20
    assert total % n == 0
    comms = nccl_amd.Communicator.init_all([0] * n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)   # the root's sendbuff
    recv = [torch.zeros(total, dtype=torch.uint8, device="cuda") for _ in range(n)]
    part = [src[r * (total // n):(r + 1) * (total // n)] for r in range(n)]                # AllGather inputs

    def call(kind):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for r in range(n):
            ev[r][0].record(streams[r])
        with nccl_amd.group():
            for r in range(n):
                if kind == "broadcast":
                    comms[r].broadcast(src if r == a.root else None, recv[r], root=a.root, stream=streams[r])
                else:
                    comms[r].allgather(part[r], recv[r], stream=streams[r])
        for r in range(n):
            ev[r][1].record(streams[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    for _ in range(a.warmup):
        call("broadcast")
        call("allgather")
    # both compute the same bytes on every rank: check once, after the warm-up
    call("allgather")
    ok_ag = all(torch.equal(x, src) for x in recv)
    for x in recv:
        x.zero_()
    call("broadcast")
    ok_bc = all(torch.equal(x, src) for x in recv)
    rounds = []
    for _ in range(a.rounds):
        t = {"broadcast": [], "allgather": []}
        for _ in range(a.iters):
            for kind in ("broadcast", "allgather"):
                t[kind].append(call(kind))
        rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for k, v in t.items()})
    errs = [c.async_error() for c in comms]
    for c in comms:
        c.destroy()
    mb = statistics.median(r["broadcast"]["median_ms"] for r in rounds)
    mg = statistics.median(r["allgather"]["median_ms"] for r in rounds)
    res = {"what": "staged Broadcast vs AllGather of the same total output bytes, ranks of one process on one GPU",
           "n_ranks": n, "bytes": total, "root": a.root, "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank", "rounds": rounds,
           "broadcast_median_ms": mb, "allgather_median_ms": mg, "broadcast_over_allgather": round(mb / mg, 3),
           "outputs_match_root": bool(ok_bc), "allgather_outputs_match": bool(ok_ag), "async_errors": errs,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok_bc and ok_ag and not any(errs) else 1


if __name__ == "__main__":
    sys.exit(main())
