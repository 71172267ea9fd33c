#!/usr/bin/env python3
"""One-GPU probe of the LL protocol of ncclSend / ncclRecv beside the staged path at the same sizes.

  p2p_ll_probe.py [--warmup 20] [--iters 50] [--rounds 3] [--timeout 240] [--out FILE.json]

Two communicators of two ranks each, all four ranks comms of ONE process on GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1): one
created with NCCL_AMD_P2P_LL_BYTES = the largest size measured (and line slots that hold it on the default four
channels), the other without the knob. A call is a ping-pong: rank 0 sends and rank 1 receives, then rank 1 sends the
bytes back and rank 0 receives them (two groups per rank, in that order on each rank's stream). Its time is the slower
rank's HIP event pair around both groups; after the warm-up the calls alternate between the two communicators, and a
round's figure is the median over its calls. Reported: the median of the rounds' medians with their spread.

The work runs in a child process started with a time limit. Every rank shares one HBM here and no byte crosses an
xGMI link: the figures record launch, handshake and HBM cost on one GPU. Where LL stops paying on xGMI is unknown until
a multi-GPU run measures it, which is why NCCL_AMD_P2P_LL_BYTES defaults to 0."""
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

SIZES = (8, 64, 512, 4096, 32768)
# 32 KiB of payload on 4 channels: 8 KiB per channel and slot = the default 16 KiB of lines
LL_ENV = {"NCCL_AMD_P2P_LL_BYTES": str(max(SIZES)), "NCCL_AMD_P2P_LL_LINE_BYTES": "16384", "NCCL_AMD_P2P_LL_NCHANNELS": "4"}


def run(a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    os.environ.update(LL_ENV)
    sets = {"ll": nccl_amd.Communicator.init_all([0, 0])}
    for k in LL_ENV:
        del os.environ[k]
    sets["staged"] = nccl_amd.Communicator.init_all([0, 0])
    streams = {k: [torch.cuda.Stream() for _ in range(2)] for k in sets}
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (max(SIZES),), dtype=torch.uint8, device="cuda", generator=g)
    mid = torch.zeros_like(src)
    back = torch.zeros_like(src)

    def call(kind, nbytes):
        comms, ss = sets[kind], streams[kind]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2)]
        for r in range(2):
            ev[r][0].record(ss[r])
        with nccl_amd.group():
            comms[0].send(src[:nbytes], 1, stream=ss[0])
            comms[1].recv(mid[:nbytes], 0, stream=ss[1])
        with nccl_amd.group():
            comms[1].send(mid[:nbytes], 0, stream=ss[1])
            comms[0].recv(back[:nbytes], 1, stream=ss[0])
        for r in range(2):
            ev[r][1].record(ss[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev) * 1e3  # us

    rows, ok = [], True
    for nbytes in SIZES:
        for kind in sets:
            for _ in range(a.warmup):
                call(kind, nbytes)
            back.zero_()
            call(kind, nbytes)
            ok = ok and torch.equal(back[:nbytes], src[:nbytes])
        meds = {k: [] for k in sets}
        for _ in range(a.rounds):
            t = {k: [] for k in sets}
            for _ in range(a.iters):
                for kind in sets:
                    t[kind].append(call(kind, nbytes))
            for k in sets:
                meds[k].append(statistics.median(t[k]))
        row = {"bytes": nbytes}
        for k in sets:
            row[k + "_us"] = round(statistics.median(meds[k]), 2)
            row[k + "_rounds_us"] = [round(m, 2) for m in meds[k]]
        row["ll_over_staged"] = round(row["ll_us"] / row["staged_us"], 3)
        rows.append(row)
    errs = [c.async_error() for cs in sets.values() for c in cs]
    for cs in sets.values():
        for c in cs:
            c.destroy()
    res = {"what": "ping-pong (0 -> 1, then 1 -> 0) through ncclSend / ncclRecv: the LL protocol beside the staged path, "
                   "four ranks of one process on one GPU; every rank shares one HBM, no xGMI link is crossed",
           "ll_env": LL_ENV, "sizes": rows, "warmup": a.warmup, "iters_per_round": a.iters, "rounds": a.rounds,
           "timing": "HIP events on both ranks' streams around the two groups, slower rank; calls alternate between the "
                     "communicators; median of the rounds' medians",
           "outputs_match": bool(ok), "async_errors": errs, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return 0 if ok and not any(errs) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return run(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(a.warmup), "--iters", str(a.iters),
           "--rounds", str(a.rounds)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.timeout} s", file=sys.stderr)
        return 1
    if out.returncode != 0:
        print(f"the probe failed ({out.returncode})\n{out.stdout[-2000:]}{out.stderr[-2000:]}", file=sys.stderr)
        return 1
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
