#!/usr/bin/env python3
"""One-GPU probe of the staged ncclSend / ncclRecv path beside a device-to-device hipMemcpyAsync of the same bytes.

  p2p_probe.py [--warmup 5] [--iters 10] [--rounds 3] [--step-timeout 240] [--out FILE.json]

Two steps, each in a fresh child process of its own (started with a time limit; a step that fails or runs out of time
ends the probe, nothing further is started on the GPU):
  exchange   2 ranks on GPU 0, each sends 256 MiB to the other and receives 256 MiB in one group;
  alltoall   4 ranks on GPU 0, ncclAlltoAll of 64 MiB per rank (16 MiB per pair).
Ranks are comms of one process on GPU 0 (NCCL_MULTI_RANK_GPU_ENABLE=1). A call's time is the slowest rank's HIP event
pair around it. The yardstick, timed in alternation with it in the same rounds: every rank copies the bytes it sends
with one hipMemcpyAsync (device to device) on its own stream. The staged path copies every byte twice (into the
peer's staging slot, out of it), so about twice the yardstick is its floor on one GPU. No byte crosses an xGMI link
here: the figures are HBM-bound rehearsal records and say nothing about link speed."""
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

STEPS = {"exchange": (2, 256 << 20), "alltoall": (4, 64 << 20)}  # ranks, bytes each rank sends


def run_step(step, a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, nbytes = STEPS[step]
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    comms = nccl_amd.Communicator.init_all([0] * n)
    streams = [torch.cuda.Stream() for _ in range(n)]
    g = torch.Generator(device="cuda").manual_seed(1)
    send = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    recv = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(n)]

    def call(kind):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for r in range(n):
            ev[r][0].record(streams[r])
        if kind == "memcpy":
            for r in range(n):
                rc = hip.hipMemcpyAsync(recv[r].data_ptr(), send[r].data_ptr(), nbytes, 3, streams[r].cuda_stream)
                assert rc == 0, f"hipMemcpyAsync returned {rc}"
        else:
            with nccl_amd.group():
                for r in range(n):
                    if step == "exchange":
                        comms[r].send(send[r], 1 - r, stream=streams[r])
                        comms[r].recv(recv[r], 1 - r, stream=streams[r])
                    else:
                        comms[r].alltoall(send[r], recv[r], stream=streams[r])
        for r in range(n):
            ev[r][1].record(streams[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    for _ in range(a.warmup):
        call("memcpy")
        call("p2p")
    blk = nbytes // n
    if step == "exchange":
        ok = all(torch.equal(recv[r], send[1 - r]) for r in range(n))
    else:
        ok = all(torch.equal(recv[r], torch.cat([send[i][r * blk:(r + 1) * blk] for i in range(n)])) for r in range(n))
    rounds = []
    for _ in range(a.rounds):
        t = {"p2p": [], "memcpy": []}
        for _ in range(a.iters):
            for kind in ("p2p", "memcpy"):
                t[kind].append(call(kind))
        rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for k, v in t.items()})
    errs = [c.async_error() for c in comms]
    for c in comms:
        c.destroy()
    mp_, mm = (statistics.median(r[k]["median_ms"] for r in rounds) for k in ("p2p", "memcpy"))
    res = {"step": step, "n_ranks": n, "bytes_sent_per_rank": nbytes, "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank", "rounds": rounds,
           "p2p_median_ms": mp_, "memcpy_median_ms": mm, "p2p_over_memcpy": round(mp_ / mm, 3),
           "outputs_match": bool(ok), "async_errors": errs, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return 0 if ok and not any(errs) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a)
    results = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--warmup", str(a.warmup), "--iters", str(a.iters),
               "--rounds", str(a.rounds)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 1
        if out.returncode != 0:
            print(f"step {step} failed ({out.returncode}); stopping\n{out.stdout[-2000:]}{out.stderr[-2000:]}", file=sys.stderr)
            return 1
        results.append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {"what": "staged send/recv and all-to-all beside hipMemcpyAsync of the same bytes, ranks of one process on one "
                   "GPU (no xGMI link is crossed)", "steps": results}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
