#!/usr/bin/env python3
"""One-GPU probe of the one-sided put beside the staged ncclSend / ncclRecv exchange and a device-to-device
hipMemcpyAsync of the same bytes, all three in alternation in the same run.

  rma_probe.py [--warmup 5] [--iters 10] [--rounds 3] [--step-timeout 240] [--out FILE.json]

One step, in a fresh child process started with a time limit (a step that fails or runs out of time ends the probe):
2 ranks on GPU 0 (comms of one process, NCCL_MULTI_RANK_GPU_ENABLE=1); per call
  put      each rank puts 256 MiB into the other's window (ncclPutSignal) and waits for the other's (ncclWaitSignal),
           both ranks' calls in one group;
  p2p      each rank sends 256 MiB to the other and receives 256 MiB in one group (the staged path, unchanged);
  memcpy   each rank copies 256 MiB with one hipMemcpyAsync (device to device) on its own stream.
A call's time is the slowest rank's HIP event pair around it. The byte model: the put reads and writes every byte once,
the staged exchange twice (into the peer's staging slot, out of it), the copy once. No byte crosses an xGMI link here:
the figures are HBM-bound rehearsal records and say nothing about link speed."""
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

N, NBYTES = 2, 256 << 20
KINDS = ("put", "p2p", "memcpy")


def run_step(a):
    import torch
    import nccl_amd
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    comms = nccl_amd.Communicator.init_all([0] * N)
    streams = [torch.cuda.Stream() for _ in range(N)]
    g = torch.Generator(device="cuda").manual_seed(1)
    send = [torch.randint(0, 256, (NBYTES,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(N)]
    recv = [torch.zeros(NBYTES, dtype=torch.uint8, device="cuda") for _ in range(N)]
    with nccl_amd.group():   # the sources: symmetric windows; the targets: the windows the puts write
        swin = [comms[r].register_window(send[r].data_ptr(), NBYTES) for r in range(N)]
    with nccl_amd.group():
        rwin = [comms[r].register_window(recv[r].data_ptr(), NBYTES) for r in range(N)]

    def call(kind):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
        for r in range(N):
            ev[r][0].record(streams[r])
        if kind == "memcpy":
            for r in range(N):
                rc = hip.hipMemcpyAsync(recv[r].data_ptr(), send[r].data_ptr(), NBYTES, 3, streams[r].cuda_stream)
                assert rc == 0, f"hipMemcpyAsync returned {rc}"
        else:
            with nccl_amd.group():
                for r in range(N):
                    if kind == "put":
                        comms[r].put_signal(send[r], 1 - r, rwin[r], 0, stream=streams[r])
                        comms[r].wait_signal([(1 - r, 1)], stream=streams[r])
                    else:
                        comms[r].send(send[r], 1 - r, stream=streams[r])
                        comms[r].recv(recv[r], 1 - r, stream=streams[r])
        for r in range(N):
            ev[r][1].record(streams[r])
        torch.cuda.synchronize()
        return max(s.elapsed_time(e) for s, e in ev)

    ok = {}
    for kind in ("put", "p2p"):   # each path's output checked on its own
        for r in range(N):
            recv[r].zero_()
        torch.cuda.synchronize()
        call(kind)
        ok[kind] = all(torch.equal(recv[r], send[1 - r]) for r in range(N))
    for _ in range(a.warmup):
        for kind in KINDS:
            call(kind)
    rounds = []
    for _ in range(a.rounds):
        t = {k: [] for k in KINDS}
        for _ in range(a.iters):
            for kind in KINDS:
                t[kind].append(call(kind))
        rounds.append({k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                           "max_ms": round(max(v), 4)} for k, v in t.items()})
    errs = [c.async_error() for c in comms]
    for r in range(N):
        comms[r].deregister_window(rwin[r])
        comms[r].deregister_window(swin[r])
    for c in comms:
        c.destroy()
    med = {k: statistics.median(r[k]["median_ms"] for r in rounds) for k in KINDS}
    res = {"step": "exchange", "n_ranks": N, "bytes_put_per_rank": NBYTES, "warmup": a.warmup, "iters_per_round": a.iters,
           "timing": "HIP events on every rank's stream around the call, slowest rank", "rounds": rounds,
           "put_median_ms": med["put"], "p2p_median_ms": med["p2p"], "memcpy_median_ms": med["memcpy"],
           "put_over_memcpy": round(med["put"] / med["memcpy"], 3), "p2p_over_memcpy": round(med["p2p"] / med["memcpy"], 3),
           "put_over_p2p": round(med["put"] / med["p2p"], 3), "outputs_match": ok, "async_errors": errs,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    return 0 if all(ok.values()) and not any(errs) else 1


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
        return run_step(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "exchange", "--warmup", str(a.warmup), "--iters", str(a.iters),
           "--rounds", str(a.rounds)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
    except subprocess.TimeoutExpired:
        print(f"no result within {a.step_timeout} s; stopping", file=sys.stderr)
        return 1
    if out.returncode != 0:
        print(f"the step failed ({out.returncode}); stopping\n{out.stdout[-2000:]}{out.stderr[-2000:]}", file=sys.stderr)
        return 1
    res = {"what": "one-sided put + wait beside the staged send/recv exchange and hipMemcpyAsync of the same bytes, in "
                   "alternation in one run; ranks of one process on one GPU (no xGMI link is crossed)",
           "steps": [json.loads(out.stdout.strip().splitlines()[-1])]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
