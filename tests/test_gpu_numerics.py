"""GPU checks of the kernels' 1-byte element arithmetic, exhaustively:

* tests/native/fp8_cvt_probe: the hardware fp8 conversions the kernels use (numerics.h fp8ToF32Hw /
  f32ToFp8SatHw: v_cvt_f32_fp8 / v_cvt_pk_fp8_f32 with a satfinite clamp and software NaN) equal the software
  conversions (checked against the oracle on the host, tests/test_numerics.py) for every code and every half;
* every (a, b) byte pair of e4m3 / e5m2 / uint8 / int8 through an n=2 AllReduce (both ranks on the one GPU)
  for every operator, on the LL kernel and on the staged kernel (there also ReduceScatter and Reduce) and on the
  forced LL128, one-shot, registered zero-copy, ring and chain kernels, bit-exact vs the oracle — the reference's
  fp8 functors (src/device/reduce_kernel.h:461-487) and integer functors (:330-357, :936-966)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp8_convert_probe(built):
    exe = os.path.join(ROOT, "tests", "native", "fp8_cvt_probe")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    for fmt in ("e4m3", "e5m2"):
        assert r[f"{fmt}_decode_mismatch"] == 0 and r[f"{fmt}_encode_mismatch"] == 0, r


def test_fp8_packed_half_probe(built):
    """The packed fp8 <-> half converts the packed-half fold runs on (numerics.h fp8DecodeH2 / fp8RoundH2): decode
    exact for every code, clamped encode exact for every non-NaN half (NaN packs take the f32 path)."""
    exe = os.path.join(ROOT, "tests", "native", "fp8_f16_probe")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    for fmt in ("e4m3", "e5m2"):
        assert r[f"{fmt}_decode_mismatch"] == 0 and r[f"{fmt}_encode_clamped_mismatch"] == 0, r


def _pairs(dtype):
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    npdt = np.int8 if dtype == 0 else np.uint8
    return [a.view(npdt), b.view(npdt)]


ONE_BYTE_TYPES = (10, 11, 1, 0)
FORCED_PATHS = ("LL128", "ONESHOT", "REGISTERED", "RING", "TREE")


def _job_one_byte_pairs(path):
    """Every byte pair of the four 1-byte types through a forced path's AllReduce at n = 2 for every operator (a
    spawned worker whose environment forces the path, tests/test_gpu_edge_values.py run_set: slices every forced path
    takes, guarded buffers, the oracle's fold for the path)."""
    from tests.test_gpu_edge_values import comms_under, destroy, run_set, slice_elems
    cs = comms_under(2)
    errs = []
    for dtype in ONE_BYTE_TYPES:
        errs += run_set(cs, "allreduce", dtype, _pairs(dtype), slice_elems(dtype), path == "REGISTERED", path)
    destroy(cs)
    return errs


@pytest.mark.parametrize("proto", ["LL", "^LL", *FORCED_PATHS])
def test_one_byte_every_pair(built, proto, monkeypatch):
    """Every (a, b) byte pair of e4m3 / e5m2 / uint8 / int8, every operator, n = 2. LL and ^LL (the LL kernel and the
    staged kernel, chosen by NCCL_PROTO): AllReduce, ReduceScatter and Reduce to root 1. The other paths — LL128,
    one-shot, the zero-copy kernel on registered buffers, the reference's ring and chain — are forced in a spawned
    worker whose kernel log must name the path's kernel for every element type and operator (integer Avg is
    SumPostDiv, template argument 4; fp8 Avg PreMulSum, 3) and no other kernel of those types."""
    if proto in FORCED_PATHS:
        from tests.test_gpu_edge_values import check_kernel_log
        from tests.test_gpu_premulsum import PATHS, spawn
        (errs, klog, _), = spawn([(_job_one_byte_pairs, proto, PATHS[proto][0])], timeout=150)
        assert not errs, "\n".join(errs[:10])
        for dtype in ONE_BYTE_TYPES:
            check_kernel_log(klog, proto, dtype, (0, 1, 2, 3) if dtype >= 10 else (0, 1, 2, 4), extra=())
        return
    import torch
    import nccl_amd
    from tests import gpu_cases as G
    monkeypatch.setenv("NCCL_PROTO", proto)
    os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
    torch.cuda.set_device(0)
    comms = nccl_amd.Communicator.init_all([0, 0])
    cs = list(zip(comms, [torch.cuda.Stream(), torch.cuda.Stream()]))
    errs = []
    try:
        for dtype in (10, 11, 1, 0):
            ins = _pairs(dtype)
            for op in (0, 1, 2, 3, 4):  # sum, prod, max, min, avg
                errs += G.run_case(cs, "allreduce", dtype, op, ins[0].size, 0, seed=0, inputs=ins)
                errs += G.run_case(cs, "reducescatter", dtype, op, ins[0].size, 0, seed=0, inputs=ins)
                errs += G.run_case(cs, "reduce", dtype, op, ins[0].size, 0, seed=0, inputs=ins, root=1)
    finally:
        for c in comms:
            c.destroy()
    assert not errs, "\n".join(errs[:10])
