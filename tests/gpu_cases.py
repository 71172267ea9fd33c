"""Shared helpers for the GPU parity tests: run a collective through the C ABI (nccl_amd) on torch
device buffers and compare with the CPU oracle. Imported by tests only."""
from __future__ import annotations

import os

import numpy as np

import oracle

# dtype code -> torch dtype name used to allocate raw storage of the same width
TORCH_STORAGE = {0: "int8", 1: "uint8", 2: "int32", 3: "int32", 4: "int64", 5: "int64", 6: "int16", 7: "float32",
                 8: "float64", 9: "int16", 10: "uint8", 11: "uint8"}
FLOAT_TYPES = {6, 7, 8, 9, 10, 11}


def to_device(arr: np.ndarray, device, offset_elems: int = 0):
    """Copy a numpy storage array to a fresh device buffer (device "pinned": pinned host memory, which the kernels
    reach across PCIe); `offset_elems` > 0 returns a view that is deliberately NOT 16-byte aligned (exercises the
    reference's unaligned fallback)."""
    import torch
    raw = np.ascontiguousarray(arr).view(np.uint8)
    es = arr.dtype.itemsize
    if device == "pinned":
        buf = torch.empty(raw.size + offset_elems * es + 64, dtype=torch.uint8, pin_memory=True)
    else:
        buf = torch.empty(raw.size + offset_elems * es + 64, dtype=torch.uint8, device=device)
    view = buf[offset_elems * es: offset_elems * es + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return buf, view


def from_device(view, dtype_np) -> np.ndarray:
    return view.cpu().numpy().view(dtype_np).copy()


def _raw(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a: np.ndarray, b: np.ndarray, dtype: int) -> bool:
    """Bitwise equality of every element — the sign of zero included (+0 and -0 differ) — except NaN payloads: a
    float NaN must sit where the oracle has one, its sign and payload are not compared here. (A NaN generated from
    non-NaN inputs, or two NaNs meeting, is the hardware's: x86 and gfx950 default NaNs differ in sign. The single-NaN
    case is compared bit for bit by test_gpu_collectives.py::test_single_nan_payloads)"""
    if a.shape != b.shape:
        return False
    ua, ub = _raw(a), _raw(b)
    if dtype not in FLOAT_TYPES:
        return np.array_equal(ua, ub)
    na, nb = np.isnan(oracle.to_f32(dtype, a)), np.isnan(oracle.to_f32(dtype, b))
    return bool(np.array_equal(na, nb) and np.array_equal(ua[~na], ub[~na]))


def make_inputs(n: int, dtype: int, count: int, seed: int, kind: int = 0):
    return [oracle.fill(dtype, seed * 131 + r, count, kind) for r in range(n)]


def _env_int(name: str, default: int) -> int:
    v = os.environ.get(name)
    return int(v) if v not in (None, "") else default


def ring_channels(n: int, ranks_per_gpu: int | None = None) -> int:
    """The channel count K a NCCL_ALGO=RING / NCCL_AMD_REF_ORDER AllReduce is planned on (enqueue.cc
    refChannelCount): NCCL_AMD_REF_NCHANNELS when set, else the communicator's co-resident channel cap —
    NCCL_MAX_CTAS / NCCL_MAX_NCHANNELS (default 256) capped at 2 workgroups per CU for one rank per GPU, at CUs
    divided by the ranks per GPU when they share one (enqueue.cc coResidentChannelCap; every test rank shares the box's
    one GPU) — and at most the reference's MAXCHANNELS = 64 (src/include/device.h:91) and the channel cap."""
    import torch
    cap = _env_int("NCCL_MAX_CTAS", _env_int("NCCL_MAX_NCHANNELS", 256))
    cap = max(1, min(cap, 256))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rpg = ranks_per_gpu or n
    cap = max(1, min(cap, 2 * cus if rpg == 1 else cus // rpg))
    k = _env_int("NCCL_AMD_REF_NCHANNELS", 0) or cap
    return max(1, min(k, 64, cap))  # every part needs a workgroup: never more parts than the channel cap


def ring_runs(n: int) -> bool:
    """Whether NCCL_ALGO=RING (from the environment the communicator was created under) runs the ring kernel for
    an AllReduce: two staging slots are needed (enqueue.cc planColl). NCCL_PROTO naming LL or LL128 alone runs the
    ring on that protocol's partition (ref_proto); with several LL-class protocols and no Simple the LL kernel
    takes what fits its line area and the ring the rest, a size rule this helper does not restate: the tests
    never use that combination with NCCL_ALGO=RING (ValueError)."""
    if os.environ.get("NCCL_ALGO", "").upper() != "RING" or n < 2:
        return False
    proto = os.environ.get("NCCL_PROTO", "")
    if proto:
        toks = {t.strip().lower() for t in proto.lstrip("^").split(",")}
        simple = ("simple" not in toks) if proto.startswith("^") else ("simple" in toks)
        if not simple and ref_proto()[0] == oracle.PROTO_SIMPLE:
            raise ValueError(f"NCCL_ALGO=RING with NCCL_PROTO={proto}: the AllReduce order depends on the LL capacity")
    return _env_int("NCCL_AMD_NSLOTS", 2) >= 2


def ref_order_runs(n: int) -> bool:
    """Whether NCCL_AMD_REF_ORDER=1 (from the communicator's environment) puts AllReduce on the reference's ring
    partition (the direct kernel in that order; enqueue.cc planColl): any size and protocol, unless
    NCCL_ALGO=TREE / RING takes the reference's own chain / ring instead."""
    return n >= 2 and _env_int("NCCL_AMD_REF_ORDER", 0) != 0 and \
        os.environ.get("NCCL_ALGO", "").upper() not in ("TREE", "RING")


def ref_proto() -> tuple[int, int]:
    """The protocol whose ring partition NCCL_AMD_REF_ORDER walks and that protocol's buffer size (0 = default):
    LL or LL128 when NCCL_PROTO enables that one protocol alone, Simple otherwise (enqueue.cc loadTuning)."""
    proto = os.environ.get("NCCL_PROTO", "")
    on = {"ll": True, "simple": True, "ll128": _env_int("NCCL_AMD_LL128", 0) != 0}
    if proto:
        excl = proto.startswith("^")
        toks = {t.strip().lower() for t in proto.lstrip("^").split(",")}
        on = {k: ((k not in toks) and (on[k] if k == "ll128" else True)) if excl else (k in toks) for k in on}
        if excl and not on["ll"] and not on["simple"] and "ll128" not in toks:
            on["ll128"] = True  # LL128 at its gate is on when it is the only protocol left (enqueue.cc resolveFuncTuning)
    if on["ll"] and not on["simple"] and not on["ll128"]:
        return oracle.PROTO_LL, _env_int("NCCL_LL_BUFFSIZE", 0)
    if on["ll128"] and not on["ll"] and not on["simple"]:
        return oracle.PROTO_LL128, _env_int("NCCL_LL128_BUFFSIZE", 0)
    return oracle.PROTO_SIMPLE, _env_int("NCCL_BUFFSIZE", 0)


def expected(coll: str, inputs, dtype: int, op: int, root: int = 0, algo: str = "", premul: int | None = None):
    """The oracle's result. `premul`: the storage bits of a user PreMulSum operator's scalar (`op` is then unused)."""
    if coll == "allreduce":
        # NCCL_ALGO=TREE folds every element in the chain's order; NCCL_ALGO=RING in the reference's ring order
        # over its own channel parts and loops (NCCL_MAX_CTAS / NCCL_BUFFSIZE as set for the communicator);
        # every other path in the one-loop ring order
        n = len(inputs)
        algo = algo or os.environ.get("NCCL_ALGO", "").upper()
        if algo == "TREE":
            out = oracle.all_reduce_chain(inputs, dtype, op, premul)
        elif (algo == "RING" and ring_runs(n)) or ref_order_runs(n):
            proto, buff = ref_proto()
            out = oracle.all_reduce_ring_nccl(inputs, dtype, op, ring_channels(n), buff, proto, premul)
        else:
            out = oracle.all_reduce(inputs, dtype, op, premul)
        return [out] * len(inputs)
    if coll == "reducescatter":
        return oracle.reduce_scatter(inputs, dtype, op, premul)
    if coll == "allgather":
        out = oracle.all_gather(inputs)
        return [out] * len(inputs)
    if coll == "reduce":
        return [oracle.reduce(inputs, dtype, op, root, premul)]
    raise ValueError(coll)


def premul_scalars(dtype: int) -> dict[str, int]:
    """The scalars the user PreMulSum tests run, as storage bits of `dtype`. Floats: 1, -1, 0.375 and -2.5 (exact in
    every type), the type's rounding of 1/3 (inexact products), both zeros, the smallest subnormal, the largest
    finite value, +Inf (e4m3 has none) and a quiet NaN. Integers: 0, 1, 3, all ones (-1), the sign bit alone,
    0x55...."""
    L = oracle.lib()
    if dtype not in FLOAT_TYPES:
        bits = 8 * np.dtype(oracle.NP_STORAGE[dtype]).itemsize
        ones = (1 << bits) - 1
        return {"0": 0, "1": 1, "3": 3, "ones": ones, "signbit": 1 << (bits - 1), "0x55": ones // 3}
    vals = {"1": 1.0, "-1": -1.0, "0.375": 0.375, "-2.5": -2.5, "third": 1.0 / 3.0, "+0": 0.0, "-0": -0.0}
    if dtype == 7:
        enc = lambda v: int(np.float32(v).view(np.uint32))
        rest = {"minsub": 0x00000001, "maxfinite": 0x7F7FFFFF, "inf": 0x7F800000, "nan": 0x7FC00000}
    elif dtype == 8:
        enc = lambda v: int(np.float64(v).view(np.uint64))
        rest = {"minsub": 1, "maxfinite": 0x7FEFFFFFFFFFFFFF, "inf": 0x7FF0000000000000, "nan": 0x7FF8000000000000}
    elif dtype == 6:
        enc = lambda v: int(np.float16(v).view(np.uint16))
        rest = {"minsub": 0x0001, "maxfinite": 0x7BFF, "inf": 0x7C00, "nan": 0x7E00}
    elif dtype == 9:
        enc = lambda v: int(L.oracle_f32_to_bf16(float(np.float32(v))))
        rest = {"minsub": 0x0001, "maxfinite": 0x7F7F, "inf": 0x7F80, "nan": 0x7FC0}
    elif dtype == 10:
        enc = lambda v: int(L.oracle_f32_to_fp8(float(np.float32(v)), 0))
        rest = {"minsub": 0x01, "maxfinite": 0x7E, "nan": 0x7F}
    else:
        enc = lambda v: int(L.oracle_f32_to_fp8(float(np.float32(v)), 1))
        rest = {"minsub": 0x01, "maxfinite": 0x7B, "inf": 0x7C, "nan": 0x7E}
    out = {k: enc(v) for k, v in vals.items()}
    out.update(rest)
    return out


def scalar_is_finite(dtype: int, bits: int) -> bool:
    """Whether a PreMulSum scalar (storage bits) is finite; integer scalars always are."""
    if dtype not in FLOAT_TYPES:
        return True
    return bool(np.isfinite(oracle.to_f32(dtype, scalar_array(dtype, bits))[0]))


def scalar_array(dtype: int, bits: int) -> np.ndarray:
    """One element of dtype's storage type holding the storage bits `bits`."""
    npdt = np.dtype(oracle.NP_STORAGE[dtype])
    return np.array([bits], dtype=np.dtype(f"u{npdt.itemsize}")).view(npdt)


def nan_cap_ok(want: np.ndarray, dtype: int) -> bool:
    """The cap on the NaN-by-position rule: at least 90 % of the oracle's own result is non-NaN, hence compared bit
    for bit (asserted for every case whose scalar is finite)."""
    if dtype not in FLOAT_TYPES:
        return True
    return bool(np.isnan(oracle.to_f32(dtype, want)).mean() <= 0.10)


# storage bits, explicit mantissa bits M and exponent bias of the float types edge_inputs builds
_EDGE_FORMAT = {6: (16, 10, 15), 9: (16, 7, 127), 7: (32, 23, 127), 8: (64, 52, 1023)}
EDGE_BLOCKS = 18


def _edge_base(dtype: int) -> np.ndarray:
    """The base list of edge_inputs as storage bits: every fp16 / bf16 pattern; for fp32 / fp64 every sign x every
    exponent field x 16 / 8 mantissas at the edges of the field (all zeros, all ones, around the half, the 0x55...
    patterns, the middle bit)."""
    bits, M, _ = _EDGE_FORMAT[dtype]
    ut = np.dtype(f"u{bits // 8}")
    if bits == 16:
        return np.arange(65536, dtype=ut)
    ones = (1 << M) - 1
    half = 1 << (M - 1)
    mant = [0, 1, 2, ones, ones - 1, half, half - 1, half + 1, ones // 3, 2 * (ones // 3), 1 << (M // 2), ones >> 1,
            3 << (M - 2), 5, ones ^ 5, half | ((ones // 3) >> 1)]
    mant = np.array(mant[:16 if dtype == 7 else 8], dtype=ut)
    sign = np.array([0, 1], dtype=ut) << ut.type(bits - 1)
    expo = np.arange(1 << (bits - 1 - M), dtype=ut) << ut.type(M)
    return (sign[:, None, None] | expo[None, :, None] | mant[None, None, :]).reshape(-1)


_edge_cache: dict = {}


def edge_inputs(dtype: int, n: int):
    """Inputs of n = 2 or 3 ranks (storage arrays of fp16 6, bf16 9, fp32 7 or fp64 8, read-only and shared between
    callers) that pair every value of the base list `a` (_edge_base) with 18 partners chosen for what goes wrong in a
    rounding: rank 0 holds `a` 18 times, rank 1 the 18 blocks
      1 a permutation of a            2 a itself (doubling, squaring: overflow and underflow)
      3 -a (exact cancellation, +-0 meeting in Min / Max)            4 the ulp neighbour (the bits + 1, wrapped)
      5 minus the ulp neighbour (tiny and subnormal exact results)
      6 exactly half an ulp of a, same sign (every Sum a rounding tie)   7 block 6 | 1 (just above the tie)
      8 block 6 negated (the tie from below)
      9 a byte-swapped (16-bit) / reversed (fp32, fp64): large exponents against small ones
      10-18 the constants 1, +-max finite, min subnormal, min normal, -0, +Inf, 1 + 1 ulp and 0.3333... x 2^-1
    and rank 2 holds rank 0's elements at (j * 25173 + 13849) mod length. Signalling NaNs are quieted in every array
    (their handling is the hardware's, tests/test_numerics.py)."""
    if (dtype, n) in _edge_cache:
        return _edge_cache[(dtype, n)]
    assert n in (2, 3)
    bits, M, bias = _EDGE_FORMAT[dtype]
    ut = np.dtype(f"u{bits // 8}")
    U = ut.type
    ones = (1 << M) - 1
    sign = U(1 << (bits - 1))
    emax = (1 << (bits - 1 - M)) - 1
    a = _edge_base(dtype)
    ln = a.size
    s = a & sign
    e = ((a & ~sign) >> U(M)).astype(np.int64)
    # half an ulp of a: a normal number while a's exponent field is at least M + 2, a subnormal power of two below
    # that, the smallest subnormal (the nearest there is) for the two lowest fields
    half = np.where(e >= M + 2, np.maximum(e - (M + 1), 0) << M,
                    np.where(e >= 2, np.int64(1) << np.clip(e - 2, 0, M), 1)).astype(ut) | s
    swapped = a.byteswap() if bits == 16 else a[::-1]
    consts = [bias << M, ((emax - 1) << M) | ones, (1 << (bits - 1)) | ((emax - 1) << M) | ones, 1, 1 << M,
              1 << (bits - 1), emax << M, (bias << M) + 1, ((bias - 2) << M) | (ones // 3)]
    blocks = [a[(np.arange(ln, dtype=np.int64) * 40503) % ln], a, a ^ sign, a + U(1), (a + U(1)) ^ sign, half,
              half | U(1), half ^ sign, swapped] + [np.full(ln, c, dtype=ut) for c in consts]
    assert len(blocks) == EDGE_BLOCKS
    r0 = np.tile(a, EDGE_BLOCKS)
    ranks = [r0, np.concatenate(blocks)]
    if n == 3:
        ranks.append(r0[(np.arange(r0.size, dtype=np.int64) * 25173 + 13849) % r0.size])
    qbit, expm = U(1 << (M - 1)), U(emax << M)
    out = []
    for x in ranks:
        x = np.ascontiguousarray(x, dtype=ut).copy()
        snan = ((x & expm) == expm) & ((x & U(ones)) != 0) & ((x & qbit) == 0)
        x[snan] |= qbit
        x = x.view(oracle.NP_STORAGE[dtype])
        x.setflags(write=False)
        out.append(x)
    _edge_cache[(dtype, n)] = out
    return out


def defined_mask(ins, dtype: int, op: int) -> np.ndarray:
    """The elements of a built-in operator's result over float inputs `ins` whose NaN bits are compared with the
    oracle's as well (same_bits compares NaN by position only): for Sum / Prod / Avg those where exactly one NaN
    arises in the fold (one NaN input, none made from Inf - Inf / 0 x Inf: the rule of test_gpu_collectives.py
    _comparable and _single_nan_errors); Min / Max (explicit selects): every element."""
    from tests.test_gpu_collectives import _comparable
    keep = _comparable(ins, dtype, op)
    if op in (2, 3):
        return keep
    return keep & (np.isnan(np.stack([oracle.to_f32(dtype, x) for x in ins])).sum(0) == 1)


def edge_errors(got: np.ndarray, want: np.ndarray, one: np.ndarray, dtype: int, what: str):
    """Error strings of one result against the oracle's: same_bits over every element, and the elements of `one`
    (defined_mask) bit for bit."""
    errs = []
    g, w = _raw(got), _raw(want)
    if not same_bits(got, want, dtype):
        nan = np.isnan(oracle.to_f32(dtype, want))
        bad = np.nonzero((g != w) & ~(nan & np.isnan(oracle.to_f32(dtype, got))))[0]
        errs.append(f"{what}: {bad.size} of {w.size} elements differ, first at {bad[:5].tolist()} got "
                    f"{[hex(int(v)) for v in g[bad[:3]]]} want {[hex(int(v)) for v in w[bad[:3]]]}")
    if not np.array_equal(g[one], w[one]):
        bad = np.nonzero((g != w) & one)[0]
        errs.append(f"{what}: {bad.size} of {int(one.sum())} elements with a defined NaN differ, first at "
                    f"{bad[:5].tolist()} got {[hex(int(v)) for v in g[bad[:3]]]} want "
                    f"{[hex(int(v)) for v in w[bad[:3]]]}")
    return errs


def out_count(coll: str, n: int, count: int) -> int:
    return {"allreduce": count, "reducescatter": count // n, "allgather": count * n, "reduce": count}[coll]


def launch(comm, coll: str, send_view, recv_view, count: int, dtype: int, op: int, root: int, stream_ptr: int):
    n = comm.nranks
    if coll == "allreduce":
        comm.all_reduce_raw(send_view.data_ptr(), recv_view.data_ptr(), count, dtype, op, stream_ptr)
    elif coll == "reducescatter":
        comm.reduce_scatter_raw(send_view.data_ptr(), recv_view.data_ptr(), count // n, dtype, op, stream_ptr)
    elif coll == "allgather":
        comm.all_gather_raw(send_view.data_ptr(), recv_view.data_ptr(), count, dtype, stream_ptr)
    elif coll == "reduce":
        rp = recv_view.data_ptr() if recv_view is not None else None
        comm.reduce_raw(send_view.data_ptr(), rp, count, dtype, op, root, stream_ptr)


# A compact but broad case list: (collective, dtype, op, count, misalign)
def case_list(n: int, quick: bool = False):
    cases = []
    counts = [1, 5, 4096 + 3, 300_001] if not quick else [5, 70_001]
    for coll in ("allreduce", "reducescatter", "allgather", "reduce"):
        for dtype in (7, 9, 6, 2, 3, 4, 0, 1, 5, 8, 10, 11):
            ops = [0] if coll == "allgather" else [0, 1, 2, 3, 4]
            for op in ops:
                if quick and dtype not in (7, 9, 2) and op != 0:
                    continue
                for count in counts:
                    if coll == "reducescatter":
                        count = max(1, count // n) * n
                    cases.append((coll, dtype, op, count, 0))
        cases.append((coll, 7, 0, 100_003 * n, 1))   # misaligned base pointers
        cases.append((coll, 9, 0, 10_001 * n, 3))
    return cases


def run_case(comms_and_streams, coll, dtype, op, count, misalign, seed, inplace=False, root=0, sync=True,
             inputs=None, algo="", host=False, user_ops=None, premul=None):
    """Run one collective on every (comm, stream) of this process; returns list of error strings.
    A user PreMulSum operator: `user_ops` maps each rank to its communicator's op handle and `premul` holds the
    scalar's storage bits for the oracle (`op` is then unused).
    `comms_and_streams` holds the ranks owned by this process: [(comm, torch stream), ...]; the
    inputs of ALL ranks are regenerated deterministically so each process can check its own ranks.
    `host` (a bool, or one per rank): that rank's buffers are pinned host memory."""
    import torch
    n = comms_and_streams[0][0].nranks
    if inputs is None:
        inputs = make_inputs(n, dtype, count, seed)
    exp = expected(coll, inputs, dtype, op, root, algo, premul)
    npdt = oracle.NP_STORAGE[dtype]
    es = np.dtype(npdt).itemsize
    ocount = out_count(coll, n, count)
    keep, views = [], []
    per_rank = misalign if isinstance(misalign, (list, tuple)) else None
    for comm, stream in comms_and_streams:
        r = comm.rank
        if per_rank is not None:  # each rank's buffers misaligned differently (protocol choice must not care)
            misalign = per_rank[r % len(per_rank)]
        dev = torch.device("cuda", comm.device)
        on_host = host[r % len(host)] if isinstance(host, (list, tuple)) else host
        with torch.cuda.device(dev):
            if on_host:
                dev = "pinned"
            if inplace:
                # one buffer: AR send==recv; RS recv = send + r*recvcount; AG send = recv + r*sendcount
                if coll in ("allreduce", "reduce"):
                    buf, sv = to_device(inputs[r], dev, misalign)
                    rv = sv
                elif coll == "reducescatter":
                    buf, sv = to_device(inputs[r], dev, misalign)
                    rc = count // n
                    rv = sv[r * rc * es:(r + 1) * rc * es]
                else:  # allgather
                    full = np.zeros(count * n, dtype=npdt)
                    full[r * count:(r + 1) * count] = inputs[r]
                    buf, rv = to_device(full, dev, misalign)
                    sv = rv[r * count * es:(r + 1) * count * es]
                keep.append(buf)
            else:
                b1, sv = to_device(inputs[r], dev, misalign)
                rv = None
                if coll != "reduce" or r == root:
                    b2, rv = to_device(np.zeros(ocount, dtype=npdt), dev, misalign)
                    keep.append(b2)
                keep.append(b1)
            views.append((comm, stream, sv, rv))
    import nccl_amd
    torch.cuda.synchronize()
    with nccl_amd.group():
        for comm, stream, sv, rv in views:
            launch(comm, coll, sv, rv, count, dtype, user_ops[comm.rank] if user_ops else op, root,
                   stream.cuda_stream)
    errs = []
    for comm, stream, sv, rv in views:
        stream.synchronize()
        ae = comm.async_error()
        if ae != 0:
            errs.append(f"rank {comm.rank}: async error {ae}")
            continue
        r = comm.rank
        if coll == "reduce" and r != root:
            continue
        got = from_device(rv, npdt)
        want = exp[0] if coll == "reduce" else exp[r]
        if not same_bits(got, want, dtype):
            bad = np.nonzero(got != want)[0]
            errs.append(f"rank {r} {coll} dt={dtype} op={op} count={count} mis={misalign} inplace={inplace}: "
                        f"{bad.size} mismatches, first at {bad[:5].tolist()} got {got[bad[:3]].tolist()} "
                        f"want {want[bad[:3]].tolist()}")
    return errs


def run_group(comms_and_streams, ops, seed):
    """Several collectives [(coll, dtype, op, count), ...] issued inside ONE group (so consecutive ops that plan
    onto the same kernel are batched into one launch), out of place, checked bit-exactly; returns errors."""
    import torch
    import nccl_amd
    n = comms_and_streams[0][0].nranks
    plan = []
    for k, (coll, dtype, op, count) in enumerate(ops):
        inputs = make_inputs(n, dtype, count, seed * 100 + k)
        exp = expected(coll, inputs, dtype, op, 0)
        npdt = oracle.NP_STORAGE[dtype]
        bufs = {}
        for comm, _ in comms_and_streams:
            dev = torch.device("cuda", comm.device)
            b1, sv = to_device(inputs[comm.rank], dev, 0)
            b2, rv = to_device(np.zeros(out_count(coll, n, count), dtype=npdt), dev, 0)
            bufs[comm.rank] = (b1, sv, b2, rv)
        plan.append((coll, dtype, op, count, exp, npdt, bufs))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for coll, dtype, op, count, _, _, bufs in plan:
            for comm, stream in comms_and_streams:
                _, sv, _, rv = bufs[comm.rank]
                launch(comm, coll, sv, rv, count, dtype, op, 0, stream.cuda_stream)
    errs = []
    for comm, stream in comms_and_streams:
        stream.synchronize()
        if comm.async_error():
            errs.append(f"rank {comm.rank}: async error {comm.async_error()}")
    for k, (coll, dtype, op, count, exp, npdt, bufs) in enumerate(plan):
        for comm, _ in comms_and_streams:
            if coll == "reduce" and comm.rank != 0:
                continue
            got = from_device(bufs[comm.rank][3], npdt)
            want = exp[0] if coll == "reduce" else exp[comm.rank]
            if not same_bits(got, want, dtype):
                bad = np.nonzero(got != want)[0]
                errs.append(f"group op {k} rank {comm.rank} {coll} dt={dtype} op={op} count={count}: "
                            f"{bad.size} mismatches, first at {bad[:5].tolist()}")
    return errs


# ---------------------------------------------------------------------------------------------- boundary counts
# Counts derived from the plan: where enqueue.cc cuts a buffer into rank blocks, channel parts, pipeline slices, LL
# lines and ring loops (tests/test_boundaries_cpu.py checks every claim against tests/native/plan_test;
# tests/test_gpu_boundaries.py runs the counts through guarded arenas). Pure Python arithmetic, no torch and no GPU.
#
# BOUNDARY_ENVS is the geometry table: every path's communicator environment, small enough that every boundary falls
# within PAYLOAD_CAP bytes per rank. NCCL_MAX_CTAS is set on every path: it is the channel cap whatever the GPU's CU
# count (init.cc computeChannelCap), so the counts do not depend on the device. Values adjusted where the planner
# clamps:
#   LL       NCCL_AMD_LL_CHANNEL_BYTES=32 with 4 channels: with 8 payloads per channel the last of 4 channels never
#            holds one line alone (part = ceil(units / 4) leaves the last channel at least part - 3 units); 4 channels
#            x 2048 lines x 8 bytes = 64 KiB of LL capacity, inside the payload cap for every collective
#   LL128    4 channels x 512 lines x 56 bytes = 112 KiB of capacity
#   ONESHOT  slots of 4096 bytes, so that the step classes fall inside the cap as on the direct path
#   WINDOW   NCCL_AMD_MIN_CHANNEL_BYTES=16 (one pack): the symmetric cut has no slices, and a last part of one element
#            needs parts of at most as many packs as there are channels
#   REF_SUB  NCCL_AMD_REF_NCHANNELS=2 below the 5 workgroups with NCCL_AMD_MIN_CHANNEL_BYTES=512: two workgroups share
#            each reference part (enqueue.cc refSubCount)
#   TABLE    the default algorithm with the size-table crossovers at 2 KiB (LL), 8 KiB (LL128) and 16 KiB (one-shot)
PAYLOAD_CAP = 256 << 10
_B_DIRECT = {"NCCL_ALGO": "DIRECT", "NCCL_PROTO": "Simple", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2",
             "NCCL_MAX_CTAS": "3", "NCCL_AMD_MIN_CHANNEL_BYTES": "512"}
_B_REF = {"NCCL_BUFFSIZE": "16384", "NCCL_MAX_CTAS": "5"}
BOUNDARY_ENVS = {
    "DIRECT": dict(_B_DIRECT),
    "PULLS_AG0": dict(_B_DIRECT, NCCL_AMD_RS_PULL="1", NCCL_AMD_AG_PULL="0"),
    "PULLS_AG1": dict(_B_DIRECT, NCCL_AMD_RS_PULL="1", NCCL_AMD_AG_PULL="1"),
    "ONESHOT": {"NCCL_ALGO": "ONESHOT", "NCCL_AMD_ONESHOT_CHANNEL_BYTES": "512", "NCCL_AMD_SLOT_BYTES": "4096",
                "NCCL_AMD_NSLOTS": "2", "NCCL_MAX_CTAS": "3"},
    "LL": {"NCCL_PROTO": "LL", "NCCL_AMD_LL_CHANNEL_BYTES": "32", "NCCL_MAX_CTAS": "4"},
    "LL128": {"NCCL_PROTO": "LL128", "NCCL_AMD_LL128_CHANNEL_BYTES": "56", "NCCL_MAX_CTAS": "4"},
    "RING": dict(_B_REF, NCCL_ALGO="RING"),
    "TREE": dict(_B_REF, NCCL_ALGO="TREE"),
    "REF_ORDER": dict(_B_REF, NCCL_AMD_REF_ORDER="1"),
    "REF_SUB": dict(_B_REF, NCCL_AMD_REF_ORDER="1", NCCL_AMD_REF_NCHANNELS="2", NCCL_AMD_MIN_CHANNEL_BYTES="512"),
    "WINDOW": {"NCCL_PROTO": "Simple", "NCCL_AMD_MIN_CHANNEL_BYTES": "16", "NCCL_MAX_CTAS": "3"},
    "WINDOW_ONESHOT": {"NCCL_PROTO": "Simple", "NCCL_AMD_MIN_CHANNEL_BYTES": "16", "NCCL_MAX_CTAS": "3",
                       "NCCL_AMD_SYM_ONESHOT": "1", "NCCL_AMD_ONESHOT_CHANNEL_BYTES": "16"},
    "TABLE": {"NCCL_AMD_LL128": "1", "NCCL_AMD_LL_BYTES": "2048", "NCCL_AMD_LL128_BYTES": "8192",
              "NCCL_AMD_ONESHOT_BYTES": "16384", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2",
              "NCCL_MAX_CTAS": "3"},
}
BOUNDARY_WINDOW_PATHS = ("WINDOW", "WINDOW_ONESHOT")   # buffers in symmetric windows
_ALL4 = ("allreduce", "reducescatter", "allgather", "reduce")
BOUNDARY_COLLS = {
    "DIRECT": _ALL4, "PULLS_AG0": _ALL4, "PULLS_AG1": _ALL4, "ONESHOT": ("allreduce",), "LL": _ALL4, "LL128": _ALL4,
    "RING": _ALL4,   # (Reduce under NCCL_ALGO=RING is the chain to the root)
    "TREE": ("allreduce",), "REF_ORDER": ("allreduce",), "REF_SUB": ("allreduce",),
    "WINDOW": ("allreduce", "reducescatter", "allgather"), "WINDOW_ONESHOT": ("allreduce",), "TABLE": ("allreduce",),
}
_PLAN_FUNC = {"allreduce": "ar", "reducescatter": "rs", "allgather": "ag", "reduce": "reduce"}
_DTYPE_OF_SIZE = {1: 1, 2: 6, 4: 2, 8: 8}   # uint8, fp16, int32, fp64: the GPU tests' type per element size
STEP_CLASSES = {"steps=1": lambda ns: 1, "steps=NSLOTS": lambda ns: ns, "steps=NSLOTS+1": lambda ns: ns + 1,
                "steps=2NSLOTS+1": lambda ns: 2 * ns + 1}


def _up(x: int, m: int) -> int:
    return -(-x // m) * m


class _Geom:
    """What init.cc commDefaults and enqueue.cc loadTuning read from a path's environment."""

    def __init__(self, path: str, n: int):
        e = BOUNDARY_ENVS[path]
        gi = lambda k, d: int(e.get(k, d))
        self.path, self.n = path, n
        self.cap = max(1, min(gi("NCCL_MAX_CTAS", 256), 256))       # chanCap: below CUs / n on any GPU of the suite
        self.nslots = max(1, gi("NCCL_AMD_NSLOTS", 2))
        sb = (1024 << 20) // (self.cap * 2 * self.nslots * max(n, 2))
        sb = max(16 << 10, min(sb, 1 << 20))
        if gi("NCCL_BUFFSIZE", 0):
            sb = gi("NCCL_BUFFSIZE", 0) // self.nslots
        self.slot = max(4096, _up(gi("NCCL_AMD_SLOT_BYTES", sb), 4096))
        proto = e.get("NCCL_PROTO", "")
        self.ll_on = proto in ("", "LL")
        self.ll128_on = proto == "LL128" or (proto == "" and gi("NCCL_AMD_LL128", 0) != 0)
        self.simple_on = proto in ("", "Simple")
        self.algo = e.get("NCCL_ALGO", "")
        self.ref_order = gi("NCCL_AMD_REF_ORDER", 0) != 0
        self.ref_k = max(1, min(gi("NCCL_AMD_REF_NCHANNELS", 0) or self.cap, 64, self.cap))
        self.ref_chunk_bytes = max(512, gi("NCCL_BUFFSIZE", 4 << 20) // 8 * 4 // 512 * 512)
        self.window = path in BOUNDARY_WINDOW_PATHS
        self.sym_oneshot = gi("NCCL_AMD_SYM_ONESHOT", 0) != 0
        self.min_channel = gi("NCCL_AMD_MIN_CHANNEL_BYTES", 16 << 10)
        self.oneshot_channel = gi("NCCL_AMD_ONESHOT_CHANNEL_BYTES", 16 << 10)
        self.ll_channel = max(8, gi("NCCL_AMD_LL_CHANNEL_BYTES", 4096))
        self.ll128_channel = max(56, gi("NCCL_AMD_LL128_CHANNEL_BYTES", 4096))
        self.ll_lim = gi("NCCL_AMD_LL_BYTES", 0) or max(16 << 10, (256 << 10) // n)
        self.ll128_lim = gi("NCCL_AMD_LL128_BYTES", 0) or max(64 << 10, (1 << 20) // n)
        self.oneshot_lim = gi("NCCL_AMD_ONESHOT_BYTES", 0) or ((2 << 20) if n == 2 else (2 << 20) // n)
        self.ll_channels, self.ll_bytes = 32, 32 << 10               # core.h: LL channels and line bytes


_geoms: dict = {}


def boundary_geom(path: str, n: int) -> "_Geom":
    if (path, n) not in _geoms:
        _geoms[(path, n)] = _Geom(path, n)
    return _geoms[(path, n)]


def _ring_parts(count: int, ts: int, K: int, n: int):
    """enqueue.cc ringParts for the Simple protocol: (parts, cbdLo, mid, cbdHi)."""
    nbytes = count * ts
    nc = K
    while nc >= 2 and nbytes < nc * 512 * 64:
        nc -= 1
    tpb = 2
    cell = _up((32 << 10) // tpb, 16)
    traffic_cell = tpb * cell
    epc = cell // ts
    cells = -(-nbytes // cell)
    traffic = max(32 << 10, tpb * nbytes)
    per_channel = _up(traffic // nc, 16)
    per_channel_cells = -(-per_channel // traffic_cell)
    cells_per = min(cells, per_channel_cells)
    cells_lo = cells if K == 1 else min(cells, per_channel_cells)
    n_mid = (cells - cells_lo) // cells_per
    cells_hi = (cells - cells_lo) % cells_per
    if K < (1 if cells_lo else 0) + n_mid + (1 if cells_hi else 0):
        n_mid = K - 2
        cells_per = (cells - cells_lo) // (n_mid + 1)
        cells_hi = cells_per + (cells - cells_lo) % (n_mid + 1)
    if cells_hi == 0 and n_mid != 0:
        cells_hi = cells_per
        n_mid -= 1
    lo, mid, hi = cells_lo * epc, (cells_per * epc if n_mid else 0), cells_hi * epc
    pad = cells * epc - count
    if hi:
        hi -= pad
    else:
        lo -= pad
    return (1 if lo else 0) + n_mid + (1 if cells_hi else 0), lo, mid, hi


def _plan_channels(g, block_bytes, es, min_part, max_ch):
    """enqueue.cc planChannels."""
    epp = 16 // es
    nch = max(1, min(-(-block_bytes // max(min_part, 16)), max_ch, g.cap))
    part = _up(-(-(block_bytes // es) // nch), epp) or epp
    sl = min(g.slot // es // epp * epp, part)
    return {"nch": nch, "part": part, "slice": sl, "steps": -(-part // sl)}


def _ll_plan(g, coll, n, es, c):
    """enqueue.cc llPlan: None where the op leaves the LL kernel."""
    nbytes = c * es
    npk, nlines = -(-nbytes // 8), -(-nbytes // 56)
    blocked = coll in ("reducescatter", "allgather")
    shape = not blocked or nbytes % 8 == 0
    fits = g.ll_on and shape and npk <= g.ll_channels * (g.ll_bytes // 16)
    fits64 = g.ll128_on and shape and nlines <= g.ll_channels * (g.ll_bytes // 64)
    sized = g.algo == ""
    proto = None
    if not g.simple_on:
        if fits and (nbytes <= g.ll_lim or not fits64):
            proto = "ll"
        elif fits64:
            proto = "ll128"
    elif fits and sized and nbytes <= g.ll_lim:
        proto = "ll"
    elif fits64 and sized and nbytes <= g.ll128_lim:
        proto = "ll128"
    if proto is None:
        return None
    units, line = (npk, 16) if proto == "ll" else (nlines, 64)
    per = g.ll_channel // 8 if proto == "ll" else g.ll128_channel // 56
    nch = max(1, min(-(-units // per), g.ll_channels, g.cap))
    part = -(-units // nch)
    if part * line > g.ll_bytes:
        return None
    nch = -(-units // part)
    epp = 16 // es
    chunk = _up(-(-c // n), epp) if coll == "allreduce" else c
    return {"algo": proto, "nch": nch, "part": part, "slice": 0, "steps": 1, "chunk": chunk or epp}


def model_plan(path: str, coll: str, n: int, es: int, c: int) -> dict:
    """The plan enqueue.cc planColl makes for one call of `c` elements (ReduceScatter: per rank) under the path's
    environment, with the keys tests/native/plan_test prints."""
    g = boundary_geom(path, n)
    epp = 16 // es
    nb = n - 1 if coll == "reduce" and n >= 3 else n
    block = _up(-(-c // nb), epp) if coll in ("allreduce", "reduce") else c
    ar = coll == "allreduce"
    one_shot = ar and (g.algo == "ONESHOT" or (g.algo == "" and c * es <= g.oneshot_lim))
    ref_order = g.ref_order and ar and g.algo not in ("RING", "TREE")
    if ref_order:
        one_shot = False
    if not ref_order:
        ll = _ll_plan(g, coll, n, es, c)
        if ll:
            return ll
    ref = None
    if ref_order or (g.algo == "RING" and ar):
        parts, lo, mid, hi = _ring_parts(c, es, g.ref_k, n)
        chunk = g.ref_chunk_bytes // es
        max_part = max(lo, mid, hi)
        ck = min(chunk, _up(-(-max_part // n), epp))
        sub = max(1, min(g.cap // max(parts, 1), ck // max(epp, g.min_channel // es)))
        ref = {"nch": parts * sub, "part": mid, "slice": min(chunk, g.slot // es // epp * epp), "steps": 0,
               "chunk": chunk, "cbdlo": lo, "cbdhi": hi, "refnch": parts, "sub": sub}
    if g.algo in ("RING", "TREE") and not (g.algo == "TREE" and not ar):
        if ar and g.algo == "RING":
            return dict(ref, algo="ring", kind=0)
        kind = 3 if ar else {"reducescatter": 1, "allgather": 2, "reduce": 4}[coll]
        chain = kind in (3, 4)
        p = _plan_channels(g, (c if chain else block) * es, es, g.min_channel, g.cap)
        return dict(p, algo="chain" if chain else "ring", kind=kind, chunk=c if chain else block, cbdlo=0, cbdhi=0,
                    refnch=p["nch"], sub=1)
    if ref_order:
        return dict(ref, algo="direct")
    if g.window and coll != "reduce":
        ar1 = ar and one_shot and g.sym_oneshot
        span, min_part, max_ch = block * es, g.min_channel, g.cap
        if ar1:
            span, min_part, max_ch = c * es, g.oneshot_channel, min(g.cap, 32)
        nch = max(1, min(-(-span // min_part), max_ch))
        part = _up(-(-(span // es) // nch), epp) or epp
        return {"algo": "sym", "nch": nch, "part": part, "slice": 0, "steps": 1, "chunk": block,
                "symcoll": 1 if ar1 else {"allreduce": 0, "reducescatter": 2, "allgather": 3}[coll]}
    if one_shot:
        p = _plan_channels(g, c * es, es, g.oneshot_channel, 32)
        return dict(p, algo="oneshot", chunk=block, cbdlo=0, cbdhi=0, refnch=p["nch"], sub=1)
    p = _plan_channels(g, block * es, es, g.min_channel, g.cap)
    return dict(p, algo="direct", chunk=block, cbdlo=0, cbdhi=0, refnch=p["nch"], sub=1)


def _ref_parts(p):
    """The element counts of a reference partition's parts, as kernels.h refInit / pipe.h walk them."""
    k = p["refnch"]
    return [p["cbdlo"] if i == 0 else p["cbdhi"] if i == k - 1 else p["part"] for i in range(k)]


def classify(path: str, coll: str, n: int, es: int, c: int, plan_of) -> set:
    """The boundary classes a call of `c` elements belongs to, recomputed from plans: `plan_of(c)` is the plan of a
    count (model_plan, or what tests/native/plan_test printed). Classes that compare two adjacent counts look at c + 1
    and hold for the lower count of the pair."""
    g = boundary_geom(path, n)
    p = plan_of(c)
    nxt = plan_of(c + pair_step(path, coll, es))
    epp = 16 // es
    algo = p["algo"]
    out = set()
    # elements and packs
    if c == 1:
        out.add("count=1")
    if c < n:
        out.add("count<n")
    if (c * es) % 16:
        out.add("not a pack multiple")
    if c > epp and c % epp == epp - 1:
        out.add("pack-1")
    if c > epp and c % epp == 1:
        out.add("pack+1")
    sym1 = algo == "sym" and p.get("symcoll") == 1
    pipe_ar = algo == "ring" and p.get("kind") == 0
    refpart = pipe_ar or (algo == "direct" and g.ref_order and coll == "allreduce")
    # rank blocks of AllReduce and Reduce (the LL Reduce sends whole lines to the root: no blocks)
    blocks = coll in ("allreduce", "reduce") and not refpart and not sym1 and algo in ("direct", "ll", "ll128", "sym") \
        and not (coll == "reduce" and algo in ("ll", "ll128"))
    chunk = p["chunk"]
    if blocks:
        nb = n - 1 if coll == "reduce" and n >= 3 else n
        last = c - (nb - 1) * chunk
        if last <= 0:
            out.add("last block empty")
        if last == 0:
            out.add("last block empty, the others full")
        if last == 1:
            out.add("last block 1")
        if last == epp - 1:
            out.add("last block pack-1")
    # channel parts and slices of the staged and zero-copy plans (not of the plans an LL path's counts fall off to)
    if algo in ("direct", "oneshot", "sym", "chain", "ring") and not refpart and path not in ("LL", "LL128"):
        whole = algo in ("oneshot", "chain") or sym1      # one block: the whole buffer
        span = c if whole else chunk
        L = c if whole or coll in ("reducescatter", "allgather") else c - ((c - 1) // chunk) * chunk
        nch, part = p["nch"], p["part"]
        c_last = (L - 1) // part
        piece = L - c_last * part                          # what the last channel with data holds of the last block
        if nxt and nxt["algo"] == algo and nxt["nch"] == nch + 1:
            out.add(f"nch {nch}->{nch + 1}")
        if nch > 1 and c_last < nch - 1:
            out.add("last part empty")
        if nch > 1 and c_last == nch - 1 and piece == 1:
            out.add("last part 1")
        nb_ = 1 if whole or coll in ("reducescatter", "allgather") else (n - 1 if coll == "reduce" and n >= 3 else n)
        if nch > 1 and part * nch == span and c == nb_ * span:   # several channels tile every (full) block exactly
            out.add("part x nch = block")
        if algo != "sym":
            for name, f in STEP_CLASSES.items():
                if p["steps"] == f(g.nslots):
                    out.add(name)
            sl = p["slice"]
            tail = piece - ((piece - 1) // sl) * sl
            if piece > sl and tail == 1:
                out.add("last slice 1")
            if p["steps"] > g.nslots and piece == part and tail == sl:   # a part that wraps the slots, ending full
                out.add("last slice full")
    # LL lines
    if algo in ("ll", "ll128"):
        nbytes = c * es
        unit = 8 if algo == "ll" else 56
        units = -(-nbytes // unit)
        if algo == "ll":
            out.add(f"LL bytes mod 8 = {nbytes % 8}")
        elif nbytes % 56 in (0, 1, 55):
            out.add(f"LL128 bytes mod 56 = {nbytes % 56}")
        if p["nch"] > 1 and units - (p["nch"] - 1) * p["part"] == 1:
            out.add("last LL channel one line")
        if coll in ("reducescatter", "allgather"):
            out.add("LL block multiple of 8")
        if nxt and nxt["algo"] not in ("ll", "ll128") and path in ("LL", "LL128"):
            out.add("LL capacity: last inside")
    elif path in ("LL", "LL128"):
        if coll in ("reducescatter", "allgather") and (c * es) % 8:
            out.add("LL block not a multiple of 8")
        else:
            out.add("LL capacity: beyond")
    # size-table crossovers (the default algorithm): the last count of a range
    if path == "TABLE" and nxt and nxt["algo"] != algo:
        out.add(f"crossover {algo}->{nxt['algo']}")
    # the reference's partition
    if refpart:
        G = p["sub"]
        loop = n * chunk
        parts = _ref_parts(p)
        if p["cbdlo"] == 1:
            out.add("ref cbdLo 1")
        if p["refnch"] > 1 and p["cbdhi"] == 1:
            out.add("ref cbdHi 1")
        if p["cbdhi"] == 0:
            out.add("ref cbdHi empty")                     # (one part: cbdLo holds everything)
        for cnt in parts:
            if cnt == 0:
                continue
            rem = cnt % loop
            if rem == 0:
                out.add("ref rem=0")
            for name, v in (("1", 1), ("n-1", n - 1), ("n", n)):
                if rem == v:
                    out.add(f"ref rem={name}")
            lens = []
            if cnt >= loop:
                lens.append((chunk, _up(-(-chunk // G), epp), [chunk] * n))
            if rem:
                ck = _up(-(-rem // n), epp)
                lens.append((ck, _up(-(-ck // G), epp), [max(0, min(ck, rem - b * ck)) for b in range(n)]))
            for ck, sc, blens in lens:
                if any(0 < b < epp for b in blens):
                    out.add("ref last-loop chunk below a pack")
                if G > 1 and any(0 < b <= (G - 1) * sc for b in blens):
                    out.add("ref sub-chunk empty for the last workgroup")
    return out


def pair_step(path: str, coll: str, es: int) -> int:
    """The distance to the upper count of a pair class ("nch k->k+1", "LL capacity: last inside", "crossover"): the
    next call count, on the LL paths' blocked collectives the next whose rank block is a multiple of 8 bytes."""
    return max(1, 8 // es) if path in ("LL", "LL128") and coll in ("reducescatter", "allgather") else 1


def _signature(p: dict, n: int):
    """What changes where a plan of n ranks crosses a boundary (the counts next to a change are the candidates)."""
    sig = [p["algo"], p["nch"], p["steps"], p.get("sub", 1), p.get("refnch", 0)]
    if "cbdlo" in p and (p.get("cbdlo") or p.get("cbdhi")):
        loop = max(1, n * p["chunk"])
        sig += [x // loop for x in _ref_parts(p)] + [p["cbdhi"] == 0]
    return tuple(sig)


_bc_cache: dict = {}


def call_count_cap(coll: str, n: int, es: int) -> int:
    """The largest per-call count whose payload stays within PAYLOAD_CAP bytes per rank."""
    return PAYLOAD_CAP // (es * (n if coll in ("reducescatter", "allgather") else 1))


def boundary_call_counts(path: str, coll: str, n: int, es: int):
    """[(call count, classes)]: per-call element counts (ReduceScatter: recvcount) chosen so that every boundary class
    the model reaches on (path, collective, n, element size) is claimed by at least one count."""
    key = (path, coll, n, es)
    if key in _bc_cache:
        return _bc_cache[key]
    g = boundary_geom(path, n)
    epp = 16 // es
    cmax = call_count_cap(coll, n, es)
    plans: dict = {}

    def plan_of(c):
        if c < 1 or c > cmax + pair_step(path, coll, es):
            return None
        if c not in plans:
            plans[c] = model_plan(path, coll, n, es, c)
        return plans[c]

    step = pair_step(path, coll, es)   # (an LL path's blocked collectives: the plan of the 8-byte multiple below)
    sig = lambda c: _signature(plan_of(c - c % step if c >= step else c), n)
    # change points of the plan's signature: a coarse grid, then bisection between grid points that differ
    grid = sorted(set([1, cmax] + [max(1, cmax * i // 256) for i in range(1, 256)]))
    changes = []
    for lo, hi in zip(grid, grid[1:]):
        while sig(lo) != sig(hi):
            a, b = lo, hi
            while b - a > 1:
                m = (a + b) // 2
                if sig(m) != sig(lo):
                    b = m
                else:
                    a = m
            changes.append(b)
            lo = b
    W = n * epp * (g.cap + 1) + 8
    cand = set(range(1, min(cmax, max(W, 128 // es + 2)) + 1)) | set(range(max(1, cmax - W), cmax + 1))
    for m in changes:
        cand.update(range(max(1, m - W), min(cmax, m + W) + 1))
    by_class: dict = {}
    for c in sorted(cand):
        for k in classify(path, coll, n, es, c, plan_of):
            by_class.setdefault(k, []).append(c)
    chosen: dict = {}
    width = lambda c: (plan_of(c)["nch"], plan_of(c)["steps"])
    for k in sorted(by_class):
        # two representatives of each class: the smallest count, and the smallest among those planned on the most
        # channels and steps the class occurs with (the same count where the class occurs once); a count already
        # chosen is reused where one fits
        top = max(width(c) for c in by_class[k])
        for pool in (by_class[k], [c for c in by_class[k] if width(c) == top]):
            hit = [c for c in pool if c in chosen]
            c = hit[0] if hit else pool[0]
            chosen.setdefault(c, set()).add(k)
            if k.startswith(("nch ", "LL capacity: last", "crossover ")):     # the upper count of the pair
                chosen.setdefault(c + pair_step(path, coll, es), set())
    out = [(c, frozenset(ks)) for c, ks in sorted(chosen.items())]
    _bc_cache[key] = out
    return out


def boundary_counts(path: str, coll: str, n: int, dtype: int):
    """[(count, classes)] in this module's count convention (run_case, launch: a ReduceScatter count is the whole
    sendbuff, a multiple of n): the boundary counts of one collective on one path's geometry for `dtype`'s element
    size, each with the classes it claims (classify names them). Every count carries at most PAYLOAD_CAP bytes per
    rank."""
    es = np.dtype(oracle.NP_STORAGE[dtype]).itemsize
    mul = n if coll == "reducescatter" else 1
    return [(c * mul, ks) for c, ks in boundary_call_counts(path, coll, n, es)]


def reachable_classes(path: str, coll: str, n: int, es: int) -> set:
    """The classes boundary_call_counts must reach on (path, collective, n, element size): every class of the list in
    classify that the path's plan can produce within PAYLOAD_CAP. What is left out, and why:
      * "last part empty" / "last part 1" on the staged paths (DIRECT, PULLS, ONESHOT, RING, TREE): a channel is added
        per 512 bytes (16 KiB on RING / TREE) of a block and the last block of an AllReduce is less than n packs
        short of a full one, so every channel holds data; reachable on the windows' one-pack parts;
      * "steps=2NSLOTS+1" on the ring ReduceScatter / AllGather: their parts stay below 16 KiB x 2 (two 8 KiB slots
        each step) until the five channels are used up, and 5 x 4 slots of a block exceed the payload cap;
      * "last slice full" (a part of more than NSLOTS steps whose last slice is a whole slot) on the ring
        ReduceScatter / AllGather at n = 3: five parts of three 8 KiB slots are 120 KiB of block, above cap / 3;
      * LL payload residues that the element size cannot produce; blocks off 8 bytes for 8-byte elements;
      * the LL128 capacity (112 KiB per rank block) on its ReduceScatter / AllGather at n = 3: above the payload cap;
      * "ref cbdHi 1" on REF_SUB: its two parts split the cells evenly; a cbdLo that is empty: ringParts gives the
        first part at least one cell; "ref sub-chunk empty" where one workgroup serves each part (RING, REF_ORDER);
      * TABLE claims the crossovers only (what else its counts hit is incidental)."""
    g = boundary_geom(path, n)
    out = {"count=1", "count<n", "not a pack multiple", "pack-1", "pack+1"}
    blocks = {"last block empty", "last block empty, the others full", "last block 1", "last block pack-1"}
    parts = {f"nch {k}->{k + 1}" for k in range(1, g.cap)} | {"part x nch = block"}
    slices = set(STEP_CLASSES) | {"last slice 1", "last slice full"}
    if path in ("DIRECT", "PULLS_AG0", "PULLS_AG1"):
        out |= parts | slices | (blocks if coll in ("allreduce", "reduce") else set())
    elif path == "ONESHOT" or path == "TREE" or (path == "RING" and coll == "reduce"):
        out |= parts | slices
    elif path == "RING" and coll in ("reducescatter", "allgather"):
        out |= parts | (slices - {"steps=2NSLOTS+1"}) - ({"last slice full"} if n == 3 else set())
    elif path in ("RING", "REF_ORDER", "REF_SUB"):
        out |= {"ref cbdLo 1", "ref cbdHi empty", "ref rem=0", "ref rem=1", "ref rem=n-1", "ref rem=n",
                "ref last-loop chunk below a pack"}
        out |= {"ref sub-chunk empty for the last workgroup"} if path == "REF_SUB" else {"ref cbdHi 1"}
    elif path in ("WINDOW", "WINDOW_ONESHOT"):
        out |= parts | {"last part 1", "last part empty"}
        if path == "WINDOW" and coll == "allreduce":
            out |= blocks
    elif path in ("LL", "LL128"):
        out |= {"last LL channel one line", "LL capacity: beyond", "LL capacity: last inside"}
        if coll == "allreduce":
            out |= blocks
        if coll in ("reducescatter", "allgather"):
            out |= {"LL block multiple of 8"} | ({"LL block not a multiple of 8"} if es < 8 else set())
            out.add("LL bytes mod 8 = 0" if path == "LL" else "LL128 bytes mod 56 = 0")
            if path == "LL128" and n == 3:
                out -= {"LL capacity: beyond", "LL capacity: last inside"}
        elif path == "LL":
            out |= {f"LL bytes mod 8 = {r}" for r in range(0, 8, es)}
        else:
            out |= {f"LL128 bytes mod 56 = {r}" for r in ((0, 1, 55) if es == 1 else (0,))}
    elif path == "TABLE":
        out |= {"crossover ll->ll128", "crossover ll128->oneshot", "crossover oneshot->direct"}
    return out


# ---------------------------------------------------------------------------------------------- guarded arenas
# One device allocation per rank for every sendbuff of a run and one for every recvbuff, each buffer a slot with at
# least ARENA_GAP bytes of ARENA_FILL before and after it. The layout is the same on every rank (symmetric windows need
# that). Output slots are prefilled with the bitwise complement of the expected result, so an element the kernel never
# writes differs in every byte. arena_errors compares the images read back; it is pure numpy
# (tests/test_boundaries_cpu.py plants faults with a numpy mock collective and asserts each is reported).
ARENA_GAP, ARENA_FILL = 64, 0x5A


class ArenaCase:
    """One call: `count` in this module's convention (launch), `mis` elements off 16-byte alignment, in place or not.
    Out of place: the sendbuff is a slot of the send arena and the recvbuff one of the recv arena (a Reduce has the
    slot on every rank, used on the root). In place: one slot of the recv arena that holds the input (AllGather: at
    this rank's block)."""

    def __init__(self, coll, dtype, op, count, root=0, inplace=False, mis=0, tag=""):
        self.coll, self.dtype, self.op, self.count, self.root = coll, dtype, op, count, root
        self.inplace, self.mis, self.tag = inplace, mis, tag
        self.es = np.dtype(oracle.NP_STORAGE[dtype]).itemsize
        self.send_off = self.recv_off = None

    def what(self):
        return (f"{self.tag} {self.coll} dt={self.dtype} op={self.op} count={self.count} root={self.root} "
                f"inplace={self.inplace} mis={self.mis}").strip()

    def send_bytes(self, n):
        return self.count * self.es

    def recv_bytes(self, n):
        if self.inplace:
            return max(self.count, out_count(self.coll, n, self.count)) * self.es
        return out_count(self.coll, n, self.count) * self.es

    def out_region(self, n, r):
        """(offset in the recv arena, bytes) of rank r's output; None where the rank has none."""
        if self.coll == "reduce" and r != self.root:
            return None
        nb = out_count(self.coll, n, self.count) * self.es
        return (self.recv_off + (r * nb if self.inplace and self.coll == "reducescatter" else 0), nb)

    def send_ptr_off(self, n, r):
        """('send' | 'recv', offset) of rank r's sendbuff."""
        if not self.inplace:
            return "send", self.send_off
        return "recv", self.recv_off + (r * self.count * self.es if self.coll == "allgather" else 0)


def arena_layout(cases, n):
    """Assign the slots; returns (send arena bytes, recv arena bytes)."""
    sizes = [ARENA_GAP, ARENA_GAP]
    for cs in cases:
        for which, nb in ((0, 0 if cs.inplace else cs.send_bytes(n)), (1, cs.recv_bytes(n))):
            if which == 0 and cs.inplace:
                continue
            off = _up(sizes[which], 16) + cs.mis * cs.es
            if which == 0:
                cs.send_off = off
            else:
                cs.recv_off = off
            sizes[which] = _up(off + nb, 16) + ARENA_GAP
    return sizes[0], sizes[1]


def arena_images(cases, n, sizes, inputs, wants):
    """The arenas before the run: per rank (send image, recv image) as uint8 arrays. inputs[k][r]: rank r's input of
    case k; wants[k][r]: its expected output (None where it has none)."""
    out = []
    for r in range(n):
        send = np.full(sizes[0], ARENA_FILL, dtype=np.uint8)
        recv = np.full(sizes[1], ARENA_FILL, dtype=np.uint8)
        for k, cs in enumerate(cases):
            reg = cs.out_region(n, r)
            if reg is not None and reg[1]:
                recv[reg[0]: reg[0] + reg[1]] = ~np.ascontiguousarray(wants[k][r]).view(np.uint8)
            which, off = cs.send_ptr_off(n, r)
            raw = np.ascontiguousarray(inputs[k][r]).view(np.uint8)
            (send if which == "send" else recv)[off: off + raw.size] = raw
        out.append((send, recv))
    return out


def _where(cases, n, which, idx):
    """Name the case next to byte `idx` of an arena: (case, 'inside' | 'before' | 'after', distance)."""
    best = None
    for cs in cases:
        off = cs.send_off if which == "send" else cs.recv_off
        if off is None:
            continue
        nb = cs.send_bytes(n) if which == "send" else cs.recv_bytes(n)
        if off <= idx < off + nb:
            return cs, "inside", idx - off
        d = off - idx if idx < off else idx - (off + nb) + 1
        if best is None or d < best[2]:
            best = (cs, "before" if idx < off else "after", d)
    return best


def arena_errors(cases, n, before, after, wants, max_errors=20):
    """Compare the arenas read back (`after`, per rank (send image, recv image)) with the images before the run and
    the expected outputs: every output bit for bit (same_bits: the inputs of these tests are finite, so every bit is
    compared), every byte outside the outputs unchanged — the fill between and around the slots, the sendbuffs, the
    slots of ranks that have no output. Returns error strings that name the rank, the case and its count."""
    errs = []
    for r in range(n):
        send0, recv0 = before[r]
        send1, recv1 = after[r]
        untouched = np.ones(recv0.size, dtype=bool)
        for k, cs in enumerate(cases):
            reg = cs.out_region(n, r)
            if reg is None:
                continue
            untouched[reg[0]: reg[0] + reg[1]] = False
            npdt = oracle.NP_STORAGE[cs.dtype]
            got = recv1[reg[0]: reg[0] + reg[1]].view(npdt)
            want = np.ascontiguousarray(wants[k][r])
            if not same_bits(got, want, cs.dtype):
                bad = np.nonzero(_raw(got) != _raw(want))[0]
                unwritten = int(np.sum(_raw(got)[bad] == ~_raw(want)[bad]))
                errs.append(f"rank {r} {cs.what()}: {bad.size} of {want.size} output elements differ ({unwritten} never "
                            f"written), first at {bad[:5].tolist()} got {[hex(int(v)) for v in _raw(got)[bad[:3]]]} "
                            f"want {[hex(int(v)) for v in _raw(want)[bad[:3]]]}")
        for which, a, b, mask in (("send", send0, send1, None), ("recv", recv0, recv1, untouched)):
            diff = a != b
            if mask is not None:
                diff &= mask
            idx = np.nonzero(diff)[0]
            seen = set()
            for i in idx[:4096]:
                cs, rel, d = _where(cases, n, which, int(i))
                if (id(cs), rel) in seen:
                    continue
                seen.add((id(cs), rel))
                if rel == "inside":
                    what = "sendbuff byte" if which == "send" or cs.inplace else "byte of a slot without output"
                    errs.append(f"rank {r} {cs.what()}: {what} {d} changed ({which} arena offset {int(i)})")
                else:
                    errs.append(f"rank {r} {cs.what()}: fill byte {d} {rel} the {which} slot was written "
                                f"({which} arena offset {int(i)}, {int(idx.size)} bytes changed in this arena)")
        if len(errs) >= max_errors:
            break
    return errs
