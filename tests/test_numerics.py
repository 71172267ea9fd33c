"""Exhaustive CPU check of the kernels' element arithmetic (nccl_amd/csrc/numerics.h, compiled for the
host as build/libnumerics_host.so) against the independent C oracle: every fp16/bf16 bit pattern,
every fp8 pair, and the integer functors on edge values."""
import ctypes
import os

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = os.path.join(ROOT, "build", "libnumerics_host.so")


@pytest.fixture(scope="module")
def nx(built):
    if not os.path.exists(NX):
        import subprocess
        subprocess.check_call(["make", "numerics-host"], cwd=ROOT)
    L = ctypes.CDLL(NX)
    U64, I = ctypes.c_uint64, ctypes.c_int
    for f in ("nx_red",):
        getattr(L, f).restype = U64
        getattr(L, f).argtypes = [I, I, U64, U64, U64]
    for f in ("nx_pre", "nx_post"):
        getattr(L, f).restype = U64
        getattr(L, f).argtypes = [I, I, U64, U64]
    L.nx_swar8.restype = ctypes.c_uint32
    L.nx_swar8.argtypes = [I, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.nx_swar_div.restype = ctypes.c_uint32
    L.nx_swar_div.argtypes = [ctypes.c_uint32, ctypes.c_uint32, I]
    L.nx_f32_to_fp8.restype = ctypes.c_uint8
    L.nx_f32_to_fp8.argtypes = [ctypes.c_float, I]
    L.nx_fp8_to_f32.restype = ctypes.c_float
    L.nx_fp8_to_f32.argtypes = [ctypes.c_uint8, I]
    L.nx_f32_to_bf16.restype = ctypes.c_uint16
    L.nx_f32_to_bf16.argtypes = [ctypes.c_float]
    L.nx_f32_to_half.restype = ctypes.c_uint16
    L.nx_f32_to_half.argtypes = [ctypes.c_float]
    return L


def _bits_eq_f(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def test_fp8_decode_all_codes(nx):
    O = oracle.lib()
    for e5 in (0, 1):
        for v in range(256):
            assert _bits_eq_f(nx.nx_fp8_to_f32(v, e5), O.oracle_fp8_to_f32(v, e5)), (e5, v)


def test_fp8_encode_from_every_half(nx):
    # every value the reference's half-precision fp8 arithmetic can produce is a half value
    O = oracle.lib()
    halves = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    for e5 in (0, 1):
        for f in halves[::7]:
            assert nx.nx_f32_to_fp8(float(f), e5) == O.oracle_f32_to_fp8(float(f), e5), (e5, f)


def test_bf16_and_half_rounding(nx):
    O = oracle.lib()
    rng = np.random.default_rng(1)
    vals = np.concatenate([rng.standard_normal(20000).astype(np.float32) * 10.0 ** rng.integers(-40, 38, 20000),
                           np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, 65520.0, 65519.99, 6e-8, 3e-8, 1e-45],
                                    dtype=np.float32)]).astype(np.float32)
    for f in vals:
        if not np.isfinite(f) and not np.isinf(f):
            continue
        assert nx.nx_f32_to_bf16(float(f)) == O.oracle_f32_to_bf16(float(f)), f
        assert nx.nx_f32_to_half(float(f)) == O.oracle_f32_to_f16(float(f)), f


@pytest.mark.parametrize("dtype", [6, 9, 10, 11])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_small_float_reduce_matches_oracle(nx, dtype, op):
    # one hop f(a, b) for many (a, b) pairs; oracle computes the same hop through a 2-rank fold
    rng = np.random.default_rng(dtype * 10 + op)
    npdt = oracle.NP_STORAGE[dtype]
    if dtype in (10, 11):
        a = np.repeat(np.arange(256, dtype=np.uint8), 256)
        b = np.tile(np.arange(256, dtype=np.uint8), 256)
    else:
        a = rng.integers(0, 65536, 60000).astype(np.uint16)
        b = rng.integers(0, 65536, 60000).astype(np.uint16)
        # signaling-NaN inputs are out of scope (fminf(sNaN, x) differs between libm and the GPU's
        # IEEE-mode v_min_f32; the reference's __hmin behaviour on sNaN is unpinned): make them quiet
        qbit = 0x200 if dtype == 6 else 0x40
        expm = 0x7C00 if dtype == 6 else 0x7F80
        for x in (a, b):
            snan = ((x & expm) == expm) & ((x & (qbit - 1)) != 0) & ((x & qbit) == 0)
            x[snan] |= qbit
    arg = 0 if op != 2 else 0  # min
    # oracle: AllReduce with n=2 folds chunk0 as f(pre(x0), x1) ... emulate one hop via reduce(root=1):
    # reduce root=1 folds ranks 0 then 1: acc = x0; acc = f(x1, acc)  -> f(b, a)
    want = oracle.reduce([a, b], dtype, {0: 0, 1: 1, 2: 3}[op], 1)
    got = np.array([nx.nx_red(dtype, op, arg, int(y), int(x)) for x, y in zip(a, b)], dtype=np.uint64).astype(npdt)
    fa, fb = oracle.to_f32(dtype, got), oracle.to_f32(dtype, want)
    ok = (got == want) | (np.isnan(fa) & np.isnan(fb))
    assert ok.all(), f"{(~ok).sum()} mismatches, e.g. a={a[~ok][:3]} b={b[~ok][:3]} got={got[~ok][:3]} want={want[~ok][:3]}"


@pytest.mark.parametrize("dtype,bits", [(0, 8), (1, 8), (2, 32), (3, 32), (4, 64), (5, 64)])
def test_integer_functors(nx, dtype, bits):
    rng = np.random.default_rng(bits + dtype)
    npdt = oracle.NP_STORAGE[dtype]
    info = np.iinfo(npdt)
    vals = np.concatenate([rng.integers(info.min, info.max, 2000, dtype=npdt, endpoint=True),
                           np.array([info.min, info.max, 0, 1, -1 if info.min < 0 else 2], dtype=npdt)])
    for op_nccl, op_dev in ((0, 0), (1, 1), (2, 2), (3, 2)):
        _, arg = oracle.dev_op(op_nccl, dtype, 4)
        a, b = vals, np.roll(vals, 1)
        want = oracle.reduce([a, b], dtype, op_nccl, 1)
        ua, ub = a.view(np.dtype(f"u{bits // 8}")), b.view(np.dtype(f"u{bits // 8}"))
        got = np.array([nx.nx_red(dtype, op_dev, arg, int(y), int(x)) for x, y in zip(ua, ub)],
                       dtype=np.uint64).astype(np.dtype(f"u{bits // 8}")).view(npdt)
        assert np.array_equal(got, want), (op_nccl, dtype)
    # avg: SumPostDiv post-op on every value
    for n in (2, 3, 7, 8):
        _, arg = oracle.dev_op(4, dtype, n)
        u = vals.view(np.dtype(f"u{bits // 8}"))
        got = np.array([nx.nx_post(dtype, 4, arg, int(x)) for x in u], dtype=np.uint64).astype(u.dtype).view(npdt)
        signed = dtype in (0, 2, 4)
        want = [(-(-int(v) // n) if (signed and int(v) < 0) else int(v) // n) for v in vals.tolist()]
        assert [int(x) for x in got] == want


@pytest.mark.parametrize("op,mask", [(0, 0), (2, 0x80), (2, 0x7f), (2, 0x00), (2, 0xff)])
def test_swar_bytes_match_functor(nx, op, mask):
    """numerics.h Swar8 (4 bytes per dword, used by the uint8/int8 Sum and MinMax folds) equals the per-byte
    functor Red<uint8_t, OP>::red for every byte pair in every lane position (masks: int8 min / max, uint8
    min / max)."""
    a = np.arange(256, dtype=np.uint32)
    pairs = [(int(x), int(y)) for x in a for y in a]
    rng = np.random.default_rng(7)
    for lane in range(4):
        for x, y in pairs[lane::4]:  # every pair once across the four lanes
            fill_a, fill_b = (int(v) for v in rng.integers(0, 2**32, 2, dtype=np.uint64))
            sh = 8 * lane
            wa = (fill_a & ~(0xff << sh)) | (x << sh)
            wb = (fill_b & ~(0xff << sh)) | (y << sh)
            got = nx.nx_swar8(op, mask, wa, wb)
            for l in range(4):
                ea, eb = (wa >> (8 * l)) & 0xff, (wb >> (8 * l)) & 0xff
                want = nx.nx_red(1, op, mask, ea, eb)
                assert (got >> (8 * l)) & 0xff == want, (op, mask, hex(wa), hex(wb), l)


def test_swar_byte_division_matches_functor(nx):
    """numerics.h swarDivBytes (the uint8 / int8 avg post-op on four bytes, multiply-shift instead of a divide)
    equals Red<uint8_t, DEV_SUMPOSTDIV>::post — magnitude / n, sign restored — for every byte in every lane, every
    rank count 1..16 and both signednesses."""
    for d in range(1, 17):
        for signed in (0, 1):
            arg = (d << 1) | signed
            for x in range(256):
                w = x | (((x * 7 + 1) & 0xff) << 8) | (((x * 13 + 5) & 0xff) << 16) | (((255 - x) & 0xff) << 24)
                got = nx.nx_swar_div(w, d, signed)
                for l in range(4):
                    want = nx.nx_post(1, 4, arg, (w >> (8 * l)) & 0xff)
                    assert (got >> (8 * l)) & 0xff == want, (d, signed, hex(w), l)


# ---- the PreMulSum pre-op (user operators: ncclRedOpCreatePreMulSum) against the oracle's one-rank PreMulSum ----

def _nx_pre(nx, dtype, scalar_bits, x):
    """nx_pre(dtype, DEV_PREMULSUM, scalar, x) for every element of x (storage array) in one call."""
    nx.nx_pre_array.restype = None
    nx.nx_pre_array.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_uint64]
    x = np.ascontiguousarray(x)
    out = np.empty_like(x)
    nx.nx_pre_array(dtype, 3, scalar_bits, x.ctypes.data, out.ctypes.data, x.size)
    return out


def _pre_vs_oracle(nx, dtype, x, scalars):
    from tests import gpu_cases as G
    for s in scalars:
        want = oracle.all_reduce([x], dtype, premul_scalar_bits=s)
        if G.scalar_is_finite(dtype, s):
            assert G.nan_cap_ok(want, dtype), (dtype, hex(s))  # the NaN-by-position rule hides < 10 % of the elements
        got = _nx_pre(nx, dtype, s, x)
        if not G.same_bits(got, want, dtype):
            bad = np.nonzero(G._raw(got) != G._raw(want))[0]
            raise AssertionError(f"dtype {dtype} scalar {hex(s)}: {bad.size} candidates differ, e.g. x="
                                 f"{[hex(int(v)) for v in G._raw(x)[bad[:4]]]} got "
                                 f"{[hex(int(v)) for v in G._raw(got)[bad[:4]]]} want "
                                 f"{[hex(int(v)) for v in G._raw(want)[bad[:4]]]}")


def test_pre_array_entry_matches_scalar_entry(nx):
    """The array entry point used below is the per-element nx_pre."""
    x = np.arange(0, 65536, 97, dtype=np.uint16)
    got = _nx_pre(nx, 6, 0x3555, x)
    assert [int(v) for v in got] == [nx.nx_pre(6, 3, 0x3555, int(v)) for v in x]


@pytest.mark.parametrize("dtype", [10, 11])
def test_premul_pre_fp8_every_pair(nx, dtype):
    """fp8: pre(x) = fromF(x * s) for every one of the 256 x 256 (x, scalar) pairs."""
    _pre_vs_oracle(nx, dtype, np.arange(256, dtype=np.uint8), range(256))


@pytest.mark.parametrize("dtype", [6, 9])
def test_premul_pre_half_bf16_every_pattern(nx, dtype):
    """fp16 (native _Float16 multiply) and bf16: every one of the 65,536 x patterns against the scalar list."""
    from tests import gpu_cases as G
    _pre_vs_oracle(nx, dtype, np.arange(65536, dtype=np.uint16), G.premul_scalars(dtype).values())


@pytest.mark.parametrize("dtype", [7, 8])
def test_premul_pre_fp32_fp64(nx, dtype):
    """fp32 / fp64: random bit patterns, random moderate values and the special values against the scalar list."""
    from tests import gpu_cases as G
    rng = np.random.default_rng(dtype)
    ut, ft = (np.uint32, np.float32) if dtype == 7 else (np.uint64, np.float64)
    info = np.finfo(ft)
    sp = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, info.smallest_subnormal, -info.smallest_subnormal,
                   info.tiny, -info.tiny * (1 - info.eps), info.max, -info.max, 1.0, 3.0, -1.5], dtype=ft)
    x = np.concatenate([rng.integers(0, np.iinfo(ut).max, 3000, dtype=ut, endpoint=True).view(ft),
                        (rng.standard_normal(3000) * 10.0 ** rng.integers(-6, 6, 3000)).astype(ft), sp])
    _pre_vs_oracle(nx, dtype, x, G.premul_scalars(dtype).values())


@pytest.mark.parametrize("dtype,bits", [(0, 8), (1, 8), (2, 32), (3, 32), (4, 64), (5, 64)])
def test_premul_pre_integers(nx, dtype, bits):
    """Integer PreMulSum: pre(x) = (x * s) mod 2^bits, against the oracle and against Python's integers."""
    from tests import gpu_cases as G
    npdt = oracle.NP_STORAGE[dtype]
    ut = np.dtype(f"u{bits // 8}")
    ones = (1 << bits) - 1
    rng = np.random.default_rng(bits + dtype)
    edge = [0, 1, 2, 3, ones, ones - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << (bits - 1)) + 1, ones // 3,
            ones // 3 * 2, 1 << (bits // 2), (1 << (bits // 2)) - 1, (1 << (bits // 2)) + 1]
    x = np.concatenate([np.array(edge, dtype=ut), rng.integers(0, ones, 500, dtype=ut, endpoint=True)]).view(npdt)
    for s in G.premul_scalars(dtype).values():
        got = _nx_pre(nx, dtype, s, x)
        want = oracle.all_reduce([x], dtype, premul_scalar_bits=s)
        assert np.array_equal(got, want), (dtype, hex(s))
        assert [int(v) for v in got.view(ut)] == [(int(v) * s) & ones for v in x.view(ut)], (dtype, hex(s))


# ---- the built-in operators over the edge-value pairs (tests/gpu_cases.py edge_inputs): the host branch of the
# functors the GPU file tests/test_gpu_edge_values.py runs on the device ----

def _nx_fold(nx, dtype, devop, arg, srcs):
    """nx_fold_array: acc = pre(src0); acc = red(pre(src_k), acc); post(acc), one call for the whole arrays."""
    nx.nx_fold_array.restype = None
    nx.nx_fold_array.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
    srcs = [np.ascontiguousarray(x) for x in srcs]
    ptrs = (ctypes.c_void_p * len(srcs))(*[x.ctypes.data for x in srcs])
    out = np.empty_like(srcs[0])
    nx.nx_fold_array(dtype, devop, arg, ptrs, len(srcs), out.ctypes.data, out.size)
    return out


def _fold_vs_oracle(nx, dtype, op, ins):
    """The host functors' fold of `ins` in rank order against oracle.reduce to the last rank — nccl_oracle.c
    fold_elem from first = (root + 1) % n = 0: acc = pre(x0), then acc = f(pre(x_k), acc) for k = 1 .. n-1 — with the
    GPU tests' comparison: every bit, NaN by position under the 10 % cap, the defined NaNs bit for bit."""
    from tests import gpu_cases as G
    n = len(ins)
    devop, arg = oracle.dev_op(op, dtype, n)
    want = oracle.reduce(ins, dtype, op, n - 1)
    assert G.nan_cap_ok(want, dtype), f"dtype {dtype} op {op} n {n}: more than 10 % of the oracle's result is NaN"
    got = _nx_fold(nx, dtype, devop, arg, ins)
    errs = G.edge_errors(got, want, G.defined_mask(ins, dtype, op), dtype, f"dtype {dtype} op {op} n {n}")
    if errs:
        bad = np.nonzero(G._raw(got) != G._raw(want))[0][:3]
        errs.append(f"inputs there: {[[hex(int(G._raw(x)[i])) for x in ins] for i in bad]}")
    assert not errs, "\n".join(errs)


def test_fold_array_entry_matches_scalar_entries(nx):
    """The array entry point used below is nx_pre / nx_red / nx_post per element, in the order it documents."""
    rng = np.random.default_rng(3)
    srcs = [rng.integers(0, 65536, 500).astype(np.uint16) & 0x7BFF for _ in range(3)]
    for dtype, devop, arg in ((6, 3, 0x3555), (9, 1, 0), (6, 2, 1)):
        want = []
        for x0, x1, x2 in zip(*srcs):
            acc = nx.nx_pre(dtype, devop, arg, int(x0))
            for x in (x1, x2):
                acc = nx.nx_red(dtype, devop, arg, nx.nx_pre(dtype, devop, arg, int(x)), acc)
            want.append(nx.nx_post(dtype, devop, arg, acc))
        assert [int(v) for v in _nx_fold(nx, dtype, devop, arg, srcs)] == want, (dtype, devop)


def test_edge_inputs_construction():
    """edge_inputs: the base list sizes times 18 blocks, no signalling NaN, and on fp16 the half-ulp partner (block 6:
    half the distance from a to its neighbour away from zero, a's sign) and the nine constants by value."""
    from tests import gpu_cases as G
    for dtype, size in ((6, 65536), (9, 65536), (7, 8192), (8, 32768)):
        r0, r1, r2 = G.edge_inputs(dtype, 3)
        assert r0.size == r1.size == r2.size == 18 * size and G._edge_base(dtype).size == size
        assert all(np.array_equal(G._raw(x), G._raw(y)) for x, y in zip(G.edge_inputs(dtype, 2), (r0, r1)))
        bits, M, _ = G._EDGE_FORMAT[dtype]
        ut = np.dtype(f"u{bits // 8}").type
        expm = ut(((1 << (bits - 1 - M)) - 1) << M)
        for u in map(G._raw, (r0, r1, r2)):
            assert not (((u & expm) == expm) & ((u & ut((1 << M) - 1)) != 0) & ((u & ut(1 << (M - 1))) == 0)).any()
    r0, r1 = (G._raw(x) for x in G.edge_inputs(6, 2))
    a, h = r0[5 * 65536:6 * 65536], r1[5 * 65536:6 * 65536]
    e = (a >> 10) & 0x1F
    finite = (e >= 2) & (e <= 29)    # half an ulp is a value of the type, the neighbour away from zero is finite
    fa, fh = (x.view(np.float16).astype(np.float64) for x in (a, h))
    up = (a + np.uint16(1)).view(np.float16).astype(np.float64)
    assert np.array_equal(fh[finite] * 2, up[finite] - fa[finite])
    c = [float(r1[(9 + k) * 65536:(9 + k) * 65536 + 1].view(np.float16)[0]) for k in range(9)]
    assert c[:5] == [1.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -14] and c[5] == 0 and np.signbit(c[5])
    assert c[6:8] == [np.inf, 1.0 + 2.0 ** -10] and abs(c[8] - 1.0 / 3.0) < 2.0 ** -12


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("op", [0, 1, 2, 3, 4], ids=["sum", "prod", "max", "min", "avg"])
@pytest.mark.parametrize("dtype", [6, 9, 7, 8], ids=["fp16", "bf16", "fp32", "fp64"])
def test_edge_pairs_fold_matches_oracle(nx, dtype, op, n):
    """Every base value against its 18 partners (ties, overflow, cancellation, subnormal results, signed zeros, every
    fp16 / bf16 NaN) through the host functors, n = 2 (one hop) and n = 3 (two hops with a rounded intermediate, Avg's
    inexact 1/3), every built-in operator (float Avg is PreMulSum by the type's 1/n)."""
    from tests import gpu_cases as G
    _fold_vs_oracle(nx, dtype, op, G.edge_inputs(dtype, n))


@pytest.mark.parametrize("op", [2, 4], ids=["max", "avg"])
@pytest.mark.parametrize("dtype", [10, 11], ids=["e4m3", "e5m2"])
def test_fp8_every_pair_max_avg(nx, dtype, op):
    """Every fp8 code pair under Max and Avg (test_small_float_reduce_matches_oracle runs Sum, Prod and Min)."""
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    devop, arg = oracle.dev_op(op, dtype, 2)
    want = oracle.reduce([a, b], dtype, op, 1)
    got = _nx_fold(nx, dtype, devop, arg, [a, b])
    fa, fb = oracle.to_f32(dtype, got), oracle.to_f32(dtype, want)
    ok = (got == want) | (np.isnan(fa) & np.isnan(fb))
    assert ok.all(), f"{(~ok).sum()} mismatches, e.g. a={a[~ok][:3]} b={b[~ok][:3]} got={got[~ok][:3]} want={want[~ok][:3]}"
