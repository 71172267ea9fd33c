"""GPU tests of user PreMulSum operators (ncclRedOpCreatePreMulSum): every datatype, every kernel path and the whole
scalar list, bit for bit against the CPU oracle's fold for that path.

Ranks share the box's one GPU (ncclCommInitAll with a repeated device, NCCL_MULTI_RANK_GPU_ENABLE=1) or run as spawned
processes. A case that must show which kernel ran reads the kernel log (NCCL_AMD_KERNEL_LOG, read when the library
loads) and therefore runs in a spawned worker, like tests/test_gpu_broadcast.py.

Comparison: gpu_cases.same_bits (every bit; a NaN must sit where the oracle has one) plus, bit for bit, the elements
where exactly one NaN arises in the fold (test_gpu_collectives.py _single_nan_errors). For every case whose scalar is
finite the oracle's own result must be at least 90 % non-NaN (gpu_cases.nan_cap_ok), so the NaN rule cannot hide a
failure; one documented exception is in _job_exhaustive_half. Every output buffer carries guard bytes, checked
unchanged."""
import ctypes
import multiprocessing as mp
import os
import queue
import re

import numpy as np
import pytest

os.environ.setdefault("NCCL_AMD_SPIN_TIMEOUT_MS", "30000")

pytestmark = pytest.mark.gpu

ALL_TYPES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
GUARD, FILL = 64, 0x5A
INVALID_ARGUMENT = 4
# the kernels' element type per datatype, as the kernel log spells it (signed integers run the unsigned kernels)
KERNEL_TYPE = {0: "unsigned char", 1: "unsigned char", 2: "unsigned int", 3: "unsigned int", 4: "unsigned long",
               5: "unsigned long", 6: "ncclamd::half_t", 7: "float", 8: "double", 9: "ncclamd::bf16_t",
               10: "ncclamd::e4m3_t", 11: "ncclamd::e5m2_t"}

_REF = {"NCCL_BUFFSIZE": "16384", "NCCL_MAX_CTAS": "5"}
# path -> (communicator environment, the AllReduce kernel the log must name: {T} the element type, {OP} the operator
# template argument — 3, DEV_PREMULSUM, for every case of this file; path_pattern)
PATHS = {
    "LL": ({"NCCL_PROTO": "LL"}, r"llKernel<{T}, {OP}, \d+, 0>"),
    "LL128": ({"NCCL_PROTO": "LL128"}, r"llKernel<{T}, {OP}, \d+, 1>"),
    "ONESHOT": ({"NCCL_ALGO": "ONESHOT"}, r"collKernel<{T}, {OP}, 4>"),
    "DIRECT": ({"NCCL_ALGO": "DIRECT", "NCCL_PROTO": "Simple", "NCCL_AMD_SLOT_BYTES": "4096", "NCCL_AMD_NSLOTS": "2",
                "NCCL_MAX_CTAS": "7"}, r"collKernel<{T}, {OP}, 0>"),
    "DIRECT_PULLS": ({"NCCL_ALGO": "DIRECT", "NCCL_PROTO": "Simple", "NCCL_AMD_AG_PULL": "1", "NCCL_AMD_RS_PULL": "1"},
                     r"collKernel<{T}, {OP}, 0>"),
    "REGISTERED": ({"NCCL_PROTO": "Simple"}, r"symKernel<{T}, {OP}, [01]>"),
    "RING": (dict(_REF, NCCL_ALGO="RING"), r"pipeKernel<{T}, {OP}, 0>"),
    "TREE": (dict(_REF, NCCL_ALGO="TREE"), r"pipeKernel<{T}, {OP}, 3>"),
    "REF_ORDER": (dict(_REF, NCCL_AMD_REF_ORDER="1"), r"collKernel<{T}, {OP}, 5>"),
}
FULL_LIST_PATHS = ("LL", "DIRECT")   # the whole scalar list for every type runs on these two
DIRECT_SIMPLE = {"NCCL_ALGO": "DIRECT", "NCCL_PROTO": "Simple"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch


def _G():
    from tests import gpu_cases as G
    return G


def _es(dtype):
    return np.dtype(_G().oracle.NP_STORAGE[dtype]).itemsize


def _is_float(dtype):
    return dtype in _G().FLOAT_TYPES


def three_scalars(dtype):
    """-2.5 / 3, the inexact one (the type's 1/3; 0x55... for integers), the smallest subnormal / the sign bit."""
    sc = _G().premul_scalars(dtype)
    return [sc[k] for k in (("-2.5", "third", "minsub") if _is_float(dtype) else ("3", "0x55", "signbit"))]


def case_inputs(n, dtype, count, seed):
    """Float inputs carry the special values of test_gpu_collectives._with_specials (3 of every 37 positions;
    not below 37 elements, where position 0's NaN alone would break the NaN cap); integer inputs span the full
    range."""
    G = _G()
    ins = G.make_inputs(n, dtype, count, seed)
    if _is_float(dtype) and count >= 37:
        from tests.test_gpu_collectives import _with_specials
        ins = _with_specials(ins, dtype)
    return ins


def single_nan_mask(ins, dtype, bits):
    """Elements where exactly one NaN arises in the PreMulSum fold of at most three ranks: one NaN input, no NaN made by
    the pre-multiply (0 x Inf, a NaN scalar) and no +Inf meeting -Inf among the pre-multiplied values. Their bits are
    defined (the one NaN, quieted, through every add) and compared with the oracle's."""
    G = _G()
    assert len(ins) <= 3
    f = np.stack([G.oracle.to_f32(dtype, x) for x in ins])
    pre = np.stack([G.oracle.to_f32(dtype, G.oracle.all_reduce([x], dtype, premul_scalar_bits=bits)) for x in ins])
    nan_in = np.isnan(f)
    made = (np.isnan(pre) & ~nan_in).any(0) | ((pre == np.inf).any(0) & (pre == -np.inf).any(0))
    return (nan_in.sum(0) == 1) & ~made


def compare(got, want, dtype, one, what):
    """Error strings: same_bits, and the single-NaN elements (`one`, or None) bit for bit."""
    G = _G()
    errs = []
    if not G.same_bits(got, want, dtype):
        bad = np.nonzero(G._raw(got) != G._raw(want))[0]
        errs.append(f"{what}: {bad.size} of {want.size} candidates differ, first at {bad[:5].tolist()} got "
                    f"{[hex(int(v)) for v in G._raw(got)[bad[:3]]]} want {[hex(int(v)) for v in G._raw(want)[bad[:3]]]}")
    if one is not None and one.any():
        a, b = G._raw(got)[one], G._raw(want)[one]
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            errs.append(f"{what}: {bad.size} of {int(one.sum())} single-NaN elements differ, e.g. "
                        f"{hex(int(a[bad[0]]))} vs {hex(int(b[bad[0]]))}")
    return errs


def create_op(comm, dtype, bits, device_ptr=None):
    """ncclRedOpCreatePreMulSum from the scalar's storage bits (host immediate) or a device pointer."""
    import nccl_amd
    op = ctypes.c_int()
    if device_ptr is not None:
        rc = nccl_amd.load().ncclRedOpCreatePreMulSum(ctypes.byref(op), device_ptr, dtype, 0, comm.ptr)
    else:
        buf = ctypes.create_string_buffer(int(bits).to_bytes(8, "little"), 8)
        rc = nccl_amd.load().ncclRedOpCreatePreMulSum(ctypes.byref(op), buf, dtype, 1, comm.ptr)
    assert rc == 0, f"ncclRedOpCreatePreMulSum returned {rc}"
    return op.value


class DevScalar:
    """A 16-byte device allocation holding a scalar's storage bits at its start."""

    def __init__(self, dtype, bits):
        import torch
        self.es = _es(dtype)
        self.t = torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.set(bits)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def set(self, bits):
        import torch
        raw = np.frombuffer(int(bits).to_bytes(8, "little"), dtype=np.uint8)[:self.es].copy()
        self.t[:self.es].copy_(torch.from_numpy(raw))
        torch.cuda.synchronize()


class Buf:
    """nbytes at byte offset GUARD + mis of a device storage that is FILL everywhere else."""

    def __init__(self, nbytes, mis=0, data=None):
        import torch
        self.store = torch.full((GUARD + mis + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.lo, self.nbytes = GUARD + mis, nbytes
        self.ptr = self.store.data_ptr() + self.lo
        assert (self.store.data_ptr() & 15) == 0
        if data is not None:
            self.put(data)

    def put(self, data):
        import torch
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert raw.size == self.nbytes
        self.store[self.lo: self.lo + self.nbytes].copy_(torch.from_numpy(raw.copy()))

    def get(self, npdt, lo=0, nbytes=None):
        raw = self.store.cpu().numpy()
        nbytes = self.nbytes - lo if nbytes is None else nbytes
        return raw[self.lo + lo: self.lo + lo + nbytes].copy().view(npdt)

    def guards_ok(self):
        raw = self.store.cpu().numpy()
        return bool(np.all(raw[:self.lo] == FILL) and np.all(raw[self.lo + self.nbytes:] == FILL))


def comms_under(n, env=None):
    """n ranks on GPU 0 in this process, created under `env` (the knobs are read at communicator init)."""
    torch = _torch()
    import nccl_amd
    env = dict(env or {})
    env["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        torch.cuda.set_device(0)
        comms = nccl_amd.Communicator.init_all([0] * n)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return list(zip(comms, [torch.cuda.Stream() for _ in range(n)]))


def destroy(cs):
    for c, _ in cs:
        c.destroy()


def run(cs, coll, dtype, bits, ins, ops, mis=0, inplace=False, root=0, register=False, what="", want=None,
        cap=True):
    """One collective with the user operators `ops` (one handle per rank of cs, scalar bits `bits`) on every
    (comm, stream) of this process, from fresh guarded buffers; `mis`: byte misalignment of every buffer. The result
    is compared with gpu_cases.expected for the communicator's environment (`want` overrides it). Returns errors."""
    torch = _torch()
    import nccl_amd
    G = _G()
    n = cs[0][0].nranks
    es = _es(dtype)
    npdt = G.oracle.NP_STORAGE[dtype]
    count = ins[0].size
    what = f"{what} {coll} dt={dtype} scalar={hex(bits)} count={count} mis={mis} inplace={inplace}"
    if want is None:
        want = G.expected(coll, ins, dtype, 0, root, "", premul=bits)
    if cap and G.scalar_is_finite(dtype, bits):
        assert all(G.nan_cap_ok(w, dtype) for w in want), f"{what}: more than 10 % of the oracle's result is NaN"
    one = single_nan_mask(ins, dtype, bits) if _is_float(dtype) else None
    per = count // n
    plan = []
    for comm, stream in cs:
        r = comm.rank
        sb = Buf(count * es, mis, ins[r])
        if inplace:
            rb, rptr = sb, sb.ptr + (r * per * es if coll == "reducescatter" else 0)
        elif coll == "reduce" and r != root:
            rb, rptr = None, None
        else:
            rb = Buf((per if coll == "reducescatter" else count) * es, mis)
            rptr = rb.ptr
        hs = []
        if register:
            for b in {id(sb): sb, id(rb): rb}.values():
                if b is not None:
                    hs.append(comm.register_buffer(b.store.data_ptr(), b.store.numel()))
        plan.append((comm, stream, sb, rb, rptr, hs))
    torch.cuda.synchronize()
    with nccl_amd.group():
        for (comm, stream, sb, rb, rptr, _), op in zip(plan, ops):
            sp = stream.cuda_stream
            if coll == "allreduce":
                comm.all_reduce_raw(sb.ptr, rptr, count, dtype, op, sp)
            elif coll == "reducescatter":
                comm.reduce_scatter_raw(sb.ptr, rptr, per, dtype, op, sp)
            else:
                comm.reduce_raw(sb.ptr, rptr, count, dtype, op, root, sp)
    errs = []
    for comm, stream, sb, rb, rptr, hs in plan:
        stream.synchronize()
        r = comm.rank
        if comm.async_error():
            errs.append(f"{what} rank {r}: async error {comm.async_error()}")
        elif rb is not None:
            if coll == "reducescatter":
                got = rb.get(npdt, r * per * es if inplace else 0, per * es)
                errs += compare(got, want[r], dtype, None if one is None else one[r * per:(r + 1) * per],
                                f"{what} rank {r}")
            else:
                errs += compare(rb.get(npdt), want[0 if coll == "reduce" else r], dtype, one, f"{what} rank {r}")
            if not rb.guards_ok() or not sb.guards_ok():
                errs.append(f"{what} rank {r}: bytes outside the buffers were written")
        for h in hs:
            comm.deregister_buffer(h)
    return errs


def run_with_scalar(cs, coll, dtype, bits, ins, device=False, **kw):
    """run() with operators created for the call and destroyed after it; device: ncclScalarDevice residence."""
    ds = [DevScalar(dtype, bits) for _ in cs] if device else [None] * len(cs)
    ops = [create_op(c, dtype, bits, d.ptr if d else None) for (c, _), d in zip(cs, ds)]
    errs = run(cs, coll, dtype, bits, ins, ops, **kw)
    for (c, _), op in zip(cs, ops):
        c.destroy_op(op)
    return errs


# ------------------------------------------------------------------------------------ spawned workers

def _worker_main(job, arg, env, q):
    try:
        os.environ["NCCL_AMD_SPIN_TIMEOUT_MS"] = "30000"
        os.environ["NCCL_MULTI_RANK_GPU_ENABLE"] = "1"
        os.environ.update(env)
        klog = f"/tmp/nccl_amd_premul_kernels_{os.getpid()}.log"
        dlog = f"/tmp/nccl_amd_premul_debug_{os.getpid()}.log"
        for f in (klog, dlog):
            if os.path.exists(f):
                os.remove(f)
        os.environ["NCCL_AMD_KERNEL_LOG"] = klog
        if "NCCL_DEBUG" in env:
            os.environ["NCCL_DEBUG_FILE"] = dlog
        import torch
        torch.cuda.set_device(0)
        errs = (job if callable(job) else JOBS[job])(arg)   # (another test file passes a function of its own)
        torch.cuda.synchronize()
        out = (errs, open(klog).read().splitlines() if os.path.exists(klog) else [],
               open(dlog).read() if os.path.exists(dlog) else "")
        for f in (klog, dlog):
            if os.path.exists(f):
                os.remove(f)
        q.put(out)
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put(([f"exception {e!r}\n{traceback.format_exc()}"], [], ""))


def spawn(jobs, timeout=240):
    """Run [(job, arg, env), ...] each in a fresh child process, all at once (at most four); returns their
    (errors, kernel log lines, debug log) in order. A worker that has not reported after `timeout` seconds is killed
    and fails the test."""
    _torch()
    assert len(jobs) <= 4
    ctx = mp.get_context("spawn")
    qs = [ctx.Queue() for _ in jobs]
    ps = [ctx.Process(target=_worker_main, args=(job, arg, env, q)) for (job, arg, env), q in zip(jobs, qs)]
    for p in ps:
        p.start()
    outs = []
    try:
        for (job, arg, _), q in zip(jobs, qs):
            try:
                outs.append(q.get(timeout=timeout))
            except queue.Empty:
                raise AssertionError(f"worker {job} {arg} did not report")
    finally:
        for p in ps:
            if len(outs) < len(ps) and p.is_alive():
                p.kill()
        for p in ps:
            p.join(timeout=60)
    return outs


def path_pattern(pattern, T, op):
    """A kernel name pattern ({T}, {OP}) compiled for the element type T and the operator template argument `op` (a
    number, or a regular expression such as "[0-3]")."""
    return re.compile(pattern.replace("{OP}", str(op)).replace("{T}", re.escape(T)))


def kernels_with_op3(klog, pattern, dtypes=ALL_TYPES):
    """For every datatype's kernel element type, the log line matching `pattern` with operator template argument 3
    (an AssertionError names the element types whose kernel never ran); returns the matched kernel names."""
    names, missing = [], []
    for T in sorted({KERNEL_TYPE[d] for d in dtypes}):
        rx = path_pattern(pattern, T, 3)
        hit = [m.group(0) for ln in klog for m in [rx.search(ln)] if m]
        if hit:
            names.append(hit[0])
        else:
            missing.append(T)
    assert not missing, (f"no kernel {pattern} in the log for {missing}; PreMulSum kernels logged: "
                         f"{[ln for ln in klog if ', 3' in ln][:40]}")
    return names


# ------------------------------------------------------------------------------------ 2. every type x every path

def path_cases(name, dtype):
    """The cases of one datatype on one path: (collective, scalar bits, count, misaligned, in place, device scalar)."""
    G = _G()
    es = _es(dtype)
    ll = name in ("LL", "LL128")
    count = 1027 if ll else 48 * 1024 // es + 3
    three = three_scalars(dtype)
    scalars = list(dict.fromkeys(three + (list(G.premul_scalars(dtype).values()) if name in FULL_LIST_PATHS else [])))
    cases = [("allreduce", s, count, False, False, i == 1) for i, s in enumerate(scalars)]
    # ReduceScatter: a rank block that is a multiple of 16 bytes, and one of 8 x odd bytes (no 16-byte packs)
    for blk in ((2064, 2056) if ll else (16400, 16392)):
        cases.append(("reducescatter", three[1], 3 * (blk // es), False, False, False))
    cases.append(("reduce", three[0], count, False, False, False))
    cases.append(("allreduce", three[1], count, True, False, False))
    cases.append(("allreduce", three[0], count, False, True, False))
    return cases


def _job_path(name):
    cs = comms_under(3)  # (the path's environment is this worker's environment)
    errs = []
    for dtype in ALL_TYPES:
        inputs = {}
        for k, (coll, bits, count, misaligned, inplace, device) in enumerate(path_cases(name, dtype)):
            if count not in inputs:
                inputs[count] = case_inputs(3, dtype, count, seed=1000 + 17 * dtype + len(inputs))
            errs += run_with_scalar(cs, coll, dtype, bits, inputs[count], device=device,
                                    mis=_es(dtype) if misaligned else 0, inplace=inplace, root=1,
                                    register=name == "REGISTERED", what=name)
        if len(errs) > 20:
            break
    destroy(cs)
    return errs


@pytest.mark.parametrize("path", list(PATHS))
def test_every_type_on_path(built, path):
    """All 12 datatypes through one kernel path at n = 3: AllReduce with three scalars (the whole list on LL and
    DIRECT; the second scalar from device memory), ReduceScatter with 16-byte and 8-byte blocks, Reduce to root 1, an
    AllReduce from bases misaligned by one element and one in place — against the oracle's fold for the path (ring,
    chain or partition where forced). The kernel log must name the path's AllReduce kernel with operator template
    argument 3 (DEV_PREMULSUM) for every element type: a path that cannot run a user operator fails here."""
    env, pattern = PATHS[path]
    (errs, klog, _), = spawn([("path", path, env)])
    assert not errs, "\n".join(errs[:20])
    names = kernels_with_op3(klog, pattern)
    print(f"\n[premulsum path {path}] kernels: {names}")


# ------------------------------------------------------------------------------------ 3. exhaustive small floats

def _fixed_allreduce(cs, dtype, sbufs, rbufs, count, bits):
    """AllReduce from preallocated buffers with a host-immediate operator created, used and destroyed here."""
    torch = _torch()
    import nccl_amd
    ops = [create_op(c, dtype, bits) for c, _ in cs]
    with nccl_amd.group():
        for (c, st), sb, rb, op in zip(cs, sbufs, rbufs, ops):
            c.all_reduce_raw(sb.ptr, rb.ptr, count, dtype, op, st.cuda_stream)
    for (c, _), op in zip(cs, ops):
        c.destroy_op(op)
    torch.cuda.synchronize()
    return [f"async error {c.async_error()}" for c, _ in cs if c.async_error()]


def _exhaustive(cs, dtype, ins, scalars, mis, cap_exempt=()):
    """Every scalar of `scalars` over the fixed inputs `ins` (n = 2), buffers allocated once."""
    G = _G()
    npdt = G.oracle.NP_STORAGE[dtype]
    count = ins[0].size
    sbufs = [Buf(x.nbytes, mis, x) for x in ins]
    rbufs = [Buf(x.nbytes, mis) for x in ins]
    errs = []
    for bits in scalars:
        want = G.oracle.all_reduce(ins, dtype, premul_scalar_bits=bits)
        if G.scalar_is_finite(dtype, bits) and bits not in cap_exempt:
            assert G.nan_cap_ok(want, dtype), f"dt={dtype} scalar={hex(bits)}: the oracle's result is > 10 % NaN"
        one = single_nan_mask(ins, dtype, bits)
        errs += _fixed_allreduce(cs, dtype, sbufs, rbufs, count, bits)
        for r, rb in enumerate(rbufs):
            errs += compare(rb.get(npdt), want, dtype, one, f"dt={dtype} scalar={hex(bits)} mis={mis} rank {r}")
        if len(errs) > 20:
            break
    if not all(b.guards_ok() for b in sbufs + rbufs):
        errs.append(f"dt={dtype} mis={mis}: bytes outside the buffers were written")
    return errs


def fp8_pair_inputs():
    return [np.repeat(np.arange(256, dtype=np.uint8), 256), np.tile(np.arange(256, dtype=np.uint8), 256)]


def half_pattern_inputs(dtype):
    """Rank 0: all 65,536 patterns; rank 1: the same permuted by i * 40503 mod 65536; signalling NaNs quieted (as
    tests/test_numerics.py: their handling is the hardware's)."""
    a = np.arange(65536, dtype=np.uint16)
    b = a[(np.arange(65536, dtype=np.int64) * 40503) % 65536].copy()
    qbit, expm = (0x200, 0x7C00) if dtype == 6 else (0x40, 0x7F80)
    for x in (a, b):
        snan = ((x & expm) == expm) & ((x & (qbit - 1)) != 0) & ((x & qbit) == 0)
        x[snan] |= qbit
    return [a, b]


def _job_exhaustive_fp8(dtype):
    cs = comms_under(2)
    ins = fp8_pair_inputs()
    errs = _exhaustive(cs, dtype, ins, range(256), 0)
    # one byte off 16-byte alignment: the per-element path
    sc = _G().premul_scalars(dtype)
    eight = [sc[k] for k in ("-2.5", "third", "minsub", "maxfinite", "-0", "0.375", "nan", "-1")]
    errs += _exhaustive(cs, dtype, ins, eight, 1)
    destroy(cs)
    return errs


def _job_exhaustive_half(dtype):
    """The scalar 'largest finite' overflows half of all patterns to +-Inf, and the permutation pairs many +Inf with
    -Inf: 19 % (fp16) / 13 % (bf16) of the oracle's result is NaN there, above the cap. That case still runs as the
    issue states it (NaN by position), and runs again with rank 1's signs copied from rank 0's, where opposite
    infinities cannot meet, the cap holds and those elements are compared bit for bit."""
    G = _G()
    cs = comms_under(2)
    ins = half_pattern_inputs(dtype)
    sc = G.premul_scalars(dtype)
    errs = _exhaustive(cs, dtype, ins, sc.values(), 0, cap_exempt=(sc["maxfinite"],))
    same_sign = [ins[0], (ins[1] & 0x7FFF) | (ins[0] & 0x8000)]
    errs += _exhaustive(cs, dtype, same_sign, [sc["maxfinite"], sc["-2.5"]], 0)
    destroy(cs)
    return errs


@pytest.mark.parametrize("dtype", [10, 11])
def test_fp8_every_triple_on_packed_fold(built, dtype):
    """fp8 on the staged direct kernel (n = 2, 16-byte aligned: numerics.h's packed-half fold, kernels.h foldFp8Packs):
    every (x0, x1) code pair under every one of the 256 scalar codes — 16.7 million triples — against the oracle.
    Packs without a NaN / Inf code stay on the half path, the others (and every pack under a NaN / Inf scalar) take
    fp8PackF32. Then eight scalars from bases one byte off alignment (the per-element functor)."""
    (errs, klog, _), = spawn([("exhaustive_fp8", dtype, DIRECT_SIMPLE)])
    assert not errs, "\n".join(errs[:20])
    kernels_with_op3(klog, r"collKernel<{T}, 3, 0>", [dtype])


@pytest.mark.parametrize("dtype", [6, 9])
def test_half_bf16_every_pattern_on_packed_fold(built, dtype):
    """fp16 / bf16 on the staged direct kernel's packed loop (n = 2): every bit pattern on rank 0 against a permutation
    of them on rank 1, under the whole scalar list (negative, zero, subnormal, huge, inexact, Inf, NaN)."""
    (errs, klog, _), = spawn([("exhaustive_half", dtype, DIRECT_SIMPLE)])
    assert not errs, "\n".join(errs[:20])
    kernels_with_op3(klog, r"collKernel<{T}, 3, 0>", [dtype])


# ------------------------------------------------------------------------------------ 4. one rank

def one_rank_counts(dtype):
    tile = 512 * (16 // _es(dtype))   # elements per tile of oneRankKernel
    return [1, 5, tile - 1, tile, tile + 1, 2 * tile + 16 // _es(dtype) + 1]


@pytest.fixture(scope="module")
def one_comm(built):
    cs = comms_under(1)
    yield cs
    destroy(cs)


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_one_rank_kernel(one_comm, dtype):
    """nRanks == 1 (kernels.h oneRankKernel, out = pre(in)) with a scalar that is not 1: counts around the tile and
    pack edges out of place and in place (in place must multiply too), bases misaligned by one element, a device
    scalar, and ReduceScatter / Reduce, which plan the same kernel; guard bytes on both sides of every output."""
    cs = one_comm
    es = _es(dtype)
    bits, other = three_scalars(dtype)[1], three_scalars(dtype)[0]
    counts = one_rank_counts(dtype)
    errs = []
    for k, count in enumerate(counts):
        ins = case_inputs(1, dtype, count, seed=300 + dtype)
        errs += run_with_scalar(cs, "allreduce", dtype, bits, ins)
        errs += run_with_scalar(cs, "allreduce", dtype, other, ins, inplace=True)
        if k in (1, 5):
            errs += run_with_scalar(cs, "allreduce", dtype, bits, ins, mis=es)
            errs += run_with_scalar(cs, "allreduce", dtype, other, ins, mis=es, inplace=True)
        if k in (2, 5):
            errs += run_with_scalar(cs, "allreduce", dtype, other, ins, device=True)
            errs += run_with_scalar(cs, "reducescatter", dtype, bits, ins)
            errs += run_with_scalar(cs, "reduce", dtype, other, ins, device=k == 5)
    assert not errs, "\n".join(errs[:20])


# ------------------------------------------------------------------------------------ 5. device scalars

LL_COUNT = 1000


def staged_count(dtype):
    return 160 * 1024 // _es(dtype) + 3   # beyond the LL range at n = 2 and n = 4 (enqueue.cc llPlan)


@pytest.fixture(scope="module")
def two_comms(built):
    cs = comms_under(2)
    yield cs
    destroy(cs)


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_device_scalar_follows_memory(two_comms, dtype):
    """ncclScalarDevice at an LL size and a staged size: the result equals ncclScalarHostImmediate's and the
    oracle's; after the device scalar is overwritten the SAME operator multiplies by the new value."""
    cs = two_comms
    a, b = three_scalars(dtype)[1], three_scalars(dtype)[0]
    errs = []
    for count in (LL_COUNT, staged_count(dtype)):
        ins = case_inputs(2, dtype, count, seed=500 + dtype)
        errs += run_with_scalar(cs, "allreduce", dtype, a, ins, what="host")
        ds = [DevScalar(dtype, a) for _ in cs]
        ops = [create_op(c, dtype, 0, d.ptr) for (c, _), d in zip(cs, ds)]
        errs += run(cs, "allreduce", dtype, a, ins, ops, what="device")
        for d in ds:
            d.set(b)
        errs += run(cs, "allreduce", dtype, b, ins, ops, what="device, overwritten")
        for (c, _), op in zip(cs, ops):
            c.destroy_op(op)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("dtype", [7, 9])
def test_device_scalar_under_graph_replay(two_comms, dtype):
    """One captured graph per rank: an LL-size and a staged-size AllReduce with a device-scalar operator and one
    AllReduce with a host-immediate operator. Each of three replays gets new inputs and a new device value: the
    device-scalar results follow it (the kernel reads the scalar when it runs, reference common.h / onerank.cu),
    the host-immediate result keeps the captured scalar."""
    torch = _torch()
    import nccl_amd
    G = _G()
    cs = two_comms
    comms = [c for c, _ in cs]
    npdt = G.oracle.NP_STORAGE[dtype]
    es = _es(dtype)
    sc = G.premul_scalars(dtype)
    host_bits = sc["0.375"]
    counts = [LL_COUNT, staged_count(dtype), LL_COUNT + 24]
    streams = [nccl_amd.dedicated_stream(0) for _ in comms]
    ds = [DevScalar(dtype, sc["1"]) for _ in comms]
    dev_ops = [create_op(c, dtype, 0, d.ptr) for c, d in zip(comms, ds)]
    host_ops = [create_op(c, dtype, host_bits) for c in comms]
    sb = [[Buf(n * es) for n in counts] for _ in comms]
    rb = [[Buf(n * es) for n in counts] for _ in comms]
    graphs = [torch.cuda.CUDAGraph() for _ in comms]
    torch.cuda.synchronize()
    for r, c in enumerate(comms):
        with torch.cuda.graph(graphs[r], stream=streams[r]):
            for k, n in enumerate(counts):
                c.all_reduce_raw(sb[r][k].ptr, rb[r][k].ptr, n, dtype, host_ops[r] if k == 2 else dev_ops[r],
                                 streams[r].cuda_stream)
    errs = []
    for it, name in enumerate(("-2.5", "third", "minsub")):
        ins = [case_inputs(2, dtype, n, seed=700 + 10 * it + k) for k, n in enumerate(counts)]
        for r in range(2):
            for k in range(3):
                sb[r][k].put(ins[k][r])
            ds[r].set(sc[name])
        torch.cuda.synchronize()
        for r in range(2):  # both ranks' graphs must run concurrently
            with torch.cuda.stream(streams[r]):
                graphs[r].replay()
        torch.cuda.synchronize()
        errs += [f"replay {it}: async error {c.async_error()}" for c in comms if c.async_error()]
        for k in range(3):
            bits = host_bits if k == 2 else sc[name]
            want = G.oracle.all_reduce(ins[k], dtype, premul_scalar_bits=bits)
            assert G.nan_cap_ok(want, dtype)
            one = single_nan_mask(ins[k], dtype, bits)
            for r in range(2):
                errs += compare(rb[r][k].get(npdt), want, dtype, one, f"replay {it} op {k} scalar {name} rank {r}")
                if not rb[r][k].guards_ok():
                    errs.append(f"replay {it} op {k} rank {r}: bytes outside the buffer were written")
    del graphs
    for c, d, h in zip(comms, dev_ops, host_ops):
        c.destroy_op(d)
        c.destroy_op(h)
    assert not errs, "\n".join(errs[:20])


def _job_rank_of_four(arg):
    """One rank of a four-process communicator on the one GPU, with a device scalar of its own."""
    import torch
    import nccl_amd
    rank, uid = arg
    comm = nccl_amd.Communicator.init(4, rank, uid)
    cs = [(comm, torch.cuda.Stream())]
    errs = []
    for dtype in (7, 9, 10, 2):
        a, b = three_scalars(dtype)[1], three_scalars(dtype)[0]
        ds = DevScalar(dtype, a)
        op = create_op(comm, dtype, 0, ds.ptr)
        for count in (LL_COUNT, staged_count(dtype)):
            G = _G()
            ins = case_inputs(4, dtype, count, seed=800 + dtype)
            for bits in (a, b):
                ds.set(bits)
                want = [G.oracle.all_reduce(ins, dtype, premul_scalar_bits=bits)] * 4
                assert G.nan_cap_ok(want[0], dtype)
                errs += _run_rank(cs, dtype, bits, ins, op, want, f"4 processes rank {rank}")
        comm.destroy_op(op)
    comm.destroy()
    return errs


def _run_rank(cs, dtype, bits, ins, op, want, what):
    """run() for a process that owns one rank of a larger communicator (no single-NaN mask: four ranks)."""
    torch = _torch()
    G = _G()
    (comm, stream), = cs
    es, npdt = _es(dtype), G.oracle.NP_STORAGE[dtype]
    sb, rb = Buf(ins[0].size * es, 0, ins[comm.rank]), Buf(ins[0].size * es)
    torch.cuda.synchronize()
    comm.all_reduce_raw(sb.ptr, rb.ptr, ins[0].size, dtype, op, stream.cuda_stream)
    stream.synchronize()
    if comm.async_error():
        return [f"{what}: async error {comm.async_error()}"]
    errs = compare(rb.get(npdt), want[comm.rank], dtype, None, f"{what} dt={dtype} scalar={hex(bits)} "
                                                                 f"count={ins[0].size}")
    if not rb.guards_ok():
        errs.append(f"{what}: bytes outside the buffer were written")
    return errs


def test_device_scalar_four_processes(built):
    """Four spawned processes on the one GPU, one rank each, every process with its own device-scalar allocation (a
    device pointer means nothing to a peer: each kernel must read its own rank's scalar): an LL-size and a
    staged-size AllReduce, the scalar overwritten between launches."""
    import nccl_amd
    _torch()
    uid = nccl_amd.get_unique_id()
    outs = spawn([("rank_of_four", (r, uid), {}) for r in range(4)])
    errs = [e for o in outs for e in o[0]]
    assert not errs, "\n".join(errs[:20])
    for _, klog, _ in outs:
        kernels_with_op3(klog, r"llKernel<{T}, 3, \d+, 0>", (7, 9, 10, 2))
        kernels_with_op3(klog, r"collKernel<{T}, 3, \d+>", (7, 9, 10, 2))


# ------------------------------------------------------------------------------------ 6. groups

GROUP_TYPES = (7, 9, 10, 3)


def _job_groups(_):
    """Per datatype and size class one group per rank: AllReduce with scalar A twice, with B, with a device scalar
    holding A, and a plain Sum — each checked against the oracle."""
    torch = _torch()
    import nccl_amd
    G = _G()
    cs = comms_under(2)
    errs = []
    for dtype in GROUP_TYPES:
        es, npdt = _es(dtype), G.oracle.NP_STORAGE[dtype]
        a, b = three_scalars(dtype)[1], three_scalars(dtype)[0]
        ds = [DevScalar(dtype, a) for _ in cs]
        ops = [[create_op(c, dtype, a), create_op(c, dtype, b), create_op(c, dtype, 0, d.ptr)]
               for (c, _), d in zip(cs, ds)]
        for count in (LL_COUNT, staged_count(dtype)):
            seq = [(0, a), (0, a), (1, b), (2, a), (None, None)]   # (operator index, its scalar); None = ncclSum
            ins = [case_inputs(2, dtype, count, seed=900 + 10 * dtype + k) for k in range(len(seq))]
            sb = [[Buf(count * es, 0, ins[k][r]) for k in range(len(seq))] for r in range(2)]
            rb = [[Buf(count * es) for _ in seq] for _ in range(2)]
            torch.cuda.synchronize()
            with nccl_amd.group():
                for r, (c, st) in enumerate(cs):
                    for k, (ix, _) in enumerate(seq):
                        c.all_reduce_raw(sb[r][k].ptr, rb[r][k].ptr, count, dtype, 0 if ix is None else ops[r][ix],
                                         st.cuda_stream)
            torch.cuda.synchronize()
            errs += [f"group dt={dtype} count={count}: async error {c.async_error()}" for c, _ in cs if c.async_error()]
            for k, (ix, bits) in enumerate(seq):
                want = G.oracle.all_reduce(ins[k], dtype, 0, premul_scalar_bits=bits)
                assert G.nan_cap_ok(want, dtype)
                one = single_nan_mask(ins[k], dtype, bits) if bits is not None and _is_float(dtype) else None
                for r in range(2):
                    errs += compare(rb[r][k].get(npdt), want, dtype, one,
                                    f"group dt={dtype} count={count} op {k} (scalar {bits and hex(bits)}) rank {r}")
                    if not rb[r][k].guards_ok():
                        errs.append(f"group dt={dtype} count={count} op {k} rank {r}: bytes outside the buffer written")
        for (c, _), o3 in zip(cs, ops):
            for op in o3:
                c.destroy_op(op)
    destroy(cs)
    return errs


def test_group_keeps_scalars_apart(built):
    """Several PreMulSum operators in one group: ops with the same scalar share a batch, a different scalar, a device
    scalar and a plain Sum do not take the first op's functor (enqueue.cc sameRedOp). The TRACE log must show, per
    rank, datatype and size class, a batch of at least two ops, and the kernel log the batched LL kernel and
    collBatchKernel with operator template argument 3."""
    (errs, klog, dlog), = spawn([("groups", None, {"NCCL_DEBUG": "TRACE"})])
    assert not errs, "\n".join(errs[:20])
    ll = [int(m) for m in re.findall(r"LL batch: (\d+) ops", dlog)]
    staged = [int(m) for m in re.findall(r"staged batch: (\d+) AllReduce ops", dlog)]
    want = 2 * len(GROUP_TYPES)   # two ranks
    assert len(ll) >= want and min(ll) >= 2, f"LL batches {ll}"
    assert len(staged) >= want and min(staged) >= 2, f"staged batches {staged}"
    # the batches are exactly the same-scalar pairs: a batch of three or more would have merged two scalars
    assert max(ll) == 2 and max(staged) == 2, f"LL {ll} staged {staged}"
    names = kernels_with_op3(klog, r"llKernel<{T}, 3, 8, 0>", GROUP_TYPES)
    names += kernels_with_op3(klog, r"collBatchKernel<{T}, 3, \d+>", GROUP_TYPES)
    print(f"\n[premulsum groups] kernels: {names}")


def test_operator_api_edges(two_comms):
    """A datatype other than the operator's, a destroyed or never-created operator and an invalid residence give
    ncclInvalidArgument; a create after a destroy reuses the slot with the new scalar; the communicator stays usable."""
    torch = _torch()
    import nccl_amd
    G = _G()
    cs = two_comms
    c0, st0 = cs[0]
    count = 256
    ins = case_inputs(2, 7, count, seed=77)
    x, y = Buf(count * 4, 0, ins[0]), Buf(count * 4)
    sc = G.premul_scalars(7)

    def rejected(dtype, op):
        with pytest.raises(nccl_amd.NcclError) as e:
            c0.all_reduce_raw(x.ptr, y.ptr, count, dtype, op, st0.cuda_stream)
        assert e.value.code == INVALID_ARGUMENT, e.value

    op = create_op(c0, 7, sc["-2.5"])
    rejected(2, op)          # int32 data, fp32 operator
    rejected(9, op)
    c0.destroy_op(op)
    rejected(7, op)          # destroyed
    with pytest.raises(nccl_amd.NcclError) as e:
        c0.destroy_op(op)
    assert e.value.code == INVALID_ARGUMENT
    rejected(7, op + 9)      # never created
    scal = ctypes.create_string_buffer(int(sc["third"]).to_bytes(8, "little"), 8)
    h = ctypes.c_int(-1)
    for residence in (2, -1):
        rc = nccl_amd.load().ncclRedOpCreatePreMulSum(ctypes.byref(h), scal, 7, residence, c0.ptr)
        assert rc == INVALID_ARGUMENT, rc
    assert nccl_amd.load().ncclRedOpCreatePreMulSum(ctypes.byref(h), scal, 12, 1, c0.ptr) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert y.guards_ok() and np.all(y.get(np.uint8) == FILL), "a rejected call wrote its output"
    assert not c0.async_error()
    # the freed slot is reused and carries the new scalar, on both ranks
    ops = [create_op(c, 7, sc["third"]) for c, _ in cs]
    assert ops[0] == op, (ops, op)
    errs = run(cs, "allreduce", 7, sc["third"], ins, ops, what="reused slot")
    for (c, _), o in zip(cs, ops):
        c.destroy_op(o)
    # and the communicator still runs a built-in operator
    errs += G.run_case(cs, "allreduce", 7, 0, 5000, 0, seed=3)
    assert not errs, "\n".join(errs[:20])


JOBS = {"path": _job_path, "exhaustive_fp8": _job_exhaustive_fp8, "exhaustive_half": _job_exhaustive_half,
        "rank_of_four": _job_rank_of_four, "groups": _job_groups}
