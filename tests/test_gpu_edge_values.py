"""GPU tests of the built-in operators (Sum, Prod, Max, Min, Avg) on fp16 / bf16 / fp32 / fp64 over edge-value pairs,
through every kernel path, bit for bit against the CPU oracle's fold for that path.

The inputs are gpu_cases.edge_inputs: every fp16 / bf16 bit pattern (fp32 / fp64: every sign and exponent with the
mantissas at the edges of the field) against 18 partners built to hit rounding ties from both sides, overflow to
+-Inf, exact and near cancellation, subnormal results, signed zeros and every NaN. tests/test_numerics.py runs the
same inputs through the host build of numerics.h; the device compiles other code for the same functors (native
_Float16 arithmetic, packed or scalar; the hardware bf16 convert), which only these tests run.

Each case is one spawned worker (its environment forces the path; it writes the kernel log, as
tests/test_gpu_premulsum.py): AllReduce of the whole set at n = 2 and n = 3 for the five operators, in slices of
48 KiB + 3 elements — what every forced path takes, each slice 16-byte aligned at its start and ending in the
per-element tail — from buffers allocated once. On LL and DIRECT also ReduceScatter and Reduce (root 1) at n = 3, and
on DIRECT one whole-set AllReduce per operator from bases one element off 16-byte alignment (kernels.h foldRange's
per-element loop).

Comparison: gpu_cases.same_bits (every bit; a NaN where the oracle has one) under the 10 % NaN cap, plus bit for bit
the elements gpu_cases.defined_mask names (Sum / Prod / Avg: exactly one NaN in the fold; Min / Max: every element).
The bytes between the slices and around every buffer must keep their fill. The kernel log must name the path's
kernel for the element type with the operator template arguments 0 (Sum), 1 (Prod), 2 (Min / Max) and 3 (float Avg is
PreMulSum by 1/n), and no other kernel of that element type."""
import re

import numpy as np
import pytest

from tests.test_gpu_premulsum import FILL, KERNEL_TYPE, PATHS, Buf, comms_under, destroy, path_pattern, spawn

pytestmark = pytest.mark.gpu

OPS = (0, 1, 2, 3, 4)                       # ncclSum, ncclProd, ncclMax, ncclMin, ncclAvg
OP_ARG = {0: 0, 1: 1, 2: 2, 3: 2, 4: 3}     # the kernels' operator template argument (float Avg: DEV_PREMULSUM)
EVERY_TYPE_PATHS = ("LL", "DIRECT", "RING")  # fp32 and fp64 run on these; fp16 and bf16 on all eight
EDGE_PATHS = ("LL", "LL128", "ONESHOT", "DIRECT", "REGISTERED", "RING", "TREE", "REF_ORDER")
CASES = [(p, d) for p in EDGE_PATHS for d in ((6, 9, 7, 8) if p in EVERY_TYPE_PATHS else (6, 9))]
# the kernels of ReduceScatter and Reduce on the staged path (kernels.h Coll: COLL_RS = 1, COLL_REDUCE = 3); the LL
# kernel runs every collective
EXTRA_KERNELS = {"LL": (), "DIRECT": (r"collKernel<{T}, {OP}, 1>", r"collKernel<{T}, {OP}, 3>")}
WORKER_SECONDS = 150


def _G():
    from tests import gpu_cases as G
    return G


def _es(dtype):
    return np.dtype(_G().oracle.NP_STORAGE[dtype]).itemsize


def slice_elems(dtype):
    """48 KiB + 3 elements: tests/test_gpu_collectives.py test_every_path_same_bits_with_specials runs this count on
    every forced path at n = 3 (enqueue.cc's LL capacity holds it); never a multiple of 16 bytes."""
    return 48 * 1024 // _es(dtype) + 3


def rs_block_elems(dtype):
    """ReduceScatter: elements per rank and slice, 16 KiB + 8 elements (test_reduce_paths_same_bits_with_specials): a
    multiple of 8 bytes, which the LL kernel needs for blocked collectives (enqueue.cc llPlan `shape`)."""
    return 16 * 1024 // _es(dtype) + 8


class Sliced:
    """`total` elements in slices of at most `per` elements: slice k lies at byte k * stride of one guarded device
    buffer, stride a multiple of 16 bytes that leaves at least 16 bytes of fill after every slice."""

    def __init__(self, total, per, es, data=None):
        self.total, self.per, self.es = total, per, es
        self.k = -(-total // per)
        self.stride = (per * es + 15) // 16 * 16 + 16
        raw = np.full(self.k * self.stride, FILL, dtype=np.uint8)
        self.used = np.zeros(raw.size, dtype=bool)
        for i in range(self.k):
            nb = self.count(i) * es
            self.used[i * self.stride: i * self.stride + nb] = True
            if data is not None:
                seg = np.ascontiguousarray(data[i * per: i * per + self.count(i)]).view(np.uint8)
                raw[i * self.stride: i * self.stride + nb] = seg
        self.buf = Buf(raw.size, 0, raw)
        assert self.buf.ptr % 16 == 0

    def count(self, i):
        return min(self.per, self.total - i * self.per)

    def ptr(self, i):
        return self.buf.ptr + i * self.stride

    def clear(self):
        self.buf.store.fill_(FILL)

    def read(self, npdt):
        """(the elements of every slice in order, whether every byte outside the slices kept its fill)."""
        raw = self.buf.get(np.uint8)
        return raw[self.used].view(npdt), bool(self.buf.guards_ok() and np.all(raw[~self.used] == FILL))


def _sliced_expected(coll, ins, dtype, op, per, root):
    """The oracle's result of the collective run slice by slice (the fold order follows the position inside the call):
    one array per rank that has an output."""
    G = _G()
    n, total = len(ins), ins[0].size
    outs = None
    for lo in range(0, total, per):
        exp = G.expected(coll, [x[lo: lo + per] for x in ins], dtype, op, root)
        outs = [[e] for e in exp] if outs is None else [o + [e] for o, e in zip(outs, exp)]
    return [np.concatenate(o) for o in outs]


def _sliced_mask(coll, one, n, per):
    """defined_mask `one` (over the input elements) as seen by each rank's output."""
    if coll != "reducescatter":
        return [one] * n
    parts = [[] for _ in range(n)]
    for lo in range(0, one.size, per):
        blk = min(per, one.size - lo) // n
        for r in range(n):
            parts[r].append(one[lo + r * blk: lo + (r + 1) * blk])
    return [np.concatenate(p) for p in parts]


def run_set(cs, coll, dtype, ins, per, register, what, root=1):
    """`coll` over the whole inputs `ins` in slices of `per` input elements for the five operators, buffers allocated
    (and registered, for the zero-copy path) once; returns errors."""
    import torch
    import nccl_amd
    G = _G()
    n, es, npdt = len(cs), _es(dtype), G.oracle.NP_STORAGE[dtype]
    total = ins[0].size
    assert len(ins) == n and (coll != "reducescatter" or (per % n == 0 and total % n == 0))
    oper = per // n if coll == "reducescatter" else per
    sb = [Sliced(total, per, es, x) for x in ins]
    rb = [Sliced(total // n if coll == "reducescatter" else total, oper, es)
          if coll != "reduce" or r == root else None for r in range(n)]
    hs = []
    if register:
        for (c, _), s, r in zip(cs, sb, rb):
            hs += [(c, c.register_buffer(b.buf.store.data_ptr(), b.buf.store.numel())) for b in (s, r)]
    errs = []
    for op in OPS:
        w = f"{what} {coll} n={n} dt={dtype} op={op}"
        want = _sliced_expected(coll, ins, dtype, op, per, root)
        assert G.nan_cap_ok(np.concatenate(want), dtype), f"{w}: more than 10 % of the oracle's result is NaN"
        one = _sliced_mask(coll, G.defined_mask(ins, dtype, op), n, per)
        for r in rb:
            if r is not None:
                r.clear()
        torch.cuda.synchronize()
        for i in range(sb[0].k):
            cnt = sb[0].count(i)
            with nccl_amd.group():
                for (c, st), s, r in zip(cs, sb, rb):
                    if coll == "allreduce":
                        c.all_reduce_raw(s.ptr(i), r.ptr(i), cnt, dtype, op, st.cuda_stream)
                    elif coll == "reducescatter":
                        c.reduce_scatter_raw(s.ptr(i), r.ptr(i), cnt // n, dtype, op, st.cuda_stream)
                    else:
                        c.reduce_raw(s.ptr(i), r.ptr(i) if r is not None else None, cnt, dtype, op, root,
                                     st.cuda_stream)
        torch.cuda.synchronize()
        errs += [f"{w} rank {c.rank}: async error {c.async_error()}" for c, _ in cs if c.async_error()]
        if errs:
            break
        k = 0
        for rank, r in enumerate(rb):
            if r is None:
                continue
            got, clean = r.read(npdt)
            errs += G.edge_errors(got, want[k], one[rank], dtype, f"{w} rank {rank}")
            if not clean:
                errs.append(f"{w} rank {rank}: bytes outside the output slices were written")
            k += 1
        if len(errs) > 20:
            break
    if not all(s.read(npdt)[1] for s in sb):
        errs.append(f"{what} {coll} n={n} dt={dtype}: bytes outside the input slices were written")
    for c, h in hs:
        c.deregister_buffer(h)
    return errs


def run_misaligned(cs, dtype, ins, what):
    """One AllReduce of the whole set per operator from bases one element off 16-byte alignment."""
    import torch
    import nccl_amd
    G = _G()
    es, npdt = _es(dtype), G.oracle.NP_STORAGE[dtype]
    total = ins[0].size
    sb = [Buf(total * es, es, x) for x in ins]
    rb = [Buf(total * es, es) for _ in ins]
    errs = []
    for op in OPS:
        w = f"{what} allreduce off alignment n={len(cs)} dt={dtype} op={op}"
        want = G.expected("allreduce", ins, dtype, op)[0]
        assert G.nan_cap_ok(want, dtype), f"{w}: more than 10 % of the oracle's result is NaN"
        one = G.defined_mask(ins, dtype, op)
        torch.cuda.synchronize()
        with nccl_amd.group():
            for (c, st), s, r in zip(cs, sb, rb):
                c.all_reduce_raw(s.ptr, r.ptr, total, dtype, op, st.cuda_stream)
        torch.cuda.synchronize()
        errs += [f"{w} rank {c.rank}: async error {c.async_error()}" for c, _ in cs if c.async_error()]
        if errs:
            break
        for rank, r in enumerate(rb):
            errs += G.edge_errors(r.get(npdt), want, one, dtype, f"{w} rank {rank}")
        if len(errs) > 20:
            break
    if not all(b.guards_ok() for b in sb + rb):
        errs.append(f"{what} off alignment dt={dtype}: bytes outside the buffers were written")
    return errs


def _job_edge(arg):
    """One (path, dtype) case; the path's environment is this worker's."""
    path, dtype = arg
    G = _G()
    errs = []
    for n in (2, 3):
        cs = comms_under(n)
        ins = G.edge_inputs(dtype, n)
        errs += run_set(cs, "allreduce", dtype, ins, slice_elems(dtype), path == "REGISTERED", path)
        if path in EXTRA_KERNELS and n == 3 and not errs:
            errs += run_set(cs, "reducescatter", dtype, ins, 3 * rs_block_elems(dtype), False, path)
            errs += run_set(cs, "reduce", dtype, ins, slice_elems(dtype), False, path)
        if path == "DIRECT" and n == 2 and not errs:
            errs += run_misaligned(cs, dtype, ins, path)
        destroy(cs)
        if errs:
            break
    return errs


def check_kernel_log(klog, path, dtype, args=(0, 1, 2, 3), extra=None):
    """The log names, for the case's element type, the path's kernel with each of the operator template arguments
    `args` (floats: 0, 1, 2 and 3) — and with each the `extra` kernel patterns, by default the ReduceScatter and
    Reduce kernels on DIRECT — and no other kernel of that type; returns the names."""
    T = KERNEL_TYPE[dtype]
    typed = sorted({ln.split(" grid=")[0] for ln in klog if f"<{T}, " in ln})
    patterns = (PATHS[path][1],) + (EXTRA_KERNELS.get(path, ()) if extra is None else extra)
    missing = [(p, arg) for p in patterns for arg in args
               if not any(path_pattern(p, T, arg).search(ln) for ln in typed)]
    assert not missing, f"{path} dt={dtype}: no kernel for {missing}; kernels of {T} in the log: {typed}"
    any_arg = "[" + "".join(str(a) for a in args) + "]"
    other = [ln for ln in typed if not any(path_pattern(p, T, any_arg).search(ln) for p in patterns)]
    assert not other, f"{path} dt={dtype}: kernels of {T} that are not the path's: {other}"
    return typed


@pytest.mark.parametrize("path,dtype", CASES, ids=[f"{p}-{d}" for p, d in CASES])
def test_edge_values_on_path(built, path, dtype):
    """The edge-value pairs of one float type through one kernel path: see the module docstring."""
    env, _ = PATHS[path]
    (errs, klog, _), = spawn([(_job_edge, (path, dtype), env)], timeout=WORKER_SECONDS)
    assert not errs, "\n".join(errs[:20])
    names = [re.sub(r"^void |ncclamd::|\(.*$", "", s) for s in check_kernel_log(klog, path, dtype)]
    print(f"\n[edge values {path} dt={dtype}] kernels: {names}")
