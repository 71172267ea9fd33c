"""GPU tests of every collective at its partition boundaries, through guarded and poisoned arenas.

The counts come from gpu_cases.boundary_counts: derived from the plan so that rank blocks, channel parts, pipeline
slices, LL lines, size-table crossovers and the reference partition's loops each hit their edge cases (empty, one
element, one short of full, exactly full, one step past a wrap); tests/test_boundaries_cpu.py checks on the CPU that
each count hits what it claims. Here every count runs on the GPU under the path's small geometry
(gpu_cases.BOUNDARY_ENVS), each (path, n) in one spawned worker whose environment forces the path.

Per element type (uint8, fp16, int32, fp64: one per element size) a rank's sendbuffs live in one device arena and its
recvbuffs in another (gpu_cases.arena_layout), uploaded once and read back once. Outputs are prefilled with the
complement of the oracle's result. After the run every output must equal the oracle's bit for bit (the inputs are
finite, so no NaN rule applies), every byte around and between the slots must keep its fill, every sendbuff must be
unchanged and no communicator may report an async error (gpu_cases.arena_errors). Every count runs out of place with
Sum, the first collective's counts again with Max; the counts whose classes name a rank block, a last slice or an LL
line run again in place and from bases one element off 16-byte alignment; Reduce runs with every root. The kernel log
must name the path's kernels for every element type and no other kernel; the kernels of the counts built to leave an
LL path are listed in FALL_OFF."""
import re

import numpy as np
import pytest

from tests import gpu_cases as G
from tests.test_gpu_edge_values import WORKER_SECONDS
from tests.test_gpu_premulsum import comms_under, destroy, spawn

pytestmark = pytest.mark.gpu

TYPES = (1, 6, 2, 8)            # uint8, fp16, int32, fp64
SUM, MAX = 0, 2
SPIN = {"NCCL_AMD_SPIN_TIMEOUT_MS": "10000"}   # a mismatch between ranks ends as an async error, not as a wait
# the element type a kernel is instantiated for; AllGather is type-erased to the unsigned type of the element size
KERNEL_T = {1: "unsigned char", 6: "ncclamd::half_t", 2: "unsigned int", 8: "double"}
GATHER_T = {1: "unsigned char", 6: "unsigned short", 2: "unsigned int", 8: "unsigned long"}
OP_ARG = {SUM: 0, MAX: 2}
# (kernel, trailing template arguments) of each path's own kernel per collective: kernels.h Coll / SymColl, pipe.h kinds
_STAGED = {"allreduce": ("collKernel", "0"), "reducescatter": ("collKernel", "1"), "allgather": ("collKernel", "2"),
           "reduce": ("collKernel", "3")}
_LL = {c: ("llKernel", "1, 0") for c in _STAGED}
_LL128 = {c: ("llKernel", "1, 1") for c in _STAGED}
PATH_KERNELS = {
    "DIRECT": _STAGED, "PULLS_AG0": _STAGED, "PULLS_AG1": _STAGED, "ONESHOT": {"allreduce": ("collKernel", "4")},
    "LL": _LL, "LL128": _LL128,
    "RING": {"allreduce": ("pipeKernel", "0"), "reducescatter": ("pipeKernel", "1"), "allgather": ("pipeKernel", "2"),
             "reduce": ("pipeKernel", "4")},
    "TREE": {"allreduce": ("pipeKernel", "3")},
    "REF_ORDER": {"allreduce": ("collKernel", "5")}, "REF_SUB": {"allreduce": ("collKernel", "5")},
    "WINDOW": {"allreduce": ("symKernel", "0"), "reducescatter": ("symKernel", "2"), "allgather": ("symKernel", "3")},
    "WINDOW_ONESHOT": {"allreduce": ("symKernel", "1")},
}
# where the counts built to leave an LL path run (beyond the line capacity; ReduceScatter / AllGather blocks off 8
# bytes): the default algorithm's one-shot AllReduce and the staged kernels
FALL_OFF = {"allreduce": ("collKernel", "4"), "reducescatter": ("collKernel", "1"), "allgather": ("collKernel", "2"),
            "reduce": ("collKernel", "3")}
# the size-table path runs the default algorithm's four AllReduce kernels back to back on one communicator
TABLE_KERNELS = (("llKernel", "1, 0"), ("llKernel", "1, 1"), ("collKernel", "4"), ("collKernel", "0"))
VARIANT_CLASSES = ("last block", "last slice", "LL bytes mod", "LL128 bytes mod", "last LL channel", "LL block")
CASES = [(p, n) for p in G.BOUNDARY_ENVS for n in (2, 3)]


def build_cases(path, n, dtype):
    """The arena cases of one element type on one path: see the module docstring."""
    cases = []
    for k, coll in enumerate(G.BOUNDARY_COLLS[path]):
        roots = range(n) if coll == "reduce" else (0,)
        for count, classes in G.boundary_counts(path, coll, n, dtype):
            tag = f"{path} n={n} [{', '.join(sorted(classes))}]"
            for root in roots:
                cases.append(G.ArenaCase(coll, dtype, SUM, count, root, tag=tag))
                if k == 0:
                    cases.append(G.ArenaCase(coll, dtype, MAX, count, root, tag=tag))
                if any(c.startswith(VARIANT_CLASSES) for c in classes):
                    if path != "WINDOW_ONESHOT":   # (NCCL_AMD_SYM_ONESHOT=1 declares every AllReduce out of place)
                        cases.append(G.ArenaCase(coll, dtype, SUM, count, root, inplace=True, tag=tag))
                    cases.append(G.ArenaCase(coll, dtype, SUM, count, root, mis=1, tag=tag))
    return cases


def group_counts(dtype=2):
    """Eight AllReduce counts of the direct geometry at n = 2 for ONE group: both counts of each pair where the
    channel count steps from k to k + 1, the generated count of NSLOTS + 1 steps with the count below it, and the
    pair at which the step count goes from NSLOTS to NSLOTS + 1."""
    gen = G.boundary_counts("DIRECT", "allreduce", 2, dtype)
    pick = []
    for count, classes in gen:
        if any(c.startswith("nch ") for c in classes):
            pick += [count, count + 1]
        if "steps=NSLOTS+1" in classes:
            pick += [count - 1, count]
    # and the pair at which the step count itself goes from NSLOTS to NSLOTS + 1 (the steps grow with the count)
    nslots = G.boundary_geom("DIRECT", 2).nslots
    es = np.dtype(G.oracle.NP_STORAGE[dtype]).itemsize
    lo, hi = 1, max(pick)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if G.model_plan("DIRECT", "allreduce", 2, es, mid)["steps"] > nslots else (mid, hi)
    pick = list(dict.fromkeys(pick + [lo, hi]))
    assert len(pick) == 8, pick
    return pick


def group_cases(dtype=2):
    return [G.ArenaCase("allreduce", dtype, SUM, c, tag="DIRECT n=2 one group") for c in group_counts(dtype)]


def run_arena(cs, cases, window=False, one_group=False):
    """Run `cases` on the communicators `cs` through one send arena and one recv arena per rank; returns errors."""
    import torch
    import nccl_amd
    n = len(cs)
    sizes = G.arena_layout(cases, n)
    ins, exp = {}, {}
    inputs, wants = [], []
    for cs_ in cases:
        ki = (cs_.dtype, cs_.count)
        if ki not in ins:
            ins[ki] = G.make_inputs(n, cs_.dtype, cs_.count, seed=7 + cs_.count % 1009 + 31 * cs_.dtype)
        kw = (cs_.coll, cs_.dtype, cs_.op, cs_.count, cs_.root if cs_.coll == "reduce" else 0)
        if kw not in exp:
            e = G.expected(cs_.coll, ins[ki], cs_.dtype, cs_.op, cs_.root)
            exp[kw] = [e[0] if r == cs_.root else None for r in range(n)] if cs_.coll == "reduce" else list(e)
        inputs.append(ins[ki])
        wants.append(exp[kw])
    before = G.arena_images(cases, n, sizes, inputs, wants)
    dev = [(torch.from_numpy(s).cuda(), torch.from_numpy(r).cuda()) for s, r in before]   # one upload per arena
    assert all(t.data_ptr() % 16 == 0 for pair in dev for t in pair)
    wins = []
    if window:   # (one window per communicator and group, as every rank's registration of it is one collective)
        for which in (0, 1):
            with nccl_amd.group():
                wins += [(comm, comm.register_window(pair[which].data_ptr(), pair[which].numel()))
                         for (comm, _), pair in zip(cs, dev)]
        assert all(w.handle for _, w in wins)
    torch.cuda.synchronize()

    def issue(case):
        for (comm, stream), (sd, rd) in zip(cs, dev):
            r = comm.rank
            which, off = case.send_ptr_off(n, r)
            sp = (sd if which == "send" else rd).data_ptr() + off
            reg = case.out_region(n, r)
            rp = None if reg is None else rd.data_ptr() + reg[0]
            if case.coll == "reduce" and rp is None and case.inplace:
                rp = sp
            st = stream.cuda_stream
            if case.coll == "allreduce":
                comm.all_reduce_raw(sp, rp, case.count, case.dtype, case.op, st)
            elif case.coll == "reducescatter":
                comm.reduce_scatter_raw(sp, rp, case.count // n, case.dtype, case.op, st)
            elif case.coll == "allgather":
                comm.all_gather_raw(sp, rp, case.count, case.dtype, st)
            else:
                comm.reduce_raw(sp, rp, case.count, case.dtype, case.op, case.root, st)

    errs = []
    try:
        if one_group:
            with nccl_amd.group():
                for case in cases:
                    issue(case)
        else:
            for k, case in enumerate(cases):
                with nccl_amd.group():
                    issue(case)
                if k % 32 == 31 and any(c.async_error() for c, _ in cs):
                    errs.append(f"async error by case {k}: {case.what()}")
                    break
        torch.cuda.synchronize()
        errs += [f"rank {c.rank}: async error {c.async_error()}" for c, _ in cs if c.async_error()]
        if not errs:
            after = [(s.cpu().numpy(), r.cpu().numpy()) for s, r in dev]                  # one readback per arena
            errs = G.arena_errors(cases, n, before, after, wants)
    finally:
        for comm, w in wins:
            comm.deregister_window(w)
    return errs


def _job_boundary(arg):
    """One (path, n); the path's environment is this worker's."""
    path, n = arg
    cs = comms_under(n)
    errs, ran = [], 0
    try:
        for dtype in TYPES:
            cases = build_cases(path, n, dtype)
            ran += len(cases)
            errs += run_arena(cs, cases, window=path in G.BOUNDARY_WINDOW_PATHS)
            if errs:
                break
    finally:
        destroy(cs)
    return [f"ran={ran}"] + errs


def _job_group(_):
    cs = comms_under(2)
    try:
        return run_arena(cs, group_cases(), one_group=True)
    finally:
        destroy(cs)


_KERNEL = re.compile(r"(\w+Kernel)<([^,<>]+), (\d+), ([0-9, ]+)>")


def logged_kernels(klog):
    """{(kernel, element type, operator argument, trailing template arguments)} of the channel kernels in the log."""
    out = set()
    for ln in klog:
        m = _KERNEL.search(ln)
        if m:
            out.add((m.group(1), m.group(2).replace("ncclamd::", ""), int(m.group(3)), m.group(4).strip()))
    return out


def expected_kernels(path):
    """(the kernels the log must name, the kernels it may name besides) for a (path, n) worker."""
    must, may = set(), set()
    for dtype in TYPES:
        T, TG = KERNEL_T[dtype].replace("ncclamd::", ""), GATHER_T[dtype]
        for k, coll in enumerate(G.BOUNDARY_COLLS[path]):
            ops = (SUM, MAX) if k == 0 else (SUM,)
            kinds = TABLE_KERNELS if path == "TABLE" else (PATH_KERNELS[path][coll],)
            for name, tail in kinds:
                for op in ops:
                    must.add((name, TG, 0, tail) if coll == "allgather" else (name, T, OP_ARG[op], tail))
            if path in ("LL", "LL128"):
                name, tail = FALL_OFF[coll]
                for op in ops:
                    may.add((name, TG, 0, tail) if coll == "allgather" else (name, T, OP_ARG[op], tail))
    return must, may


@pytest.mark.parametrize("path,n", CASES, ids=[f"{p}-n{n}" for p, n in CASES])
def test_boundary_counts_on_path(built, path, n):
    """Every boundary count of one path at one rank count: see the module docstring."""
    env = dict(G.BOUNDARY_ENVS[path], **SPIN)
    (errs, klog, _), = spawn([(_job_boundary, (path, n), env)], timeout=WORKER_SECONDS)
    ran, errs = [e for e in errs if e.startswith("ran=")], [e for e in errs if not e.startswith("ran=")]
    assert not errs and ran, "\n".join(errs[:20])
    got = logged_kernels(klog)
    must, may = expected_kernels(path)
    assert must <= got, f"{path} n={n}: kernels that never ran: {sorted(must - got)}; logged: {sorted(got)}"
    # the fall-off kernels of an LL path must run where its counts leave it: the one-shot AllReduce and the staged
    # Reduce beyond the line capacity (every type has such counts), the staged ReduceScatter / AllGather for blocks
    # off 8 bytes (every element size below 8 bytes)
    if path in ("LL", "LL128"):
        off8 = {"unsigned long", "double"}
        need = {k for k in may if k[3] in ("3", "4") or k[1] not in off8}
        assert need <= got, f"{path} n={n}: fall-off kernels that never ran: {sorted(need - got)}"
    assert got <= must | may, f"{path} n={n}: kernels that are not the path's: {sorted(got - must - may)}"
    print(f"\n[boundaries {path} n={n}] {ran[0]} calls, kernels: {sorted(got)}")


def test_group_batch_at_boundaries(built):
    """Eight boundary counts in one group on the direct geometry at n = 2: one collBatchKernel launch, its channel
    offsets wrapping the channel cap, checked through the same arenas."""
    env = dict(G.BOUNDARY_ENVS["DIRECT"], **SPIN)
    (errs, klog, _), = spawn([(_job_group, None, env)], timeout=WORKER_SECONDS)
    assert not errs, "\n".join(errs[:20])
    assert logged_kernels(klog) == {("collBatchKernel", "unsigned int", 0, "0")}, klog
