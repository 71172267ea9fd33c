"""ncclPutSignal / ncclSignal / ncclWaitSignal without a GPU: the exported symbols and their Python bindings, the
null-comm check, every row of the argument table and the batching rules (tests/native/rma_plan_test: rma.cc and
group.cc with the kernel launches recorded instead of run), and the new kernels' register budget from the build's
report."""
import ctypes
import os
import subprocess

import pytest

from tests.test_occupancy import _reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"ncclPutSignal": 11, "ncclSignal": 6, "ncclWaitSignal": 4}
INVALID_ARGUMENT = 4
REFUSED = ("put_type13", "put_peer4", "signal_peer-1",
           "put_ctx1", "put_sigidx1", "put_flags1", "signal_ctx1", "signal_sigidx1", "signal_flags1",
           "put_nullwin", "put_nullbuff", "put_nullbuff_count0", "put_src_outside", "put_src_nonsym", "put_unknown_win",
           "put_past_peer0", "put_offset_past_peer0", "put_huge_offset",
           "wait_nulldescs", "wait_ndesc0", "wait_opcnt0", "wait_sigidx1", "wait_ctx1", "wait_peer4", "wait_peer-1")
ACCEPTED = ("put_end_peer0", "put_within_peer2", "put_ok", "put_self_ok", "put_count0_ok", "signal_ok", "wait_ok")


@pytest.fixture(scope="module")
def exe(built):
    path = os.path.join(ROOT, "tests", "native", "rma_plan_test")
    subprocess.check_call(["make", "rma-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    return path


def _run(exe, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    out = subprocess.run([exe, *args], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [dict(kv.split("=", 1) for kv in line.split() if "=" in kv) for line in out.stdout.splitlines() if "=" in line]


def test_symbols_exported_and_bound(built):
    import nccl_amd
    lib = ctypes.CDLL(nccl_amd.LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name in FUNCS:
        assert hasattr(lib, name), name
        assert hasattr(lib, "p" + name), "p" + name
    assert set(FUNCS) <= set(nccl_amd.EXPORTED)
    bound = nccl_amd.load()
    for name, arity in FUNCS.items():
        f = getattr(bound, name)
        assert f.argtypes is not None and len(f.argtypes) == arity, name
    for method in ("put_signal", "put_signal_raw", "signal", "wait_signal"):
        assert callable(getattr(nccl_amd.Communicator, method)), method
    assert ctypes.sizeof(nccl_amd.WaitSignalDesc) == 16
    assert [f[0] for f in nccl_amd.WaitSignalDesc._fields_] == ["opCnt", "peer", "sigIdx", "ctx"]


def test_null_comm_rejected_like_allreduce(built):
    import nccl_amd
    lib = nccl_amd.load()
    want = lib.ncclAllReduce(None, None, 1, 7, 0, None, None)
    assert want != 0
    desc = (nccl_amd.WaitSignalDesc * 1)(nccl_amd.WaitSignalDesc(1, 0, 0, 0))
    for count in (1, 0):
        assert lib.ncclPutSignal(None, count, 7, 0, None, 0, 0, 0, 0, None, None) == want
    assert lib.ncclSignal(0, 0, 0, 0, None, None) == want
    assert lib.ncclWaitSignal(1, desc, None, None) == want
    # ... and poisons a group like any refused call
    assert lib.ncclGroupStart() == 0
    assert lib.ncclSignal(0, 0, 0, 0, None, None) == want
    assert lib.ncclGroupEnd() == want


def test_argument_table(exe):
    """Every row of the argument table is ncclInvalidArgument and launches nothing; the calls at the very edge of the
    peer's registered size, a self put, a put of no elements, a signal and a wait launch exactly once each."""
    rows = {k: (int(v), int(row["launches"])) for row in _run(exe, "args") for k, v in row.items() if k != "launches"}
    assert set(rows) == set(REFUSED) | set(ACCEPTED) | {"put_nullcomm", "signal_nullcomm", "wait_nullcomm"}
    for call in REFUSED:
        assert rows[call] == (INVALID_ARGUMENT, 0), call
    for call in ("put_nullcomm", "signal_nullcomm", "wait_nullcomm"):
        assert rows[call][0] != 0 and rows[call][1] == 0, call
    for call in ACCEPTED:
        assert rows[call] == (0, 1), call


def test_batching(exe):
    """rma_plan_test batch: puts to three peers in one group are one launch; a wait splits batches and its duplicate
    descriptors add up; two puts to one peer stay in issue order on one workgroup set; count == 0 degenerates to a
    signal; a batch beyond chanCap or the argument block is split between peers with every stream whole, a stream of
    more than 96 messages in issue order; another stream closes a batch; a refused call launches nothing and leaves the
    communicator usable; ncclGroupSimulateEnd plans and drops."""
    out = _run(exe, "batch")[-1]
    assert int(out["checks"]) > 500


def test_plan_under_asan(built):
    """The same stand-alone driver built with ASan + UBSan (Makefile `build/asan/rma_plan_test`, host code only): both
    modes exit 0 without a sanitizer report."""
    subprocess.check_call(["make", "build/asan/rma_plan_test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "build", "asan", "rma_plan_test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "native", "lsan.supp"))
    for mode in ("args", "batch"):
        r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=180)
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        assert not any(s in out for s in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")), out[-4000:]


def test_rma_kernels_fit_two_workgroups_per_cu(built):
    """The rule tests/test_occupancy.py applies to the kernels it names: <= 128 VGPRs, >= 4 waves per SIMD, no VGPR
    spill, no scratch (from the build's report, build/kern_gather.usage)."""
    reps = {k: v for k, v in _reports().items() if "rmaPutKernel" in k or "rmaWaitKernel" in k}
    assert sum("rmaPutKernel" in k for k in reps) >= 2 and sum("rmaWaitKernel" in k for k in reps) >= 1, sorted(reps)
    for name, r in reps.items():
        occ, vgpr = int(r.get("Occupancy", 0)), int(r.get("VGPRs", 999))
        spill, scratch = int(r.get("VGPRs Spill", 0)), int(r.get("ScratchSize", 0))
        assert occ >= 4 and vgpr <= 128 and not spill and not scratch, \
            f"{r['file']}: {name}: VGPRs {vgpr} occupancy {occ} VGPR spills {spill} scratch {scratch}"
