"""CPU tests of ncclCommSplit / ncclCommShrink below the GPU: tests/native/comm_split_test.cc — the
membership rules against the reference's insertion rule, the GPU occupancy a child inherits and the channel cap it
gives, the bootstrap's subset rounds over a real root thread (a rank that hangs up, a silent rank, a round naming a
departed rank, disagreeing masks) and the split / shrink rendezvous — built plain, under ASan+UBSan and under TSan
(host code only, stand-alone programs run directly); and the two calls' argument checks through the C ABI."""
import ctypes
import os
import subprocess

import pytest

import nccl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "WARNING: ThreadSanitizer")


def _run(target, *args, timeout_ms="20000"):
    r = subprocess.run(["make", "-s", target], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    e.update(NCCL_AMD_BOOTSTRAP_TIMEOUT_MS=timeout_ms, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
             LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "native", "lsan.supp"),
             TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, target), *args], env=e, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(s in out for s in REPORTS), out[-4000:]
    assert "failures=0" in out and "roots_left=0" in out, out[-4000:]
    return out


@pytest.mark.parametrize("target,mode", [("build/comm_split_test", "all"), ("build/asan/comm_split_test", "all"),
                                         ("build/tsan/comm_split_test", "bootstrap")])
def test_membership_occupancy_and_rounds(target, mode):
    """Mode "all": membership (the by-hand case, n = 1..16 against the reference's insertion rule, ties, negative keys,
    NOCOLOR, unsorted shrink lists), occupancy (8 ranks on one GPU, a child of 2 and its grandchild keep 8 and the cap
    32, not 128; 8 GPUs give 1) and the bootstrap rounds; "bootstrap": the threaded half alone, for TSan."""
    _run(target, mode)


@pytest.mark.parametrize("target", ["build/comm_split_test", "build/tsan/comm_split_test"])
def test_silent_rank_times_out(target):
    """A subset round naming a rank that is connected but never joins: the root fails it on the participants once
    NCCL_AMD_BOOTSTRAP_TIMEOUT_MS has passed (300 ms here: the limit running out is what is tested), and the next
    valid round works."""
    _run(target, "timeout", timeout_ms="300")


def test_argument_checks_without_gpu(built):
    """What can be checked without a communicator: a NULL or corrupted comm is refused with ncclInvalidArgument and
    nothing is written, inside a group the group fails with it; the constants and the export list. (The checks behind
    commCheck — a NULL newcomm, the shrink list, the config — need a live communicator:
    tests/test_gpu_comm_split.py::test_arguments.)"""
    lib = nccl_amd.load()
    P = ctypes.c_void_p
    child = P(0x1234)
    excl = (ctypes.c_int * 1)(0)
    assert lib.ncclCommSplit(None, 0, 0, ctypes.byref(child), None) == 4           # NULL comm
    assert lib.ncclCommShrink(None, excl, 1, ctypes.byref(child), None, 0) == 4
    assert child.value == 0x1234                                                  # nothing was written
    # a comm that fails the magic check is refused (here with a NULL newcomm too, which is never reached)
    fake = ctypes.create_string_buffer(1 << 16)
    assert lib.ncclCommSplit(fake, 0, 0, None, None) == 4
    assert lib.ncclCommShrink(fake, excl, 1, None, None, 0) == 4
    assert b"corrupted" in lib.ncclGetLastError(None)
    # a call that fails its checks inside a group fails the group (reference ncclGroupErrCheck); the next group is clean
    assert lib.ncclGroupStart() == 0
    assert lib.ncclCommSplit(None, 0, 0, ctypes.byref(child), None) == 4
    assert lib.ncclGroupEnd() == 4
    assert lib.ncclGroupStart() == 0 and lib.ncclGroupEnd() == 0
    assert (nccl_amd.SPLIT_NOCOLOR, nccl_amd.SHRINK_DEFAULT, nccl_amd.SHRINK_ABORT) == (-1, 0, 1)
    hdr = open(os.path.join(ROOT, "include", "nccl.h")).read()
    for line in ("#define NCCL_SPLIT_NOCOLOR -1", "#define NCCL_SHRINK_DEFAULT 0x00", "#define NCCL_SHRINK_ABORT 0x01"):
        assert line in hdr
    assert "ncclCommSplit" in nccl_amd.EXPORTED and "ncclCommShrink" in nccl_amd.EXPORTED
