"""The RDV (zero-copy rendezvous) planning of ncclSend / ncclRecv without a GPU (tests/native/p2p_zc_plan_test: p2p.cc
with the launches stubbed, device_abi.h's host-callable descriptor functions)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(built):
    subprocess.check_call(["make", "p2p-zc-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "native", "p2p_zc_plan_test")


@pytest.mark.parametrize("mode,want", [("desc", "OK cases=30"), ("kind", "OK cases=25"), ("cap", "OK launches=")])
def test_rdv_planning(exe, mode, want):
    """desc: the descriptor's round trip at the serial and offset extremes. kind: LL / staged / RDV at both thresholds,
    alike on both ends, and the receiver's descriptor for a recvbuff inside, outside and straddling a window. cap: a
    launch that holds an RDV message keeps within the smaller message cap, one descriptor per message."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    out = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and want in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
