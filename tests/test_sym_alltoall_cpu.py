"""The zero-copy AlltoAll / Gather without a GPU: the channel cut its kernel walks (tests/native/sym_a2a_plan_test, a
stand-alone host program built under ASan + UBSan that sweeps device_abi.h symA2ACut / symA2APart, the functions the
kernel and the host plan call) and the kernel's register budget from the build's report."""
import os
import subprocess

import pytest

from tests.test_occupancy import _reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cut_covers_every_block_alike(built):
    """B in {1, 15, 16, 17, 8202, 16384, 16385, 280004, 64 MiB} x caps {1, 3, 32, 256} x minCTAs {1, 2} x
    minChannelBytes {16, 4096, 16384}: parts disjoint, in order, covering [0, B) exactly, every part start a multiple
    of 16, nch within its bounds, the same cut on every rank."""
    subprocess.check_call(["make", "sym-a2a-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    env = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    out = subprocess.run([os.path.join(ROOT, "tests", "native", "sym_a2a_plan_test")], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    last = dict(kv.split("=", 1) for kv in out.stdout.splitlines()[-1].split() if "=" in kv)
    assert out.stdout.splitlines()[-1].startswith("OK ")
    assert int(last["cases"]) == 9 * 4 * 2 * 3
    assert int(last["maxnch"]) == 256       # 64 MiB at the largest cap
    assert int(last["empty"]) > 0           # e.g. 1 byte with minCTAs 2: a channel that only runs the handshake


def test_kernel_fits_two_workgroups_per_cu():
    """The rule tests/test_occupancy.py applies to the kernels it names: <= 128 VGPRs, >= 4 waves per SIMD, no VGPR
    spill, no scratch — every workgroup of every rank's launch must be co-resident. One instantiation, bytes."""
    if not _reports():
        pytest.skip("no build/*.usage reports: run `make` first")
    reps = {k: v for k, v in _reports().items() if "symA2AKernel" in k}
    assert len(reps) == 1, f"symA2AKernel instantiations in the reports: {sorted(reps)}"
    for name, r in reps.items():
        assert r["file"] == "kern_gather.usage", r["file"]
        occ, vgpr = int(r.get("Occupancy", 0)), int(r.get("VGPRs", 999))
        spill, scratch = int(r.get("VGPRs Spill", 0)), int(r.get("ScratchSize", 0))
        assert occ >= 4 and vgpr <= 128 and not spill and not scratch, \
            f"{r['file']}: {name}: VGPRs {vgpr} occupancy {occ} VGPR spills {spill} scratch {scratch}"
