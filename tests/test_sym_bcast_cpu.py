"""The zero-copy Broadcast without a GPU: the cut its kernel walks (tests/native/sym_bcast_plan_test, a stand-alone host
program built under ASan + UBSan that sweeps device_abi.h symBcastOwner / symBcastDirect / symBcastCut, the functions
the kernel and the host plan call) and the kernel's register budget from the build's report."""
import os
import subprocess

import pytest

from tests.test_occupancy import _reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cut_tiles_the_payload_for_every_root(built):
    """n = 2..8, every root, byte counts around 0, 16, the variant switch, block edges and channel-part edges: owner
    indices a bijection of the non-roots, blocks and parts tiling [0, bytes) exactly once, every part start a multiple
    of 16 within its block, the variant rule as stated (direct iff n == 2 or bytes < (n - 1) * minChannelBytes)."""
    subprocess.check_call(["make", "sym-bcast-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    env = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    out = subprocess.run([os.path.join(ROOT, "tests", "native", "sym_bcast_plan_test")], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.splitlines()[-1].startswith("OK ")
    last = dict(kv.split("=", 1) for kv in out.stdout.splitlines()[-1].split() if "=" in kv)
    assert int(last["cases"]) == 7 * 3 * 23 * 4 * 2     # n x minChannelBytes x byte counts x caps x minCTAs
    assert int(last["direct"]) > 0 and int(last["twophase"]) > 0
    assert int(last["empty"]) > 0                       # e.g. 1 byte at n = 8: trailing blocks only run the handshakes


def test_kernel_fits_two_workgroups_per_cu():
    """The rule tests/test_occupancy.py applies to the kernels it names: <= 128 VGPRs, >= 4 waves per SIMD, no VGPR
    spill, no scratch — every workgroup of every rank's launch must be co-resident. One instantiation, bytes."""
    if not _reports():
        pytest.skip("no build/*.usage reports: run `make` first")
    reps = {k: v for k, v in _reports().items() if "symBcastKernel" in k}
    assert len(reps) == 1, f"symBcastKernel instantiations in the reports: {sorted(reps)}"
    for name, r in reps.items():
        assert r["file"] == "kern_gather.usage", r["file"]
        occ, vgpr = int(r.get("Occupancy", 0)), int(r.get("VGPRs", 999))
        spill, scratch = int(r.get("VGPRs Spill", 0)), int(r.get("ScratchSize", 0))
        assert occ >= 4 and vgpr <= 128 and not spill and not scratch, \
            f"{r['file']}: {name}: VGPRs {vgpr} occupancy {occ} VGPR spills {spill} scratch {scratch}"
