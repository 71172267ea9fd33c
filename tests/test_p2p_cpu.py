"""ncclSend / ncclRecv / ncclAlltoAll / ncclGather / ncclScatter without a GPU: the exported symbols and their Python
bindings, the null-comm check, the host plan (tests/native/p2p_plan_test: p2p.cc with the launches stubbed) sliced
with the kernel's own host-callable functions, and the p2p kernels' register budget from the build's report."""
import ctypes
import os
import subprocess

import pytest

from tests.test_occupancy import _reports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"ncclSend": 6, "ncclRecv": 6, "ncclAlltoAll": 6, "ncclGather": 7, "ncclScatter": 7}
INVALID_ARGUMENT, INVALID_USAGE = 4, 5


@pytest.fixture(scope="module")
def exe(built):
    path = os.path.join(ROOT, "tests", "native", "p2p_plan_test")
    subprocess.check_call(["make", "p2p-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
    return path


def _run(exe, *args, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("NCCL_")}
    e.update({k: str(v) for k, v in env.items()})
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
    for method in ("send", "recv", "send_raw", "recv_raw", "alltoall", "alltoall_raw", "gather", "gather_raw", "scatter",
                   "scatter_raw"):
        assert callable(getattr(nccl_amd.Communicator, method)), method


def test_null_comm_rejected_like_allreduce(built):
    import nccl_amd
    lib = nccl_amd.load()
    want = lib.ncclAllReduce(None, None, 1, 7, 0, None, None)
    assert want != 0
    for count in (1, 0):   # before the count == 0 shortcut, as there
        assert lib.ncclSend(None, count, 7, 0, None, None) == want
        assert lib.ncclRecv(None, count, 7, 0, None, None) == want
        assert lib.ncclAlltoAll(None, None, count, 7, None, None) == want
        assert lib.ncclGather(None, None, count, 7, 0, None, None) == want
        assert lib.ncclScatter(None, None, count, 7, 0, None, None) == want


@pytest.mark.parametrize("env", [{}, {"NCCL_AMD_P2P_CHUNK_BYTES": 16, "NCCL_MIN_P2P_NCHANNELS": 4},
                                 {"NCCL_MAX_P2P_NCHANNELS": 1}, {"NCCL_AMD_P2P_CHUNK_BYTES": 4096, "NCCL_MAX_P2P_NCHANNELS": 64}],
                         ids=["default", "tiny-chunk", "one-channel", "small-chunk"])
def test_plan_symmetry_and_coverage(exe, env):
    """n in 2..16 x {0, 1, 15, 16, 17, slot-1, slot, slot+1, 16*maxch-1, 16*maxch+1, 300001, 1<<20|3} bytes x slots
    {4096, default} (p2p_plan_test cut): the sender, planning the message among arbitrary other ops, and the receiver,
    planning it alone, cut it into the same channel parts; the (channel, step) slices tile [0, bytes) exactly once,
    16-byte aligned, within a slot, with no empty channel below nch; an empty message is not planned at all."""
    out = _run(exe, "cut", **env)[-1]
    assert int(out["cases"]) == 15 * 2 * 12
    if "NCCL_MAX_P2P_NCHANNELS" in env and env["NCCL_MAX_P2P_NCHANNELS"] == 1:
        assert int(out["maxnch"]) == 1
    elif env:
        assert int(out["maxnch"]) > 9     # the small chunks spread over many channels
    else:
        assert int(out["maxnch"]) == 9    # 1 MiB + 3 in 128 KiB parts


def test_plan_packing(exe):
    """n in {2, 5, 8, 16} x grid budgets {2, 4, 16, 32, 512} x 25 random op sets (p2p_plan_test pack): every launch
    within the budget, rounds increasing across launches, every stream whole in one launch inside its launch's round
    range (so a round's send and recv are never split), every message once and in issue order; a budget of 1 refused."""
    out = _run(exe, "pack")[-1]
    assert int(out["cases"]) == 4 * 5 * 25
    assert int(out["split"]) > 0 and int(out["launches"]) > int(out["cases"]) // 2


def test_self_sends_need_their_recv(exe):
    out = _run(exe, "self")[-1]
    assert (out["matched"], out["copies"], out["launches"]) == ("0", "1", "0")     # a matched pair is a local copy
    assert int(out["sendonly"]) == INVALID_USAGE and int(out["recvonly"]) == INVALID_USAGE
    assert int(out["onerank"]) == 0 and int(out["onerankalone"]) == INVALID_USAGE  # one rank: the same path


def test_bad_peer_or_root_is_invalid_argument(exe):
    rows = {k: (int(v), int(row["launches"])) for row in _run(exe, "args") for k, v in row.items() if k != "launches"}
    for call in ("send_peer4", "recv_peer-1", "gather_root4", "scatter_root-1", "send_type13"):
        assert rows[call] == (INVALID_ARGUMENT, 0), call
    assert rows["send_nullcomm"][0] != 0 and rows["send_nullcomm"][1] == 0
    assert rows["send_empty"] == (0, 0)                      # count == 0: valid, nothing launched
    for call in ("send_ok", "alltoall_ok", "gather_ok", "scatter_ok"):
        assert rows[call] == (0, 1), call                    # an ungrouped call is a group of one: one launch


def test_p2p_kernels_fit_two_workgroups_per_cu():
    """The rule tests/test_occupancy.py applies to the kernels it names: <= 128 VGPRs, >= 4 waves per SIMD, no VGPR
    spill, no scratch — every workgroup of a p2p launch must be co-resident."""
    reps = {k: v for k, v in _reports().items() if "p2pKernel" in k}
    if not _reports():
        pytest.skip("no build/*.usage reports: run `make` first")
    assert len(reps) >= 2, f"p2pKernel instantiations in the reports: {sorted(reps)}"
    for name, r in reps.items():
        occ, vgpr = int(r.get("Occupancy", 0)), int(r.get("VGPRs", 999))
        spill, scratch = int(r.get("VGPRs Spill", 0)), int(r.get("ScratchSize", 0))
        assert occ >= 4 and vgpr <= 128 and not spill and not scratch, \
            f"{r['file']}: {name}: VGPRs {vgpr} occupancy {occ} VGPR spills {spill} scratch {scratch}"
