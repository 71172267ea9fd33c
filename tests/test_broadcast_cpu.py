"""ncclBroadcast / ncclBcast without a GPU: the exported symbols and their Python bindings, the null-comm check, the
`broadcast:` rows of NCCL_ALGO / NCCL_PROTO, the host plan (tests/native/bcast_plan_test, enqueue.cc with the launches
stubbed) and the partition its kernels walk, sliced with the kernels' own host-callable functions."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(built):
    path = os.path.join(ROOT, "tests", "native", "bcast_plan_test")
    subprocess.check_call(["make", "bcast-plan-test"], cwd=ROOT, stdout=subprocess.DEVNULL)
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
    for name in ("ncclBroadcast", "pncclBroadcast", "ncclBcast", "pncclBcast"):
        assert hasattr(lib, name), name
    assert {"ncclBroadcast", "ncclBcast"} <= set(nccl_amd.EXPORTED)
    bound = nccl_amd.load()
    assert bound.ncclBroadcast.argtypes is not None and len(bound.ncclBroadcast.argtypes) == 7
    assert bound.ncclBcast.argtypes is not None and len(bound.ncclBcast.argtypes) == 6
    for method in ("broadcast", "bcast", "broadcast_raw"):
        assert callable(getattr(nccl_amd.Communicator, method))


def test_null_comm_rejected_like_allreduce(built):
    import nccl_amd
    lib = nccl_amd.load()
    want = lib.ncclAllReduce(None, None, 1, 7, 0, None, None)
    assert want != 0
    assert lib.ncclBroadcast(None, None, 1, 7, 0, None, None) == want
    assert lib.ncclBcast(None, 1, 7, 0, None, None) == want
    assert lib.ncclBroadcast(None, None, 0, 7, 0, None, None) == want   # before the count == 0 shortcut, as there


def test_env_rows_parse(exe):
    m = _run(exe, "matrix", NCCL_ALGO="broadcast:ring", NCCL_PROTO="broadcast:ll")
    assert m[0] == {"parse": "0"}
    assert m[1]["func"] == "broadcast" and m[1]["algo"] == "ring" and m[1]["noalgo"] == "0"
    assert (m[1]["ll"], m[1]["ll128"], m[1]["simple"]) == ("1", "0", "0")
    # untouched rows keep their defaults: a plain run
    m = _run(exe, "matrix")
    assert m[1]["algo"] == "none" and m[1]["noalgo"] == "0" and (m[1]["ll"], m[1]["simple"]) == ("1", "1")
    # an unknown name under the prefix fails the parse (ncclInvalidUsage), as for every collective
    assert _run(exe, "matrix", NCCL_ALGO="broadcast:bogus")[0] == {"parse": "5"}


def test_no_algorithm_is_invalid_usage(exe):
    m = _run(exe, "matrix", NCCL_ALGO="broadcast:nvls")
    assert m[0] == {"parse": "0"} and m[1]["noalgo"] == "1"
    assert _run(exe, "plan", "4", "1000", NCCL_ALGO="broadcast:nvls")[0] == {"result": "5", "launches": "0"}
    assert _run(exe, "plan", "4", "1000", NCCL_PROTO="broadcast:^LL,LL128,Simple")[0]["result"] == "5"
    # the other collectives' rows do not reach Broadcast
    assert _run(exe, "plan", "4", "1000", NCCL_ALGO="allreduce:nvls")[0] == {"result": "0", "launches": "1"}


def test_plan_choices(exe):
    """LL where llPlan admits the payload, direct otherwise; one rank copies (or does nothing in place); a bad root
    and count == 0 launch nothing; forced algorithms land on the direct plan."""
    assert _run(exe, "plan", "4", "1000", "3")[1] == {"algo": "ll", "nch": "1", "part": "125", "root": "3"}
    big = _run(exe, "plan", "4", "10000000", "2")[1]
    assert big["algo"] == "direct" and big["root"] == "2" and int(big["chunk"]) == 2_500_000
    assert _run(exe, "plan", "4", "70001", NCCL_AMD_LL128=1, NCCL_AMD_LL_BYTES=1024)[1]["algo"] == "ll128"
    assert _run(exe, "plan", "1", "1000")[1]["algo"] == "copy"
    assert _run(exe, "plan", "4", "1000", "4")[0] == {"result": "4", "launches": "0"}    # ncclInvalidArgument
    assert _run(exe, "plan", "4", "1000", "-1")[0] == {"result": "4", "launches": "0"}
    assert _run(exe, "plan", "4", "0")[0] == {"result": "0", "launches": "0"}
    for algo in ("RING", "DIRECT", "TREE", "ONESHOT"):
        assert _run(exe, "plan", "4", "1000", NCCL_ALGO=algo)[1]["algo"] == "direct", algo
    assert _run(exe, "plan", "4", "1000", NCCL_ALGO="broadcast:ring", NCCL_PROTO="broadcast:ll")[1]["algo"] == "ll"


def test_partition_coverage(exe):
    """n in 2..8 x {1, 15, 16, 17, 16n-1, 16n, 16n+1, 4099, 300001, 1<<20|3} bytes x slots {4096, default} under
    NCCL_PROTO unset / Simple / LL / LL128 (bcast_plan_test sweep): direct slices tile [0, bytes) exactly once, an
    empty block moves nothing, LL / LL64 parts tile the payload units with no empty channel."""
    out = _run(exe, "sweep")[-1]
    assert int(out["cases"]) == 4 * 7 * 10 * 2
    assert int(out["direct"]) > 0 and int(out["ll"]) > 0 and int(out["ll128"]) > 0
