"""CPU tests of the device API (include/nccl_device.h, nccl_amd/csrc/devcomm.cc): the five host entry points are
exported and bound and refuse bad arguments before touching a device, the public headers compile for their audiences
(nccl.h as C, nccl_device.h as host-only C++17), a relaxed barrier sync compiles to code without a fence, and the
header's pure functions — resource layout, teams, epoch compare — pass the stand-alone sweep tests/native/devapi_layout_test (built under ASan+UBSan)."""
import ctypes
import os
import re
import subprocess

import nccl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang"
NAMES = ["ncclCommQueryProperties", "ncclDevCommCreate", "ncclDevCommDestroy", "ncclGetLsaDevicePointer",
         "ncclGetPeerDevicePointer"]
INVALID_ARGUMENT = 4


def test_symbols_exported_and_bound(built):
    lib = nccl_amd.load()
    for n in NAMES:
        assert n in nccl_amd.EXPORTED
        assert hasattr(lib, n) and hasattr(lib, "p" + n), n
        assert getattr(lib, n).argtypes is not None, f"{n} has no ctypes signature"
    for meth in ("query_properties", "dev_comm_create", "dev_comm_destroy"):
        assert callable(getattr(nccl_amd.Communicator, meth))
    assert callable(nccl_amd.Window.lsa_pointer)


def test_bad_arguments_without_gpu(built):
    lib = nccl_amd.load()
    P = ctypes.c_void_p
    props = nccl_amd.CommProperties.default()
    reqs = nccl_amd.DevCommRequirements.default()
    dc = nccl_amd.DevCommStruct()
    out = P()
    # NULL communicator, whatever else is passed
    assert lib.ncclCommQueryProperties(None, ctypes.byref(props)) == INVALID_ARGUMENT
    assert lib.ncclCommQueryProperties(None, None) == INVALID_ARGUMENT
    assert lib.ncclDevCommCreate(None, ctypes.byref(reqs), ctypes.byref(dc)) == INVALID_ARGUMENT
    assert lib.ncclDevCommCreate(None, None, None) == INVALID_ARGUMENT
    assert lib.ncclDevCommDestroy(None, ctypes.byref(dc)) == INVALID_ARGUMENT
    assert lib.ncclDevCommDestroy(None, None) == INVALID_ARGUMENT
    # A caller struct with a bad magic or size is refused before the communicator is looked at, so these calls reach
    # that check even with a NULL communicator: the recorded message names the initializer, not the communicator.
    # (tests/test_gpu_device_api.py::test_properties_and_lifecycle repeats them on a live communicator.)
    def last():
        return lib.ncclGetLastError(None).decode()

    for field, value in (("magic", 0), ("size", 8)):
        bad = nccl_amd.CommProperties.default()
        setattr(bad, field, value)
        assert lib.ncclCommQueryProperties(None, ctypes.byref(bad)) == INVALID_ARGUMENT
        assert "NCCL_COMM_PROPERTIES_INITIALIZER" in last(), last()
        badq = nccl_amd.DevCommRequirements.default()
        setattr(badq, field, value)
        assert lib.ncclDevCommCreate(None, ctypes.byref(badq), ctypes.byref(dc)) == INVALID_ARGUMENT
        assert "NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER" in last(), last()
    assert lib.ncclDevCommDestroy(None, ctypes.byref(nccl_amd.DevCommStruct())) == INVALID_ARGUMENT   # magic 0
    assert "not made by ncclDevCommCreate" in last(), last()
    # well-formed structs with a NULL communicator: now it is the communicator that is refused
    assert lib.ncclCommQueryProperties(None, ctypes.byref(props)) == INVALID_ARGUMENT
    assert "comm argument is NULL" in last(), last()
    assert lib.ncclDevCommCreate(None, ctypes.byref(reqs), ctypes.byref(dc)) == INVALID_ARGUMENT
    assert "comm argument is NULL" in last(), last()
    made = nccl_amd.DevCommStruct()
    made.magic = 0xCAFEBEEF
    assert lib.ncclDevCommDestroy(None, ctypes.byref(made)) == INVALID_ARGUMENT
    assert "comm argument is NULL" in last(), last()
    # the pointer getters: NULL window, NULL result
    assert lib.ncclGetLsaDevicePointer(None, 0, 0, ctypes.byref(out)) == INVALID_ARGUMENT
    assert lib.ncclGetPeerDevicePointer(None, 0, 0, ctypes.byref(out)) == INVALID_ARGUMENT
    assert lib.ncclGetLsaDevicePointer(None, 0, 0, None) == INVALID_ARGUMENT
    assert lib.ncclGetPeerDevicePointer(None, 0, 0, None) == INVALID_ARGUMENT
    assert lib.ncclGetLastError(None) != b""


def test_pointer_getters_bound_offset_and_rank():
    """The getters read the window's table only (no device): a hand-made table of 3 ranks with different sizes."""
    lib = nccl_amd.load()

    class Win(ctypes.Structure):  # the device-read head of ncclWindow_vidmem (include/nccl_device.h)
        _fields_ = [("peerPtr", ctypes.c_uint64 * 16), ("peerSize", ctypes.c_size_t * 16), ("nRanks", ctypes.c_int),
                    ("rank", ctypes.c_int), ("host", ctypes.c_uint64 * 24)]

    w = Win()
    w.nRanks, w.rank = 3, 1
    for r in range(3):
        w.peerPtr[r] = 0x100000 * (r + 1)
        w.peerSize[r] = 1000 + 100 * r
    out = ctypes.c_void_p()
    for fn in (lib.ncclGetLsaDevicePointer, lib.ncclGetPeerDevicePointer):
        for r in range(3):
            for off in (0, 16, 1000 + 100 * r - 1):
                assert fn(ctypes.addressof(w), off, r, ctypes.byref(out)) == 0
                assert out.value == 0x100000 * (r + 1) + off
            assert fn(ctypes.addressof(w), 1000 + 100 * r, r, ctypes.byref(out)) == INVALID_ARGUMENT
        assert fn(ctypes.addressof(w), 0, 3, ctypes.byref(out)) == INVALID_ARGUMENT
        assert fn(ctypes.addressof(w), 0, -1, ctypes.byref(out)) == INVALID_ARGUMENT


def test_headers_compile_for_their_audiences(tmp_path):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    c = tmp_path / "only_c.c"
    c.write_text('#include "nccl.h"\n'
                 "ncclResult_t f(ncclComm_t c, ncclDevComm_t* d, const ncclDevCommRequirements_t* q) {\n"
                 "  return ncclDevCommCreate(c, q, d);\n}\n")
    r = subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", *inc, str(c)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    cpp = tmp_path / "host_only.cc"
    cpp.write_text('#include "nccl_device.h"\n'
                   "ncclDevCommRequirements_t q = NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER;\n"
                   "ncclCommProperties_t p = NCCL_COMM_PROPERTIES_INITIALIZER;\n"
                   "int f(const ncclDevComm& dc) { return ncclTeamRankToWorld(dc, ncclTeamLsa(dc), 0) + (int)sizeof(q); }\n"
                   "static_assert(sizeof(ncclTeam) == 12, \"\");\n")
    r = subprocess.run([CLANG + "++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", *inc, str(cpp)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_relaxed_barrier_emits_no_fence(tmp_path):
    """The gfx950 code of one sync: acq_rel has the L2 write-back and the cache invalidate, relaxed has neither."""
    src = tmp_path / "one_sync.hip"
    src.write_text('#include "nccl_device.h"\n'
                   "template <int ORDER> __global__ void oneSync(ncclDevComm dc) {\n"
                   "  ncclCoopCta cta;\n"
                   "  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);\n"
                   "  bar.sync(cta, (std::memory_order)ORDER);\n}\n"
                   "template __global__ void oneSync<(int)std::memory_order_relaxed>(ncclDevComm);\n"
                   "template __global__ void oneSync<(int)std::memory_order_acq_rel>(ncclDevComm);\n")
    out = tmp_path / "one_sync.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-I" + os.path.join(ROOT, "include"), "-o", str(out), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    bodies = {}
    for m in re.finditer(r"^(_Z7oneSyncILi(\d+)E\w*):\s.*?s_endpgm", out.read_text(), re.M | re.S):
        bodies[int(m.group(2))] = m.group(0)
    relaxed, acq_rel = bodies[0], bodies[4]     # std::memory_order_relaxed = 0, acq_rel = 4
    assert "buffer_wbl2" in acq_rel and "buffer_inv" in acq_rel
    assert "buffer_wbl2" not in relaxed and "buffer_inv" not in relaxed
    assert "s_waitcnt vmcnt(0)" in relaxed       # the drain before the inbox stores stays


def test_layout_teams_and_epochs(built):
    """tests/native/devapi_layout_test: the resource layout for n in 1..8, barrier counts {0, 1, 7, 64, cap} and buffer
    lists including (1, 1), (1000, 256), (65536, 4096); every team function against brute-force rank sets for every
    (nRanks <= 8, innerSize | nRanks); the epoch compare at 0, 2^31-1, 2^32-2, 2^32-1. Its printed struct sizes are
    what the ctypes mirrors must have."""
    subprocess.check_call(["make", "-s", "devapi-layout-test"], cwd=ROOT)
    r = subprocess.run([os.path.join(ROOT, "tests", "native", "devapi_layout_test")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    sizes = dict((k, int(v)) for k, v in re.findall(r"(ncclDev\w+|ncclComm\w+)=(\d+)", r.stdout))
    assert sizes == {
        "ncclDevComm": ctypes.sizeof(nccl_amd.DevCommStruct),
        "ncclDevCommRequirements": ctypes.sizeof(nccl_amd.DevCommRequirements),
        "ncclCommProperties": ctypes.sizeof(nccl_amd.CommProperties),
        "ncclDevResourceRequirements": ctypes.sizeof(nccl_amd.DevResourceRequirements),
    }


def test_python_layout_constants_match_header():
    src = open(os.path.join(ROOT, "include", "nccl_device.h")).read()
    for name, val in (("NCCL_DEVICE_MAX_RANKS", nccl_amd.DEV_MAX_RANKS),
                      ("NCCL_DEVICE_MAX_LSA_BARRIERS", nccl_amd.DEV_MAX_LSA_BARRIERS),
                      ("NCCL_DEVICE_RESOURCE_GRANULE", nccl_amd.DEV_RESOURCE_GRANULE)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == val
