"""nccl_amd — Python host mirror of the MI355X tensor-bucket reduction engine.

The product is the C-ABI shared library ``nccl_amd/lib/libnccl.so`` (declared in ``include/nccl.h``,
built from ``nccl_amd/csrc``). This module binds it with ctypes and mirrors the reference's own Python
interface, nccl4py (``/root/reference/bindings/nccl4py/nccl/core/communicator.py``): ``get_unique_id``,
``Communicator.init`` / ``Communicator.init_all``, ``allreduce`` / ``reduce_scatter`` / ``allgather`` /
``reduce``, ``group()`` and ``create_pre_mul_sum``. Buffers are torch tensors on the communicator's
device (nccl4py takes CuPy/DLPack buffers); streams are HIP streams (torch.cuda streams on ROCm).

There is no fallback: if the HIP library is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import enum
import os
from typing import Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnccl.so")

_lib = None


class NcclError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = _lib.ncclGetErrorString(code).decode() if _lib is not None else str(code)
        last = _lib.ncclGetLastError(None).decode() if _lib is not None else ""
        super().__init__(f"{where} failed: {msg} ({code}){': ' + last if last else ''}")


class Result(enum.IntEnum):  # nccl.h.in:44-53
    Success = 0
    UnhandledCudaError = 1
    SystemError = 2
    InternalError = 3
    InvalidArgument = 4
    InvalidUsage = 5
    RemoteError = 6
    InProgress = 7
    Timeout = 8


class RedOp(enum.IntEnum):  # nccl.h.in:364-372
    SUM = 0
    PROD = 1
    MAX = 2
    MIN = 3
    AVG = 4


class DataType(enum.IntEnum):  # nccl.h.in:382-395
    INT8 = 0
    UINT8 = 1
    INT32 = 2
    UINT32 = 3
    INT64 = 4
    UINT64 = 5
    FLOAT16 = 6
    FLOAT32 = 7
    FLOAT64 = 8
    BFLOAT16 = 9
    FLOAT8E4M3 = 10
    FLOAT8E5M2 = 11


SUM, PROD, MAX, MIN, AVG = RedOp.SUM, RedOp.PROD, RedOp.MAX, RedOp.MIN, RedOp.AVG
TYPE_SIZE = {0: 1, 1: 1, 2: 4, 3: 4, 4: 8, 5: 8, 6: 2, 7: 4, 8: 8, 9: 2, 10: 1, 11: 1}


class UniqueId(ctypes.Structure):
    _fields_ = [("internal", ctypes.c_char * 128)]


class SimInfo(ctypes.Structure):  # ncclSimInfo_t, nccl.h.in:136-152
    _fields_ = [("size", ctypes.c_size_t), ("magic", ctypes.c_uint), ("version", ctypes.c_uint),
                ("estimatedTime", ctypes.c_float)]

    @classmethod
    def default(cls) -> "SimInfo":
        s = cls()
        s.size = ctypes.sizeof(cls)
        s.magic = 0x74685283
        s.version = get_version_code_static()
        s.estimatedTime = -1.0
        return s


@dataclasses.dataclass(frozen=True)
class GroupSimInfo:
    """nccl4py GroupSimInfo (bindings/nccl4py/nccl/core/group.py:28-36)."""
    estimated_time: float  # seconds


class WaitSignalDesc(ctypes.Structure):  # ncclWaitSignalDesc_t, nccl.h.in:668-673
    _fields_ = [("opCnt", ctypes.c_int), ("peer", ctypes.c_int), ("sigIdx", ctypes.c_int), ("ctx", ctypes.c_int)]


class MemStat(enum.IntEnum):  # ncclCommMemStat_t, nccl.h.in:333-338
    GPU_MEM_SUSPEND = 0
    GPU_MEM_SUSPENDED = 1
    GPU_MEM_PERSIST = 2
    GPU_MEM_TOTAL = 3


class Config(ctypes.Structure):  # ncclConfig_t, nccl.h.in:84-108
    _fields_ = [
        ("size", ctypes.c_size_t), ("magic", ctypes.c_uint), ("version", ctypes.c_uint),
        ("blocking", ctypes.c_int), ("cgaClusterSize", ctypes.c_int), ("minCTAs", ctypes.c_int),
        ("maxCTAs", ctypes.c_int), ("netName", ctypes.c_char_p), ("splitShare", ctypes.c_int),
        ("trafficClass", ctypes.c_int), ("commName", ctypes.c_char_p), ("collnetEnable", ctypes.c_int),
        ("CTAPolicy", ctypes.c_int), ("shrinkShare", ctypes.c_int), ("nvlsCTAs", ctypes.c_int),
        ("nChannelsPerNetPeer", ctypes.c_int), ("nvlinkCentricSched", ctypes.c_int),
        ("graphUsageMode", ctypes.c_int), ("numRmaCtx", ctypes.c_int), ("maxP2pPeers", ctypes.c_int),
        ("graphStreamOrdering", ctypes.c_int),
    ]

    @classmethod
    def default(cls, **kw) -> "Config":
        undef = -(2 ** 31)
        c = cls()
        c.size = ctypes.sizeof(cls)
        c.magic = 0xCAFEBEEF
        c.version = get_version_code_static()
        for name, ty in cls._fields_[3:]:
            setattr(c, name, None if ty is ctypes.c_char_p else undef)
        for k, v in kw.items():
            setattr(c, k, v.encode() if isinstance(v, str) else v)
        return c


class DevResourceRequirements(ctypes.Structure):  # ncclDevResourceRequirements, include/nccl_device.h
    pass


DevResourceRequirements._fields_ = [
    ("next", ctypes.POINTER(DevResourceRequirements)), ("bufferSize", ctypes.c_size_t), ("bufferAlign", ctypes.c_size_t),
    ("outBufferHandle", ctypes.POINTER(ctypes.c_uint32)), ("ginSignalCount", ctypes.c_int),
    ("ginCounterCount", ctypes.c_int), ("outGinSignalStart", ctypes.c_void_p), ("outGinCounterStart", ctypes.c_void_p),
]


class DevCommRequirements(ctypes.Structure):  # ncclDevCommRequirements, include/nccl_device.h
    _fields_ = [
        ("size", ctypes.c_size_t), ("magic", ctypes.c_uint), ("version", ctypes.c_uint),
        ("resourceRequirementsList", ctypes.POINTER(DevResourceRequirements)), ("teamRequirementsList", ctypes.c_void_p),
        ("lsaMultimem", ctypes.c_bool), ("barrierCount", ctypes.c_int), ("lsaBarrierCount", ctypes.c_int),
        ("railGinBarrierCount", ctypes.c_int), ("lsaLLA2ABlockCount", ctypes.c_int), ("lsaLLA2ASlotCount", ctypes.c_int),
        ("ginForceEnable", ctypes.c_bool), ("ginContextCount", ctypes.c_int), ("ginSignalCount", ctypes.c_int),
        ("ginCounterCount", ctypes.c_int), ("ginConnectionType", ctypes.c_int), ("ginExclusiveContexts", ctypes.c_bool),
        ("ginQueueDepth", ctypes.c_int), ("ginTrafficClass", ctypes.c_int), ("worldGinBarrierCount", ctypes.c_int),
        ("ginStrongSignalsRequired", ctypes.c_bool), ("ginVaSignalsRequired", ctypes.c_bool),
    ]

    @classmethod
    def default(cls, **kw) -> "DevCommRequirements":
        """NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER, then the given fields."""
        q = cls()
        q.size = ctypes.sizeof(cls)
        q.magic = 0xCAFEBEEF
        q.version = get_version_code_static()
        q.ginContextCount = 4
        q.ginTrafficClass = -(2 ** 31)
        q.ginStrongSignalsRequired = q.ginVaSignalsRequired = True
        for k, v in kw.items():
            setattr(q, k, v)
        return q


class CommProperties(ctypes.Structure):  # ncclCommProperties, include/nccl_device.h
    _fields_ = [
        ("size", ctypes.c_size_t), ("magic", ctypes.c_uint), ("version", ctypes.c_uint),
        ("rank", ctypes.c_int), ("nRanks", ctypes.c_int), ("cudaDev", ctypes.c_int), ("nvmlDev", ctypes.c_int),
        ("deviceApiSupport", ctypes.c_bool), ("multimemSupport", ctypes.c_bool), ("ginType", ctypes.c_int),
        ("nLsaTeams", ctypes.c_int), ("hostRmaSupport", ctypes.c_bool), ("railedGinType", ctypes.c_int),
    ]

    @classmethod
    def default(cls) -> "CommProperties":
        p = cls()
        p.size = ctypes.sizeof(cls)
        p.magic = 0xCAFEBEEF
        p.version = get_version_code_static()
        return p


DEV_MAX_RANKS = 16              # NCCL_DEVICE_MAX_RANKS
DEV_MAX_LSA_BARRIERS = 4096     # NCCL_DEVICE_MAX_LSA_BARRIERS
DEV_RESOURCE_GRANULE = 128      # NCCL_DEVICE_RESOURCE_GRANULE


class DevCommStruct(ctypes.Structure):
    """ncclDevComm (include/nccl_device.h), handed to kernels by value. Opaque to Python callers except for the
    fields a test or a launcher may want to read."""
    _fields_ = [
        ("magic", ctypes.c_uint), ("version", ctypes.c_uint), ("rank", ctypes.c_int), ("nRanks", ctypes.c_int),
        ("lsaRank", ctypes.c_int), ("lsaSize", ctypes.c_int), ("resourceWindow", ctypes.c_void_p),
        ("resourcePeerPtr", ctypes.c_void_p * DEV_MAX_RANKS), ("lsaBarrierBufHandle", ctypes.c_uint32),
        ("lsaBarrierCount", ctypes.c_int), ("abortFlag", ctypes.c_void_p), ("errorWord", ctypes.c_void_p),
        ("timeoutTicks", ctypes.c_uint64), ("hostState", ctypes.c_void_p),
    ]


class DevComm:
    """What Communicator.dev_comm_create returns: the ncclDevComm struct (`struct`, pass ctypes.byref(d.struct) or
    d.ptr to a launcher taking `const ncclDevComm*`) and the resource-buffer handles in the order asked."""

    def __init__(self, comm: "Communicator", lsa_barriers: int, buffers):
        self.comm = comm
        self.struct = DevCommStruct()
        self.lsa_barriers = lsa_barriers
        self._handles = (ctypes.c_uint32 * max(1, len(buffers)))()
        self._nbuf = len(buffers)
        self._reqs = (DevResourceRequirements * max(1, len(buffers)))()
        for k, (size, align) in enumerate(buffers):
            r = self._reqs[k]
            r.bufferSize, r.bufferAlign = size, align
            r.outBufferHandle = ctypes.cast(ctypes.byref(self._handles, 4 * k), ctypes.POINTER(ctypes.c_uint32))
            if k + 1 < len(buffers):
                r.next = ctypes.pointer(self._reqs[k + 1])

    @property
    def ptr(self) -> int:
        return ctypes.addressof(self.struct)

    @property
    def buffer_handles(self) -> list:
        """ncclDevResourceHandle of every buffer (valid once the creation ran: after the group, inside one)."""
        return [int(self._handles[k]) for k in range(self._nbuf)]

    @property
    def resource_window(self) -> int:
        return self.struct.resourceWindow or 0


def get_version_code_static() -> int:
    return 2 * 10000 + 30 * 100 + 7  # NCCL_VERSION(2,30,7)


# Every function include/nccl.h declares (the C-ABI surface the tests check for).
EXPORTED = [
    "ncclMemAlloc", "ncclMemFree", "ncclGetVersion", "ncclGetUniqueId", "ncclCommInitRankConfig",
    "ncclCommInitRank", "ncclCommInitAll", "ncclCommFinalize", "ncclCommDestroy", "ncclCommAbort",
    "ncclGetErrorString", "ncclGetLastError", "ncclCommGetAsyncError", "ncclCommCount", "ncclCommCuDevice",
    "ncclCommUserRank", "ncclRedOpCreatePreMulSum", "ncclRedOpDestroy", "ncclReduce", "ncclAllReduce",
    "ncclReduceScatter", "ncclAllGather", "ncclGroupStart", "ncclGroupEnd",
    "ncclCommRegister", "ncclCommDeregister", "ncclCommWindowRegister", "ncclCommWindowDeregister",
    "ncclWinGetUserPtr", "ncclCommInitRankScalable", "ncclCommMemStats", "ncclGroupSimulateEnd",
    "ncclBroadcast", "ncclBcast", "ncclSend", "ncclRecv", "ncclAlltoAll", "ncclGather", "ncclScatter",
    "ncclPutSignal", "ncclSignal", "ncclWaitSignal", "ncclCommSplit", "ncclCommShrink",
    "ncclCommQueryProperties", "ncclDevCommCreate", "ncclDevCommDestroy", "ncclGetLsaDevicePointer",
    "ncclGetPeerDevicePointer",
]


SPLIT_NOCOLOR = -1          # nccl.h.in:57
SHRINK_DEFAULT = 0x00       # nccl.h.in:76-77
SHRINK_ABORT = 0x01
WIN_DEFAULT = 0x00          # nccl.h.in:64-68
WIN_COLL_SYMMETRIC = 0x01
WIN_STRICT_ORDERING = 0x02
WIN_REQUIRED_ALIGNMENT = 4096


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libnccl.so (RTLD_LOCAL; the library is linked -Bsymbolic so RCCL, which torch loads, can
    never interpose on its internal calls)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch ships its own libamdhip64 (same soname as /opt/rocm's). If this
    # library were loaded first it would pull in /opt/rocm's runtime and torch would later bring a second
    # one ("no ROCm-capable device" from whichever initialises second), so let torch load its runtime first
    # and bind to that one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    p = path or os.environ.get("NCCL_AMD_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise RuntimeError(f"nccl_amd: HIP library {p} is missing — build it first (make, or __graft_entry__.build())")
    lib = ctypes.CDLL(p, mode=ctypes.RTLD_LOCAL)
    R, P, I, S, U64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64
    sig = {
        "ncclGetVersion": (R, [ctypes.POINTER(I)]),
        "ncclGetUniqueId": (R, [ctypes.POINTER(UniqueId)]),
        "ncclCommInitRank": (R, [ctypes.POINTER(P), I, UniqueId, I]),
        "ncclCommInitRankConfig": (R, [ctypes.POINTER(P), I, UniqueId, I, ctypes.POINTER(Config)]),
        "ncclCommInitAll": (R, [ctypes.POINTER(P), I, ctypes.POINTER(I)]),
        "ncclCommFinalize": (R, [P]),
        "ncclCommDestroy": (R, [P]),
        "ncclCommAbort": (R, [P]),
        "ncclGetErrorString": (ctypes.c_char_p, [I]),
        "ncclGetLastError": (ctypes.c_char_p, [P]),
        "ncclCommGetAsyncError": (R, [P, ctypes.POINTER(I)]),
        "ncclCommCount": (R, [P, ctypes.POINTER(I)]),
        "ncclCommCuDevice": (R, [P, ctypes.POINTER(I)]),
        "ncclCommUserRank": (R, [P, ctypes.POINTER(I)]),
        "ncclRedOpCreatePreMulSum": (R, [ctypes.POINTER(I), P, I, I, P]),
        "ncclRedOpDestroy": (R, [I, P]),
        "ncclAllReduce": (R, [P, P, S, I, I, P, P]),
        "ncclReduceScatter": (R, [P, P, S, I, I, P, P]),
        "ncclAllGather": (R, [P, P, S, I, P, P]),
        "ncclReduce": (R, [P, P, S, I, I, I, P, P]),
        "ncclBroadcast": (R, [P, P, S, I, I, P, P]),
        "ncclBcast": (R, [P, S, I, I, P, P]),
        "ncclSend": (R, [P, S, I, I, P, P]),
        "ncclRecv": (R, [P, S, I, I, P, P]),
        "ncclAlltoAll": (R, [P, P, S, I, P, P]),
        "ncclGather": (R, [P, P, S, I, I, P, P]),
        "ncclScatter": (R, [P, P, S, I, I, P, P]),
        "ncclPutSignal": (R, [P, S, I, I, P, S, I, I, ctypes.c_uint, P, P]),
        "ncclSignal": (R, [I, I, I, ctypes.c_uint, P, P]),
        "ncclWaitSignal": (R, [I, ctypes.POINTER(WaitSignalDesc), P, P]),
        "ncclGroupStart": (R, []),
        "ncclGroupEnd": (R, []),
        "ncclMemAlloc": (R, [ctypes.POINTER(P), S]),
        "ncclCommRegister": (R, [P, P, S, ctypes.POINTER(P)]),
        "ncclCommDeregister": (R, [P, P]),
        "ncclCommWindowRegister": (R, [P, P, S, ctypes.POINTER(P), I]),
        "ncclCommWindowDeregister": (R, [P, P]),
        "ncclWinGetUserPtr": (R, [P, P, ctypes.POINTER(P)]),
        "ncclMemFree": (R, [P]),
        "ncclCommInitRankScalable": (R, [ctypes.POINTER(P), I, I, I, ctypes.POINTER(UniqueId), ctypes.POINTER(Config)]),
        "ncclCommMemStats": (R, [P, I, ctypes.POINTER(U64)]),
        "ncclGroupSimulateEnd": (R, [ctypes.POINTER(SimInfo)]),
        "ncclCommSplit": (R, [P, I, I, ctypes.POINTER(P), ctypes.POINTER(Config)]),
        "ncclCommShrink": (R, [P, ctypes.POINTER(I), I, ctypes.POINTER(P), ctypes.POINTER(Config), I]),
        "ncclCommQueryProperties": (R, [P, ctypes.POINTER(CommProperties)]),
        "ncclDevCommCreate": (R, [P, ctypes.POINTER(DevCommRequirements), ctypes.POINTER(DevCommStruct)]),
        "ncclDevCommDestroy": (R, [P, ctypes.POINTER(DevCommStruct)]),
        "ncclGetLsaDevicePointer": (R, [P, S, I, ctypes.POINTER(P)]),
        "ncclGetPeerDevicePointer": (R, [P, S, I, ctypes.POINTER(P)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


def _check(code: int, where: str) -> None:
    if code != 0:
        raise NcclError(code, where)


def get_version() -> int:
    v = ctypes.c_int()
    _check(load().ncclGetVersion(ctypes.byref(v)), "ncclGetVersion")
    return v.value


def get_unique_id() -> bytes:
    uid = UniqueId()
    _check(load().ncclGetUniqueId(ctypes.byref(uid)), "ncclGetUniqueId")
    return ctypes.string_at(ctypes.addressof(uid), 128)


def _uid(b: bytes) -> UniqueId:
    u = UniqueId()
    ctypes.memmove(ctypes.byref(u), b, 128)
    return u


def group_start() -> None:
    _check(load().ncclGroupStart(), "ncclGroupStart")


def group_end(*, simulate: bool = False) -> Optional[GroupSimInfo]:
    """nccl4py group_end (group.py:54-76): simulate=True plans the group's collectives without launching
    them (ncclGroupSimulateEnd) and returns the cost model's estimate, in seconds."""
    if not simulate:
        _check(load().ncclGroupEnd(), "ncclGroupEnd")
        return None
    si = SimInfo.default()
    _check(load().ncclGroupSimulateEnd(ctypes.byref(si)), "ncclGroupSimulateEnd")
    return GroupSimInfo(estimated_time=si.estimatedTime * 1e-6)


@contextlib.contextmanager
def group():
    group_start()
    try:
        yield
    finally:
        group_end()


def torch_dtype_to_nccl(dtype) -> int:
    import torch
    m = {
        torch.int8: 0, torch.uint8: 1, torch.int32: 2, torch.int64: 4, torch.float16: 6, torch.float32: 7,
        torch.float64: 8, torch.bfloat16: 9,
    }
    for name, code in (("uint32", 3), ("uint64", 5), ("float8_e4m3fn", 10), ("float8_e5m2", 11)):
        if hasattr(torch, name):
            m[getattr(torch, name)] = code
    if dtype not in m:
        raise TypeError(f"unsupported dtype {dtype}")
    return m[dtype]


def _stream_ptr(stream, device: int) -> int:
    import torch
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


_HIP = None


def dedicated_stream(device: int = 0):
    """A torch ExternalStream with a hardware queue of its own (created with a full CU mask).

    Only needed when several ranks share one GPU inside one process AND the caller replays captured
    graphs of their collectives on its own streams: HIP multiplexes a process's streams onto a few
    hardware queues, and two ranks' kernels on one queue would serialise (each spins on the other).
    Direct ncclAllReduce/... calls handle this inside the library (ncclComm::internalStream)."""
    global _HIP
    import torch
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    words = (ncu + 31) // 32
    mask = (ctypes.c_uint32 * words)(*([0xFFFFFFFF] * words))
    if ncu % 32:
        mask[words - 1] = (1 << (ncu % 32)) - 1
    s = ctypes.c_void_p()
    with torch.cuda.device(device):
        rc = _HIP.hipExtStreamCreateWithCUMask(ctypes.byref(s), ctypes.c_uint32(words), mask)
    if rc != 0:
        raise RuntimeError(f"hipExtStreamCreateWithCUMask failed: {rc}")
    return torch.cuda.ExternalStream(s.value, device=device)


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


class Window:
    """An ncclWindow_t; the handle storage stays alive until the (possibly deferred) registration ends."""

    def __init__(self, comm: "Communicator"):
        self.comm = comm
        self._h = ctypes.c_void_p()

    @property
    def handle(self) -> int:
        return self._h.value or 0

    def lsa_pointer(self, offset: int, rank: int) -> int:
        """ncclGetLsaDevicePointer: byte `offset` of rank `rank`'s part of this window as mapped in this process."""
        p = ctypes.c_void_p()
        _check(load().ncclGetLsaDevicePointer(self.handle, offset, rank, ctypes.byref(p)), "ncclGetLsaDevicePointer")
        return p.value or 0


class Communicator:
    """Mirror of nccl4py's Communicator (bindings/nccl4py/nccl/core/communicator.py:223)."""

    def __init__(self, ptr: Optional[int]):
        self._h = ctypes.c_void_p(ptr)  # split / shrink inside a group: filled in when the group ends
        # the child of this communicator's latest split / shrink: inside a group the library writes its handle when the
        # group ends, so its storage lives at least as long as this parent (one such call per parent and group)
        self._child = None
        self._nranks = None
        self._rank = None
        self._device = None

    # ---- construction (nccl4py Communicator.init / init_all) ----
    @classmethod
    def init(cls, nranks: int, rank: int, unique_id, config: Optional[Config] = None) -> "Communicator":
        """unique_id: one id (bytes), or a sequence of ids for ncclCommInitRankScalable (nccl4py
        communicator.py:333-334)."""
        lib = load()
        c = ctypes.c_void_p()
        if not isinstance(unique_id, (bytes, bytearray)):
            ids = list(unique_id)
            arr = (UniqueId * len(ids))(*[_uid(b) for b in ids])
            rc = lib.ncclCommInitRankScalable(ctypes.byref(c), nranks, rank, len(ids), arr,
                                              ctypes.byref(config) if config is not None else None)
            if not (rc == Result.InProgress and config is not None and config.blocking == 0):
                _check(rc, "ncclCommInitRankScalable")
            return cls(c.value)
        if config is None:
            _check(lib.ncclCommInitRank(ctypes.byref(c), nranks, _uid(unique_id), rank), "ncclCommInitRank")
        else:
            rc = lib.ncclCommInitRankConfig(ctypes.byref(c), nranks, _uid(unique_id), rank, ctypes.byref(config))
            if not (rc == Result.InProgress and config.blocking == 0):  # non-blocking: poll wait_ready()
                _check(rc, "ncclCommInitRankConfig")
        return cls(c.value)

    def wait_ready(self, timeout_s: float = 600.0) -> None:
        """Non-blocking communicators: poll ncclCommGetAsyncError until it leaves ncclInProgress."""
        import time
        t0 = time.time()
        while True:
            e = self.async_error()
            if e != Result.InProgress:
                _check(e, "ncclCommInitRankConfig (non-blocking)")
                return
            if time.time() - t0 > timeout_s:
                raise TimeoutError("communicator still initialising")
            time.sleep(0.001)

    @classmethod
    def init_all(cls, devices: Sequence[int] | int) -> list["Communicator"]:
        lib = load()
        devs = list(range(devices)) if isinstance(devices, int) else list(devices)
        arr = (ctypes.c_void_p * len(devs))()
        dl = (ctypes.c_int * len(devs))(*devs)
        _check(lib.ncclCommInitAll(arr, len(devs), dl), "ncclCommInitAll")
        return [cls(arr[i]) for i in range(len(devs))]

    # ---- child communicators (nccl.h.in:227-240) ----
    def split(self, color: int, key: int = 0, config: Optional[Config] = None) -> Optional["Communicator"]:
        """ncclCommSplit: every rank of this communicator calls it; ranks passing the same color form one child, ordered
        by key (ties by rank here). SPLIT_NOCOLOR returns None (the rank still takes part). The call returns with the
        child ready; inside group() it runs when the group ends (one thread splitting every communicator of an
        init_all clique), and the returned object is usable from then on. One split or shrink per parent and group."""
        child = self._child = Communicator(None)
        _check(load().ncclCommSplit(self._comm, color, key, ctypes.byref(child._h),
                                    ctypes.byref(config) if config is not None else None), "ncclCommSplit")
        return None if color == SPLIT_NOCOLOR else child

    def shrink(self, exclude: Sequence[int], flags: int = SHRINK_DEFAULT, config: Optional[Config] = None) -> "Communicator":
        """ncclCommShrink: called by the ranks that are not in `exclude` (parent ranks, any order); the child keeps
        their order. SHRINK_ABORT first ends this communicator's operations in flight."""
        ex = list(exclude)
        arr = (ctypes.c_int * max(1, len(ex)))(*ex)
        child = self._child = Communicator(None)
        _check(load().ncclCommShrink(self._comm, arr if ex else None, len(ex), ctypes.byref(child._h),
                                     ctypes.byref(config) if config is not None else None, flags), "ncclCommShrink")
        return child

    # ---- properties ----
    @property
    def _comm(self) -> int:
        return self._h.value or 0

    @_comm.setter
    def _comm(self, v: int) -> None:
        self._h = ctypes.c_void_p(v)

    @property
    def ptr(self) -> int:
        return self._comm

    @property
    def nranks(self) -> int:
        if self._nranks is None:
            v = ctypes.c_int()
            _check(load().ncclCommCount(self._comm, ctypes.byref(v)), "ncclCommCount")
            self._nranks = v.value
        return self._nranks

    @property
    def rank(self) -> int:
        if self._rank is None:
            v = ctypes.c_int()
            _check(load().ncclCommUserRank(self._comm, ctypes.byref(v)), "ncclCommUserRank")
            self._rank = v.value
        return self._rank

    @property
    def device(self) -> int:
        if self._device is None:
            v = ctypes.c_int()
            _check(load().ncclCommCuDevice(self._comm, ctypes.byref(v)), "ncclCommCuDevice")
            self._device = v.value
        return self._device

    def mem_stats(self, stat: "MemStat" = MemStat.GPU_MEM_TOTAL) -> int:
        """ncclCommMemStats: device bytes this communicator holds (everything is persistent here)."""
        v = ctypes.c_uint64()
        _check(load().ncclCommMemStats(self._comm, int(stat), ctypes.byref(v)), "ncclCommMemStats")
        return v.value

    def async_error(self) -> int:
        v = ctypes.c_int()
        _check(load().ncclCommGetAsyncError(self._comm, ctypes.byref(v)), "ncclCommGetAsyncError")
        return v.value

    # ---- collectives on torch tensors ----
    def _check_tensors(self, where: str, *ts) -> None:
        """Buffers handed to the C ABI are raw pointers: they must be dense and on this communicator's GPU."""
        for t in ts:
            if t is None:
                continue
            if not t.is_contiguous():
                raise ValueError(f"{where}: tensors must be contiguous")
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError(f"{where}: tensor on {t.device}, communicator on cuda:{self.device}")

    def allreduce(self, sendbuf, recvbuf, op=RedOp.SUM, *, stream=None) -> None:
        self._check_tensors("allreduce", sendbuf, recvbuf)
        if sendbuf.numel() != recvbuf.numel() or sendbuf.dtype != recvbuf.dtype:
            raise ValueError("allreduce: sendbuf/recvbuf must match in dtype and count")
        self.all_reduce_raw(sendbuf.data_ptr(), recvbuf.data_ptr(), sendbuf.numel(),
                            torch_dtype_to_nccl(sendbuf.dtype), int(op), _stream_ptr(stream, self.device))

    def reduce_scatter(self, sendbuf, recvbuf, op=RedOp.SUM, *, stream=None) -> None:
        self._check_tensors("reduce_scatter", sendbuf, recvbuf)
        if sendbuf.numel() != recvbuf.numel() * self.nranks or sendbuf.dtype != recvbuf.dtype:
            raise ValueError("reduce_scatter: sendbuf must hold nranks * recvbuf.numel() elements of the same dtype")
        self.reduce_scatter_raw(sendbuf.data_ptr(), recvbuf.data_ptr(), recvbuf.numel(),
                                torch_dtype_to_nccl(sendbuf.dtype), int(op), _stream_ptr(stream, self.device))

    def allgather(self, sendbuf, recvbuf, *, stream=None) -> None:
        self._check_tensors("allgather", sendbuf, recvbuf)
        if recvbuf.numel() != sendbuf.numel() * self.nranks or sendbuf.dtype != recvbuf.dtype:
            raise ValueError("allgather: recvbuf must hold nranks * sendbuf.numel() elements of the same dtype")
        self.all_gather_raw(sendbuf.data_ptr(), recvbuf.data_ptr(), sendbuf.numel(),
                            torch_dtype_to_nccl(sendbuf.dtype), _stream_ptr(stream, self.device))

    def reduce(self, sendbuf, recvbuf, op=RedOp.SUM, root: int = 0, *, stream=None) -> None:
        self._check_tensors("reduce", sendbuf, recvbuf if self.rank == root else None)
        if self.rank == root and (recvbuf is None or recvbuf.numel() != sendbuf.numel()
                                  or recvbuf.dtype != sendbuf.dtype):
            raise ValueError("reduce: the root's recvbuf must match sendbuf in dtype and count")
        self.reduce_raw(sendbuf.data_ptr(), _ptr(recvbuf), sendbuf.numel(), torch_dtype_to_nccl(sendbuf.dtype),
                        int(op), root, _stream_ptr(stream, self.device))

    def broadcast(self, sendbuf, recvbuf, root: int = 0, *, stream=None) -> None:
        """recvbuf on every rank := the root's sendbuf (sendbuf is read on the root only: None elsewhere is fine)."""
        self._check_tensors("broadcast", sendbuf if self.rank == root else None, recvbuf)
        if self.rank == root and (sendbuf is None or sendbuf.numel() != recvbuf.numel()
                                  or sendbuf.dtype != recvbuf.dtype):
            raise ValueError("broadcast: the root's sendbuf must match recvbuf in dtype and count")
        self.broadcast_raw(_ptr(sendbuf) if self.rank == root else None, recvbuf.data_ptr(), recvbuf.numel(),
                           torch_dtype_to_nccl(recvbuf.dtype), root, _stream_ptr(stream, self.device))

    def bcast(self, buf, root: int = 0, *, stream=None) -> None:
        """In place: buf on every rank := the root's buf (ncclBcast)."""
        self._check_tensors("bcast", buf)
        _check(load().ncclBcast(buf.data_ptr(), buf.numel(), torch_dtype_to_nccl(buf.dtype), root, self._comm,
                                _stream_ptr(stream, self.device)), "ncclBcast")

    # ---- point-to-point, and the collectives built from it ----
    def send(self, tensor, peer: int, *, stream=None) -> None:
        """Send `tensor` to rank `peer`, whose matching recv has the same dtype and count. Sends and recvs that must
        progress together (an exchange) go inside one group()."""
        self._check_tensors("send", tensor)
        self.send_raw(tensor.data_ptr(), tensor.numel(), torch_dtype_to_nccl(tensor.dtype), peer,
                      _stream_ptr(stream, self.device))

    def recv(self, tensor, peer: int, *, stream=None) -> None:
        """Receive into `tensor` what rank `peer` sends."""
        self._check_tensors("recv", tensor)
        self.recv_raw(tensor.data_ptr(), tensor.numel(), torch_dtype_to_nccl(tensor.dtype), peer,
                      _stream_ptr(stream, self.device))

    def alltoall(self, sendbuf, recvbuf, *, stream=None) -> None:
        """Block j of sendbuf goes to rank j; block i of recvbuf comes from rank i (nranks equal blocks each). With
        sendbuf inside a WIN_COLL_SYMMETRIC window (the same offset on every rank) the call runs zero-copy."""
        self._check_tensors("alltoall", sendbuf, recvbuf)
        if sendbuf.numel() != recvbuf.numel() or sendbuf.dtype != recvbuf.dtype or sendbuf.numel() % self.nranks:
            raise ValueError("alltoall: sendbuf/recvbuf must match in dtype and hold nranks equal blocks")
        self.alltoall_raw(sendbuf.data_ptr(), recvbuf.data_ptr(), sendbuf.numel() // self.nranks,
                          torch_dtype_to_nccl(sendbuf.dtype), _stream_ptr(stream, self.device))

    def gather(self, sendbuf, recvbuf, root: int = 0, *, stream=None) -> None:
        """The root's recvbuf := every rank's sendbuf, rank i's at block i (recvbuf is used on the root only). With
        sendbuf inside a WIN_COLL_SYMMETRIC window (the same offset on every rank) the call runs zero-copy."""
        self._check_tensors("gather", sendbuf, recvbuf if self.rank == root else None)
        if self.rank == root and (recvbuf is None or recvbuf.numel() != sendbuf.numel() * self.nranks
                                  or recvbuf.dtype != sendbuf.dtype):
            raise ValueError("gather: the root's recvbuf must hold nranks * sendbuf.numel() elements of the same dtype")
        self.gather_raw(sendbuf.data_ptr(), _ptr(recvbuf) if self.rank == root else None, sendbuf.numel(),
                        torch_dtype_to_nccl(sendbuf.dtype), root, _stream_ptr(stream, self.device))

    def scatter(self, sendbuf, recvbuf, root: int = 0, *, stream=None) -> None:
        """Every rank's recvbuf := block i of the root's sendbuf (sendbuf is used on the root only)."""
        self._check_tensors("scatter", sendbuf if self.rank == root else None, recvbuf)
        if self.rank == root and (sendbuf is None or sendbuf.numel() != recvbuf.numel() * self.nranks
                                  or sendbuf.dtype != recvbuf.dtype):
            raise ValueError("scatter: the root's sendbuf must hold nranks * recvbuf.numel() elements of the same dtype")
        self.scatter_raw(_ptr(sendbuf) if self.rank == root else None, recvbuf.data_ptr(), recvbuf.numel(),
                         torch_dtype_to_nccl(recvbuf.dtype), root, _stream_ptr(stream, self.device))

    # ---- one-sided operations on registered windows ----
    def put_signal(self, tensor, peer: int, win, offset: int = 0, *, stream=None) -> None:
        """Write `tensor` (inside a WIN_COLL_SYMMETRIC window of this communicator) into rank `peer`'s part of window
        `win` at byte `offset`, then raise the signal `peer` holds for this rank by one."""
        self._check_tensors("put_signal", tensor)
        self.put_signal_raw(tensor.data_ptr(), tensor.numel(), torch_dtype_to_nccl(tensor.dtype), peer, win, offset,
                            _stream_ptr(stream, self.device))

    def signal(self, peer: int, *, stream=None, sig_idx: int = 0, ctx: int = 0, flags: int = 0) -> None:
        """Raise the signal rank `peer` holds for this rank by one; no data moves (ncclSignal)."""
        _check(load().ncclSignal(peer, sig_idx, ctx, flags, self._comm, _stream_ptr(stream, self.device)), "ncclSignal")

    def wait_signal(self, descs, *, stream=None) -> None:
        """ncclWaitSignal: `descs` is a sequence of (peer, op_cnt) pairs or WaitSignalDesc; the stream waits until
        op_cnt further signals from each peer have arrived and consumes them (entries naming one peer add up)."""
        ds = [d if isinstance(d, WaitSignalDesc) else WaitSignalDesc(int(d[1]), int(d[0]), 0, 0) for d in descs]
        arr = (WaitSignalDesc * max(1, len(ds)))(*ds)
        _check(load().ncclWaitSignal(len(ds), arr, self._comm, _stream_ptr(stream, self.device)), "ncclWaitSignal")

    # ---- collectives on raw device pointers (the C ABI one-to-one) ----
    def all_reduce_raw(self, send: int, recv: int, count: int, dtype: int, op: int, stream: int) -> None:
        _check(load().ncclAllReduce(send, recv, count, dtype, op, self._comm, stream), "ncclAllReduce")

    def reduce_scatter_raw(self, send: int, recv: int, recvcount: int, dtype: int, op: int, stream: int) -> None:
        _check(load().ncclReduceScatter(send, recv, recvcount, dtype, op, self._comm, stream), "ncclReduceScatter")

    def all_gather_raw(self, send: int, recv: int, sendcount: int, dtype: int, stream: int) -> None:
        _check(load().ncclAllGather(send, recv, sendcount, dtype, self._comm, stream), "ncclAllGather")

    def reduce_raw(self, send: int, recv: Optional[int], count: int, dtype: int, op: int, root: int,
                   stream: int) -> None:
        _check(load().ncclReduce(send, recv, count, dtype, op, root, self._comm, stream), "ncclReduce")

    def broadcast_raw(self, send: Optional[int], recv: int, count: int, dtype: int, root: int, stream: int) -> None:
        _check(load().ncclBroadcast(send, recv, count, dtype, root, self._comm, stream), "ncclBroadcast")

    def send_raw(self, send: int, count: int, dtype: int, peer: int, stream: int) -> None:
        _check(load().ncclSend(send, count, dtype, peer, self._comm, stream), "ncclSend")

    def recv_raw(self, recv: int, count: int, dtype: int, peer: int, stream: int) -> None:
        _check(load().ncclRecv(recv, count, dtype, peer, self._comm, stream), "ncclRecv")

    def alltoall_raw(self, send: int, recv: int, count: int, dtype: int, stream: int) -> None:
        _check(load().ncclAlltoAll(send, recv, count, dtype, self._comm, stream), "ncclAlltoAll")

    def gather_raw(self, send: int, recv: Optional[int], count: int, dtype: int, root: int, stream: int) -> None:
        _check(load().ncclGather(send, recv, count, dtype, root, self._comm, stream), "ncclGather")

    def scatter_raw(self, send: Optional[int], recv: int, count: int, dtype: int, root: int, stream: int) -> None:
        _check(load().ncclScatter(send, recv, count, dtype, root, self._comm, stream), "ncclScatter")

    def put_signal_raw(self, local: Optional[int], count: int, dtype: int, peer: int, win, offset: int, stream: int,
                       sig_idx: int = 0, ctx: int = 0, flags: int = 0) -> None:
        h = win.handle if isinstance(win, Window) else win
        _check(load().ncclPutSignal(local, count, dtype, peer, h, offset, sig_idx, ctx, flags, self._comm, stream),
               "ncclPutSignal")

    # ---- registration (nccl.h.in:301-360; nccl4py Communicator.register_buffer / register_window) ----
    def register_buffer(self, ptr: int, size: int) -> int:
        """ncclCommRegister (local); returns the handle."""
        h = ctypes.c_void_p()
        _check(load().ncclCommRegister(self._comm, ptr, size, ctypes.byref(h)), "ncclCommRegister")
        return h.value or 0

    def deregister_buffer(self, handle: int) -> None:
        _check(load().ncclCommDeregister(self._comm, handle), "ncclCommDeregister")

    def register_window(self, ptr: int, size: int, flags: int = WIN_COLL_SYMMETRIC) -> "Window":
        """ncclCommWindowRegister (collective: every rank calls it; one thread driving several ranks
        calls it inside group(), and the handle is filled in when the group ends)."""
        w = Window(self)
        _check(load().ncclCommWindowRegister(self._comm, ptr, size, ctypes.byref(w._h), flags),
               "ncclCommWindowRegister")
        return w

    def deregister_window(self, win) -> None:
        h = win.handle if isinstance(win, Window) else win
        _check(load().ncclCommWindowDeregister(self._comm, h), "ncclCommWindowDeregister")

    def window_user_ptr(self, win) -> int:
        h = win.handle if isinstance(win, Window) else win
        p = ctypes.c_void_p()
        _check(load().ncclWinGetUserPtr(self._comm, h, ctypes.byref(p)), "ncclWinGetUserPtr")
        return p.value or 0

    # ---- device API (include/nccl_device.h) ----
    def query_properties(self) -> CommProperties:
        """ncclCommQueryProperties."""
        p = CommProperties.default()
        _check(load().ncclCommQueryProperties(self._comm, ctypes.byref(p)), "ncclCommQueryProperties")
        return p

    def dev_comm_create(self, lsa_barriers: int = 0, buffers=(), requirements: Optional[DevCommRequirements] = None) -> DevComm:
        """ncclDevCommCreate (collective: every rank calls it with the same arguments; one thread driving several
        ranks calls it inside group(), and the struct and handles are filled in when the group ends). `buffers` is a
        sequence of (size, align) resource buffers; `requirements` overrides the struct built from the two."""
        d = DevComm(self, lsa_barriers, list(buffers))
        q = requirements if requirements is not None else DevCommRequirements.default(lsaBarrierCount=lsa_barriers)
        if requirements is None and d._nbuf:
            q.resourceRequirementsList = ctypes.pointer(d._reqs[0])
        _check(load().ncclDevCommCreate(self._comm, ctypes.byref(q), ctypes.byref(d.struct)), "ncclDevCommCreate")
        return d

    def dev_comm_destroy(self, dev_comm: DevComm) -> None:
        _check(load().ncclDevCommDestroy(self._comm, ctypes.byref(dev_comm.struct)), "ncclDevCommDestroy")

    # ---- custom operators ----
    def create_pre_mul_sum(self, scalar, dtype: int, device_scalar_ptr: Optional[int] = None) -> int:
        """ncclRedOpCreatePreMulSum; `scalar` is a host value (ncclScalarHostImmediate) unless
        `device_scalar_ptr` is given (ncclScalarDevice)."""
        import numpy as np
        op = ctypes.c_int()
        if device_scalar_ptr is not None:
            _check(load().ncclRedOpCreatePreMulSum(ctypes.byref(op), device_scalar_ptr, dtype, 0, self._comm),
                   "ncclRedOpCreatePreMulSum")
        else:
            npdt = {0: np.int8, 1: np.uint8, 2: np.int32, 3: np.uint32, 4: np.int64, 5: np.uint64, 6: np.float16,
                    7: np.float32, 8: np.float64}.get(dtype)
            if npdt is not None:
                buf = np.array([scalar], dtype=npdt).tobytes()
            else:  # bf16 / fp8: caller passes the raw bit pattern as an int
                buf = int(scalar).to_bytes(TYPE_SIZE[dtype], "little")
            cbuf = ctypes.create_string_buffer(buf, 8)
            _check(load().ncclRedOpCreatePreMulSum(ctypes.byref(op), cbuf, dtype, 1, self._comm),
                   "ncclRedOpCreatePreMulSum")
        return op.value

    def destroy_op(self, op: int) -> None:
        _check(load().ncclRedOpDestroy(op, self._comm), "ncclRedOpDestroy")

    # ---- teardown ----
    def finalize(self) -> None:
        _check(load().ncclCommFinalize(self._comm), "ncclCommFinalize")

    def destroy(self) -> None:
        if self._comm:
            _check(load().ncclCommDestroy(self._comm), "ncclCommDestroy")
            self._comm = 0

    def abort(self) -> None:
        if self._comm:
            _check(load().ncclCommAbort(self._comm), "ncclCommAbort")
            self._comm = 0


def ddp_comm_hook(comm: "Communicator"):
    """A torch DDP communication hook that reduces every gradient bucket with this engine (ncclAvg, in
    place, on the current stream) instead of the process group's backend:
    ``ddp_model.register_comm_hook(None, nccl_amd.ddp_comm_hook(comm))``."""
    import torch

    def hook(state, bucket):
        t = bucket.buffer()
        comm.allreduce(t, t, RedOp.AVG)
        fut = torch.futures.Future()
        fut.set_result(t)
        return fut

    return hook
