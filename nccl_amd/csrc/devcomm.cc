// devcomm.cc — host side of the device API (include/nccl_device.h).
//
// Reference: src/include/nccl_device/core.h:194-205 (ncclCommQueryProperties, ncclDevCommCreate / Destroy, the host
// pointer getters), src/dev_runtime.cc (the resource window of a DevComm). A DevComm here owns one uncached,
// zero-filled allocation per rank holding the LSA barriers' epochs and inboxes and the caller's resource buffers
// (ncclDevCommResourceLayout), registered with every peer through the window path (register.cc windowRegister) as a
// symmetric "resource window": the resource-buffer getters are window getters, and ncclDevComm carries a copy of that
// window's table beside the communicator's abort word, error word and spin timeout.
#include <string.h>

#include <algorithm>
#include <mutex>

#include "core.h"

namespace ncclamd {

struct DevCommState {
  void* mem;               // this rank's resource allocation
  size_t bytes;
  ncclWindow_vidmem* win;  // its window (nullptr once windowsFree released it)
};

struct DevCommPlan {  // one rank's requirements, resolved
  int lsaBarrierCount;
  std::vector<size_t> sizes, aligns, offsets;
  std::vector<ncclDevResourceHandle_t*> outHandles;
  ncclDevResourceLayout layout;
};

struct DevCommSummary {  // compared across ranks: every rank must ask for the same resources
  int32_t lsaBarrierCount;
  int32_t nBuffers;
  uint64_t totalBytes;
  uint64_t digest;  // of every buffer's size and alignment, in list order
  uint64_t allocated;  // this rank has its memory (1 on every rank, or the creation fails on every rank)
};

size_t devCommBytes(const ncclComm* comm) {
  size_t b = 0;
  for (const DevCommState* s : comm->devComms) b += s->bytes;
  return b;
}

static void devCommRelease(ncclComm* comm, DevCommState* s, bool dropWindow) {
  if (dropWindow && s->win) windowDrop(comm, s->win);
  if (s->mem) {
    std::lock_guard<std::mutex> g(ipcMapMutex());
    (void)hipFree(s->mem);
  }
  delete s;
}

void devCommsFree(ncclComm* comm) {
  for (DevCommState* s : comm->devComms) devCommRelease(comm, s, /*dropWindow=*/false);
  comm->devComms.clear();
}

bool devCommOwnsWindow(const ncclComm* comm, const ncclWindow_vidmem* w) {
  for (const DevCommState* s : comm->devComms)
    if (s->win == w) return true;
  return false;
}

static ncclResult_t refuse(const char* field) {
  WARN("ncclDevCommCreate: requirement %s has no counterpart on this engine (LSA device API only)", field);
  return ncclInvalidUsage;
}

// The checks of one rank's requirements, without touching a device.
static ncclResult_t devCommResolve(const ncclDevCommRequirements* q, int nRanks, DevCommPlan* plan) {
  if (q->lsaMultimem) return refuse("lsaMultimem");
  if (q->ginConnectionType != NCCL_GIN_CONNECTION_NONE) return refuse("ginConnectionType");
  if (q->ginForceEnable) return refuse("ginForceEnable");
  if (q->barrierCount != 0) return refuse("barrierCount");
  if (q->railGinBarrierCount != 0) return refuse("railGinBarrierCount");
  if (q->worldGinBarrierCount != 0) return refuse("worldGinBarrierCount");
  if (q->lsaLLA2ABlockCount != 0) return refuse("lsaLLA2ABlockCount");
  if (q->lsaLLA2ASlotCount != 0) return refuse("lsaLLA2ASlotCount");
  if (q->ginSignalCount != 0) return refuse("ginSignalCount");
  if (q->ginCounterCount != 0) return refuse("ginCounterCount");
  if (q->teamRequirementsList != nullptr) return refuse("teamRequirementsList");
  if (q->lsaBarrierCount < 0 || q->lsaBarrierCount > NCCL_DEVICE_MAX_LSA_BARRIERS) {
    WARN("ncclDevCommCreate: lsaBarrierCount %d is outside [0, %d]", q->lsaBarrierCount, NCCL_DEVICE_MAX_LSA_BARRIERS);
    return ncclInvalidArgument;
  }
  plan->lsaBarrierCount = q->lsaBarrierCount;
  int k = 0;
  for (const ncclDevResourceRequirements* r = q->resourceRequirementsList; r; r = r->next, k++) {
    if (k >= 1024) {
      WARN("ncclDevCommCreate: resourceRequirementsList holds more than 1024 entries (or is a cycle)");
      return ncclInvalidArgument;
    }
    if (r->ginSignalCount != 0) return refuse("resourceRequirementsList[].ginSignalCount");
    if (r->ginCounterCount != 0) return refuse("resourceRequirementsList[].ginCounterCount");
    const size_t a = r->bufferAlign ? r->bufferAlign : 1;
    if ((a & (a - 1)) != 0 || a > NCCL_DEVICE_MAX_BUFFER_ALIGN || r->bufferSize > ((size_t)1 << 40)) {
      WARN("ncclDevCommCreate: resource buffer %d: size %zu align %zu (a power of two up to %d)", k, r->bufferSize,
           r->bufferAlign, NCCL_DEVICE_MAX_BUFFER_ALIGN);
      return ncclInvalidArgument;
    }
    plan->sizes.push_back(r->bufferSize);
    plan->aligns.push_back(a);
    plan->outHandles.push_back(r->outBufferHandle);
  }
  plan->offsets.assign(plan->sizes.size(), 0);
  plan->layout = ncclDevCommResourceLayout(nRanks, plan->lsaBarrierCount, (int)plan->sizes.size(), plan->sizes.data(),
                                           plan->aligns.data(), plan->offsets.data());
  if (plan->layout.totalBytes / NCCL_DEVICE_RESOURCE_GRANULE > 0xffffffffull) {
    WARN("ncclDevCommCreate: %zu bytes of resources are beyond a resource handle's range", plan->layout.totalBytes);
    return ncclInvalidArgument;
  }
  return ncclSuccess;
}

static DevCommSummary summarise(const DevCommPlan& p) {
  DevCommSummary s = {p.lsaBarrierCount, (int32_t)p.sizes.size(), p.layout.totalBytes, 0xcbf29ce484222325ull, 1};
  for (size_t k = 0; k < p.sizes.size(); k++)
    for (uint64_t v : {(uint64_t)p.sizes[k], (uint64_t)p.aligns[k]}) s.digest = (s.digest ^ v) * 0x100000001b3ull;
  return s;
}

// The collective part: allocate, agree, register, fill *out.
static ncclResult_t devCommCreate(ncclComm* comm, const DevCommPlan& plan, ncclDevComm* out) {
  HIPCHECK(hipSetDevice(comm->device));
  const int n = comm->nRanks, me = comm->rank;
  // This rank's allocation first, so that its outcome travels with the summary: a rank without memory fails every
  // rank together instead of leaving its peers in the registration's exchange.
  DevCommState* st = new DevCommState{nullptr, plan.layout.totalBytes, nullptr};
  hipError_t e;
  {
    std::lock_guard<std::mutex> g(ipcMapMutex());
    e = hipExtMallocWithFlags(&st->mem, st->bytes, hipDeviceMallocUncached);
  }
  if (e != hipSuccess) st->mem = nullptr;
  if (e == hipSuccess) e = hipMemset(st->mem, 0, st->bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // zero before any peer can reach it (the exchanges below)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    WARN("ncclDevCommCreate: %zu bytes of uncached resource memory: %s", st->bytes, hipGetErrorString(e));
  }
  std::vector<DevCommSummary> all(n);
  all[me] = summarise(plan);
  all[me].allocated = e == hipSuccess;
  ncclResult_t res = commAllGather(comm, all.data(), sizeof(DevCommSummary));
  for (int r = 0; r < n && res == ncclSuccess; r++) {  // every rank sees the same table: all fail together
    if (!all[r].allocated) {
      if (r != me) WARN("ncclDevCommCreate: rank %d could not allocate its resources", r);
      res = ncclUnhandledCudaError;
    } else if (memcmp(&all[r], &all[me], sizeof(DevCommSummary)) != 0) {
      WARN("ncclDevCommCreate: rank %d asked for %d LSA barriers, %d buffers, %lu bytes; rank %d for %d, %d, %lu: every "
           "rank must pass the same requirements", me, all[me].lsaBarrierCount, all[me].nBuffers,
           (unsigned long)all[me].totalBytes, r, all[r].lsaBarrierCount, all[r].nBuffers, (unsigned long)all[r].totalBytes);
      res = ncclInvalidArgument;
    }
  }
  ncclWindow_t win = nullptr;
  if (res == ncclSuccess) res = windowRegister(comm, st->mem, st->bytes, &win, NCCL_WIN_COLL_SYMMETRIC);
  if (res != ncclSuccess) {
    devCommRelease(comm, st, false);
    return res;
  }
  st->win = win;
  comm->devComms.push_back(st);

  memset(out, 0, sizeof(*out));
  out->magic = NCCL_API_MAGIC;
  out->version = NCCL_VERSION_CODE;
  out->rank = out->lsaRank = me;
  out->nRanks = out->lsaSize = n;
  out->resourceWindow = win;
  for (int r = 0; r < n; r++) out->resourceWindow_inlined.peerPtr[r] = win->peerPtr[r];
  out->lsaBarrier.bufHandle = (ncclDevResourceHandle_t)(plan.layout.epochOffset / NCCL_DEVICE_RESOURCE_GRANULE);
  out->lsaBarrier.nBarriers = plan.lsaBarrierCount;
  out->abortFlag = comm->hostDevComm.abortFlag;
  out->errorWord = comm->hostDevComm.errorWord;
  out->timeoutTicks = comm->hostDevComm.timeoutTicks;
  out->hostState = st;
  for (size_t k = 0; k < plan.offsets.size(); k++)
    if (plan.outHandles[k])
      *plan.outHandles[k] = (ncclDevResourceHandle_t)(plan.offsets[k] / NCCL_DEVICE_RESOURCE_GRANULE);
  INFO("rank %d: DevComm with %d LSA barriers, %zu buffers, %zu bytes of resources", me, plan.lsaBarrierCount,
       plan.sizes.size(), st->bytes);
  return ncclSuccess;
}

// size / magic of a caller-initialised struct, as ncclConfig_t's are checked (init.cc checkConfig)
template <typename T>
static bool structOk(const T* s) {
  return s->magic == NCCL_API_MAGIC && s->size >= sizeof(T);
}

static ncclResult_t windowPointer(const char* fn, ncclWindow_t w, size_t offset, int rank, void** outPtr) {
  if (w == nullptr || outPtr == nullptr) {
    WARN("%s : NULL argument", fn);
    return ncclInvalidArgument;
  }
  if (rank < 0 || rank >= w->nRanks) {
    WARN("%s : rank %d is outside [0, %d)", fn, rank, w->nRanks);
    return ncclInvalidArgument;
  }
  if (offset >= w->peerSize[rank]) {
    WARN("%s : offset %zu is outside the %zu bytes rank %d registered", fn, offset, w->peerSize[rank], rank);
    return ncclInvalidArgument;
  }
  *outPtr = w->peerPtr[rank] + offset;
  return ncclSuccess;
}

}  // namespace ncclamd

using namespace ncclamd;

#define NCCL_ALIAS(ret, name, ...) extern "C" __attribute__((visibility("default"), alias(#name))) ret p##name(__VA_ARGS__);

NCCL_EXPORT ncclResult_t ncclCommQueryProperties(ncclComm_t comm, ncclCommProperties_t* props) {
  // the caller's struct first: its check needs no communicator
  if (props == nullptr || !structOk(props)) {
    WARN("ncclCommQueryProperties : props is NULL or was not initialized with NCCL_COMM_PROPERTIES_INITIALIZER");
    return ncclInvalidArgument;
  }
  NCCLCHECK(commCheck(comm, "ncclCommQueryProperties", "comm"));
  props->rank = comm->rank;
  props->nRanks = comm->nRanks;
  props->cudaDev = comm->device;
  props->nvmlDev = -1;
  props->deviceApiSupport = true;
  props->multimemSupport = false;
  props->ginType = NCCL_GIN_TYPE_NONE;
  props->nLsaTeams = 1;
  props->hostRmaSupport = true;  // ncclPutSignal / ncclSignal / ncclWaitSignal
  props->railedGinType = NCCL_GIN_TYPE_NONE;
  return ncclSuccess;
}
NCCL_ALIAS(ncclResult_t, ncclCommQueryProperties, ncclComm_t, ncclCommProperties_t*)

NCCL_EXPORT ncclResult_t ncclDevCommCreate(ncclComm_t comm, const ncclDevCommRequirements_t* reqs,
                                           ncclDevComm_t* outDevComm) {
  if (reqs == nullptr || outDevComm == nullptr || !structOk(reqs)) {
    WARN("ncclDevCommCreate : NULL argument, or reqs was not initialized with NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER");
    groupRecordError(ncclInvalidArgument);
    return ncclInvalidArgument;
  }
  NCCLCHECK(commCheck(comm, "ncclDevCommCreate", "comm"));
  int st = comm->asyncResult.load();
  if (st != ncclSuccess) return st == ncclInProgress ? ncclInProgress : ncclInvalidUsage;
  DevCommPlan plan;
  ncclResult_t res = devCommResolve(reqs, comm->nRanks, &plan);  // (the list is read now: it need not outlive the call)
  if (res != ncclSuccess) {
    groupRecordError(res);
    return res;
  }
  ipcDrainReleases();
  regBlockingPoint(comm);
  ROCTX_RANGE("ncclDevCommCreate comm=%p barriers=%d", (void*)comm, plan.lsaBarrierCount);
  // collective, like ncclCommWindowRegister: inside a group every rank's part runs concurrently at ncclGroupEnd
  if (groupActive()) return groupDeferInit([=]() { return devCommCreate(comm, plan, outDevComm); });
  DeviceRestore restore;
  return devCommCreate(comm, plan, outDevComm);
}
NCCL_ALIAS(ncclResult_t, ncclDevCommCreate, ncclComm_t, const ncclDevCommRequirements_t*, ncclDevComm_t*)

NCCL_EXPORT ncclResult_t ncclDevCommDestroy(ncclComm_t comm, const ncclDevComm_t* devComm) {
  if (devComm == nullptr || devComm->magic != NCCL_API_MAGIC) {
    WARN("ncclDevCommDestroy : devComm is NULL or was not made by ncclDevCommCreate");
    return ncclInvalidArgument;
  }
  NCCLCHECK(commCheck(comm, "ncclDevCommDestroy", "comm"));
  auto it = std::find(comm->devComms.begin(), comm->devComms.end(), (DevCommState*)devComm->hostState);
  if (it == comm->devComms.end()) {
    WARN("ncclDevCommDestroy : this communicator holds no such DevComm (destroyed already?)");
    return ncclInvalidArgument;
  }
  ipcDrainReleases();
  regBlockingPoint(comm);
  // kernels enqueued on it may still run: wait for the device before the peers' mappings and the memory go
  DeviceRestore restore;
  HIPCHECK(hipSetDevice(comm->device));
  HIPCHECK(hipDeviceSynchronize());
  DevCommState* s = *it;
  comm->devComms.erase(it);
  devCommRelease(comm, s, /*dropWindow=*/true);
  return ncclSuccess;
}
NCCL_ALIAS(ncclResult_t, ncclDevCommDestroy, ncclComm_t, const ncclDevComm_t*)

NCCL_EXPORT ncclResult_t ncclGetLsaDevicePointer(ncclWindow_t window, size_t offset, int lsaRank, void** outPtr) {
  return windowPointer("ncclGetLsaDevicePointer", window, offset, lsaRank, outPtr);
}
NCCL_ALIAS(ncclResult_t, ncclGetLsaDevicePointer, ncclWindow_t, size_t, int, void**)

NCCL_EXPORT ncclResult_t ncclGetPeerDevicePointer(ncclWindow_t window, size_t offset, int peer, void** outPtr) {
  return windowPointer("ncclGetPeerDevicePointer", window, offset, peer, outPtr);
}
NCCL_ALIAS(ncclResult_t, ncclGetPeerDevicePointer, ncclWindow_t, size_t, int, void**)
