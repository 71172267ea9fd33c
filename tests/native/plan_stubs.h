// plan_stubs.h — what the CPU plan drivers (plan_test, bcast_plan_test, p2p_plan_test, rma_plan_test) share: the few
// HIP runtime calls the planning sources make and the library functions they call outside themselves, stubbed so that
// every plan is recorded instead of launched. One translation unit per driver includes it once. The switches in
// gStubs default to plan_test's behaviour; a driver sets what it needs before it plans.
#pragma once
#include <stdint.h>

#include "../../nccl_amd/csrc/core.h"

// ---- HIP runtime stubs (the planning sources only set the device, query attributes and record events) ----
static bool gStubCapturing = false;   // hipStreamIsCapturing answers "active" for every stream
static bool gStubHostMemory = false;  // hipPointerGetAttributes answers "pinned host memory" for every pointer
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attr, const void* p) {
  if (!gStubHostMemory) return hipErrorInvalidValue;
  *attr = {};
  attr->type = hipMemoryTypeHost;
  attr->devicePointer = const_cast<void*>(p);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) {
  *st = gStubCapturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
}

namespace ncclamd {
struct PlanStubs {
  // switches
  bool refuseLaunch = false;     // launchPlan answers ncclInternalError (drivers whose code never launches a collective)
  bool refuseSymLaunch = false;  // launchSymPlan / bounceLaunch answer ncclInternalError
  bool regLookupAlways = false;  // regLookup: true whatever is asked (default: its `eager` argument — eager
                                 // registration of an eligible op succeeds, the plan shows the zero-copy kernel)
  bool regCoversAnswer = false;  // regCovers
  int tunerAlgo = -1, tunerNch = 0;  // tunerAlgo >= 0: tunerPick answers (tunerAlgo, tunerNch); else *nch = 0 only
  bool bounce = false;           // a regLookup that succeeds does so through the bounce allocation (comm->bounceUsed)
  // called with what planning passes OUT to findSymWindow / regLookup / regCovers / tunerPick (extents, byte counts,
  // masks), so that a driver can record them beside the plans
  void (*onCall)(const char* what, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t e, uint64_t f) = nullptr;
  // what was launched last, and hooks called on every launch
  LaunchPlan plan;
  SymPlan sym;
  int kind = -1;  // 0 LaunchPlan, 1 SymPlan
  int launches = 0;
  void (*onLaunch)(const LaunchPlan&) = nullptr;
  void (*onSymLaunch)(const SymPlan&) = nullptr;
};
static PlanStubs gStubs;

ncclResult_t launchPlan(const LaunchPlan& p) {
  if (gStubs.refuseLaunch) return ncclInternalError;
  gStubs.plan = p;
  gStubs.kind = 0;
  gStubs.launches++;
  if (gStubs.onLaunch) gStubs.onLaunch(p);
  return ncclSuccess;
}
ncclResult_t launchSymPlan(const SymPlan& p) {
  if (gStubs.refuseSymLaunch) return ncclInternalError;
  gStubs.sym = p;
  gStubs.kind = 1;
  gStubs.launches++;
  if (gStubs.onSymLaunch) gStubs.onSymLaunch(p);
  return ncclSuccess;
}
ncclResult_t bounceLaunch(ncclComm*, const SymPlan& sp) { return launchSymPlan(sp); }
// register.cc's lookup, over the windows the driver put into comm->windows (none: no window holds anything). A fake
// symmetric window is a ncclWindow_vidmem of the driver's with NCCL_WIN_COLL_SYMMETRIC covering its buffers.
ncclWindow_vidmem* findSymWindow(ncclComm* comm, const void* p, size_t bytes) {
  const uintptr_t a = (uintptr_t)p;
  if (gStubs.onCall) gStubs.onCall("findSymWindow", a, bytes, 0, 0, 0, 0);
  for (ncclWindow_vidmem* w : comm->windows) {
    const uintptr_t b = (uintptr_t)w->userPtr;
    if ((w->flags & NCCL_WIN_COLL_SYMMETRIC) && a >= b && a + bytes <= b + w->size) return w;
  }
  return nullptr;
}
bool regLookup(ncclComm* comm, hipStream_t stream, const void* send, size_t sendBytes, const void* recv, size_t recvBytes,
               const char**, char**, bool eager) {
  if (gStubs.onCall)
    gStubs.onCall("regLookup", (uintptr_t)stream, (uintptr_t)send, sendBytes, (uintptr_t)recv, recvBytes, eager);
  if (!gStubs.regLookupAlways && !eager) return false;
  // as register.cc leaves the communicator after a hit: the registrations found and, when it bounced, the copies
  comm->regLastUse[0] = (RegAlloc*)0xa000;
  comm->regLastUse[1] = (RegAlloc*)0xa800;
  comm->bounceUsed = gStubs.bounce;
  if (gStubs.bounce) comm->bounceNext = {(RegAlloc*)0xb000, send, (void*)recv, (char*)0xc000, (char*)0xd000, sendBytes, recvBytes};
  return true;
}
bool regCovers(ncclComm*, const void* p, size_t bytes) {
  if (gStubs.onCall) gStubs.onCall("regCovers", (uintptr_t)p, bytes, 0, 0, 0, 0);
  return gStubs.regCoversAnswer;
}
void tunerPick(ncclComm*, CollFunc func, size_t bytes, int numPipeOps, int llMask, int regBuff, int* algo, int* nch) {
  if (gStubs.onCall) gStubs.onCall("tunerPick", func, bytes, numPipeOps, llMask, regBuff, 0);
  if (gStubs.tunerAlgo >= 0) *algo = gStubs.tunerAlgo;
  *nch = gStubs.tunerAlgo >= 0 ? gStubs.tunerNch : 0;
}
ncclResult_t commCheck(const ncclComm* c, const char*, const char*) { return c ? ncclSuccess : ncclInvalidArgument; }
void commPollAsync(ncclComm*) {}
void ipcDrainReleases() {}
void ipcProgressReleases() {}
void ipcNoteLaunch(hipStream_t, int) {}
bool ipcLibraryIdle() { return true; }
void regProgress(ncclComm*) {}
void regRecordUse(ncclComm*, const SymPlan&) {}
#ifdef PLAN_STUBS_NO_GROUP
// no group machinery: every call is planned and launched at once
bool groupActive() { return false; }
ncclResult_t groupDeferColl(const CollInfo&) { return ncclSuccess; }
void groupRecordError(ncclResult_t) {}
#endif

// A communicator as commDefaults would leave it for n ranks on one channel-cap, with the tuning the environment gives.
// slotBytes 0: commDefaults' slot size, 1 GiB staging budget / (channels x 2 kinds x 2 slots x n), in [16 KiB, 1 MiB].
static void stubComm(ncclComm& comm, int n, int rank, size_t slotBytes, int chanCap) {
  comm.startMagic = comm.endMagic = kCommMagic;
  comm.rank = rank;
  comm.nRanks = n;
  comm.device = 0;
  comm.minCTAs = 1;
  comm.maxCTAs = comm.maxChannels = 256;
  comm.nSlots = 2;
  if (slotBytes == 0) {
    slotBytes = ((size_t)1 << 30) / (256 * 2 * 2 * (n > 1 ? n : 2));
    if (slotBytes > ((size_t)1 << 20)) slotBytes = (size_t)1 << 20;
    if (slotBytes < ((size_t)16 << 10)) slotBytes = (size_t)16 << 10;
  }
  comm.slotBytes = slotBytes;
  comm.chanCap = chanCap;
  comm.devComm = (DevComm*)0x1000;
  loadTuning(&comm.tune);
}
}  // namespace ncclamd
