// kern_gather.hip — instantiation unit of the collective kernels (kernels.h) for one element type.
#include "kernels.h"
namespace ncclamd {
ncclResult_t launchKernGather(const LaunchPlan& p) {
  if (p.func == FUNC_BROADCAST) return launchBcast<>(p);
  switch (p.eltSize) {
    case 1: return launchTyped<uint8_t, 0>(p);
    case 2: return launchTyped<uint16_t, 0>(p);
    case 4: return launchTyped<uint32_t, 0>(p);
    default: return launchTyped<uint64_t, 0>(p);
  }
}
// ncclSend / ncclRecv: bytes, in this unit beside the Broadcast kernels (p2p.cc)
ncclResult_t launchP2pKernel(const ncclComm* comm, const P2pLaunch& l, hipStream_t stream) {
  return launchP2pT<>(comm, l, stream);
}
// ncclPutSignal / ncclSignal / ncclWaitSignal: bytes too (rma.cc)
ncclResult_t launchRmaPutKernel(const ncclComm* comm, const RmaLaunch& l, hipStream_t stream) {
  return launchRmaPutT<>(comm, l, stream);
}
ncclResult_t launchRmaWaitKernel(const ncclComm* comm, const RmaWaitArgs& w, hipStream_t stream) {
  return launchRmaWaitT<>(comm, w, stream);
}
// zero-copy ncclAlltoAll / ncclGather on symmetric windows: bytes as well (enqueue.cc planSymA2A)
ncclResult_t launchSymA2AKernel(const SymPlan& p) { return launchSymA2AT<>(p); }
// Force this code object to load now (see warmKernels in kernels.hip).
hipError_t warmKernGather() {
  hipFuncAttributes attr;
  return hipFuncGetAttributes(&attr, (const void*)&collKernel<uint32_t, 0, COLL_AG>);
}
ncclResult_t launchSymKernGather(const SymPlan& p) {
  switch (p.eltSize) {
    case 1: return launchSymTyped<uint8_t, 0>(p);
    case 2: return launchSymTyped<uint16_t, 0>(p);
    case 4: return launchSymTyped<uint32_t, 0>(p);
    default: return launchSymTyped<uint64_t, 0>(p);
  }
}
}  // namespace ncclamd
