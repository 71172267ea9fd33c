// Test kernels of the device API's reduce-copy family (include/nccl_device_reduce_copy.h), written against the two
// public headers only (libdevapi_rc_kernels.so, driven through ctypes by tests/test_gpu_device_rc.py and
// tests/test_gpu_device_rc_edge.py). Every launcher
// enqueues one kernel on `stream` and returns the launch's hipError_t (or -1 for a code it does not know); the caller
// guarantees that pointers, offsets and counts lie inside the buffers it passes.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "nccl.h"
#include "nccl_device.h"

#define DEVAPI extern "C" __attribute__((visibility("default")))

// the header's P for the default UNROLL
DEVAPI size_t rc_round_elts(size_t eltSize, int coopSize) {
  return ncclReduceCopyRoundElts(eltSize, coopSize, 4 * 16 / (int)eltSize);
}

// ---- local forms, no communicator. One coop of the block calls: thread 0 alone (ncclCoopThread, the rest of its
// wave inactive), the second wave of two (ncclCoopWarp), or all threads (ncclCoopCta: 256, or 72 with a last wave of 8).
//   form 0  ncclLocalReduceSum, lambda (source i is srcTable[i])      -> dstBase
//   form 1  ncclLocalReduceSum, strided (srcBase + i·srcDispl)        -> dstBase
//   form 2  ncclLocalCopy, lambda (destination i is dstTable[i])      <- srcBase
//   form 3  ncclLocalCopy, strided (dstBase + i·dstDispl)             <- srcBase
//   form 4  ncclLocalReduceSumCopy, strided both
template <typename T, typename Coop, typename IntCount>
__device__ __forceinline__ void localForms(Coop coop, int form, T* const* srcTable, T* const* dstTable, T* srcBase,
                                           size_t srcDispl, T* dstBase, size_t dstDispl, int nSrc, int nDst,
                                           IntCount count) {
  if (form == 0)
    ncclLocalReduceSum<T>(coop, [=](int i) -> T* { return srcTable[i]; }, nSrc, dstBase, count);
  else if (form == 1)
    ncclLocalReduceSum<T>(coop, nSrc, srcBase, srcDispl, dstBase, count);
  else if (form == 2)
    ncclLocalCopy<T>(coop, srcBase, [=](int i) -> T* { return dstTable[i]; }, nDst, count);
  else if (form == 3)
    ncclLocalCopy<T>(coop, srcBase, nDst, dstBase, dstDispl, count);
  else
    ncclLocalReduceSumCopy<T>(coop, nSrc, srcBase, srcDispl, nDst, dstBase, dstDispl, count);
}

template <typename T, int COOP, typename IntCount>
__global__ void __launch_bounds__(256) rcLocalKernel(int form, T* const* srcTable, T* const* dstTable, T* srcBase,
                                                     size_t srcDispl, T* dstBase, size_t dstDispl, int nSrc, int nDst,
                                                     size_t count) {
  if (COOP == 0) {
    if (threadIdx.x == 0)
      localForms<T>(ncclCoopThread(), form, srcTable, dstTable, srcBase, srcDispl, dstBase, dstDispl, nSrc, nDst,
                    (IntCount)count);
  } else if (COOP == 1) {
    if (threadIdx.x / 64 == 1)
      localForms<T>(ncclCoopWarp(), form, srcTable, dstTable, srcBase, srcDispl, dstBase, dstDispl, nSrc, nDst,
                    (IntCount)count);
  } else {
    localForms<T>(ncclCoopCta(), form, srcTable, dstTable, srcBase, srcDispl, dstBase, dstDispl, nSrc, nDst,
                  (IntCount)count);
  }
}

template <typename T, int COOP, typename IntCount>
static int launchLocal(int oddCta, int form, void* const* srcTable, void* const* dstTable, void* srcBase, size_t srcDispl,
                       void* dstBase, size_t dstDispl, int nSrc, int nDst, size_t count, hipStream_t stream) {
  const int threads = COOP == 0 ? 64 : (COOP == 1 ? 128 : (oddCta ? 72 : 256));
  hipLaunchKernelGGL((rcLocalKernel<T, COOP, IntCount>), dim3(1), dim3(threads), 0, stream, form, (T* const*)srcTable,
                     (T* const*)dstTable, (T*)srcBase, srcDispl, (T*)dstBase, dstDispl, nSrc, nDst, count);
  return (int)hipGetLastError();
}

template <typename T>
static int launchLocalT(int coop, int wideCount, int form, void* const* srcTable, void* const* dstTable, void* srcBase,
                        size_t srcDispl, void* dstBase, size_t dstDispl, int nSrc, int nDst, size_t count,
                        hipStream_t stream) {
#define RC_GO(C, I) \
  return launchLocal<T, C, I>(coop == 3, form, srcTable, dstTable, srcBase, srcDispl, dstBase, dstDispl, nSrc, nDst, count, stream)
  switch (coop * 2 + (wideCount ? 1 : 0)) {
    case 0: RC_GO(0, int);
    case 1: RC_GO(0, size_t);
    case 2: RC_GO(1, int);
    case 3: RC_GO(1, size_t);
    case 4: RC_GO(2, int);
    case 5: RC_GO(2, size_t);
    case 6: RC_GO(2, int); /* coop 3: the CTA kernels with 72 threads, a last wave of 8 */
    case 7: RC_GO(2, size_t);
  }
#undef RC_GO
  return -1;
}

// type: 0 int8, 1 uint8, 2 int32, 3 uint32, 4 int64, 5 uint64, 6 float, 7 double, 8 __half, 9 __hip_bfloat16
// coop: 0 thread, 1 warp, 2 CTA of 256 threads, 3 CTA of 72 threads; wideCount: IntCount is size_t (else int)
DEVAPI int rc_local(int type, int coop, int wideCount, int form, void* const* srcTable, void* const* dstTable,
                    void* srcBase, size_t srcDispl, void* dstBase, size_t dstDispl, int nSrc, int nDst, size_t count,
                    hipStream_t stream) {
#define RC_T(T) \
  return launchLocalT<T>(coop, wideCount, form, srcTable, dstTable, srcBase, srcDispl, dstBase, dstDispl, nSrc, nDst, \
                         count, stream)
  switch (type) {
    case 0: RC_T(int8_t);
    case 1: RC_T(uint8_t);
    case 2: RC_T(int32_t);
    case 3: RC_T(uint32_t);
    case 4: RC_T(int64_t);
    case 5: RC_T(uint64_t);
    case 6: RC_T(float);
    case 7: RC_T(double);
    case 8: RC_T(__half);
    case 9: RC_T(__hip_bfloat16);
  }
#undef RC_T
  return -1;
}

// ---- user RedOps: ncclLsaReduceLsaCopy, sources and destinations from pointer tables, one CTA. OpMax is a select;
// OpUserSum is a + b in T and is not nccl::utility::OpSum, so __half and __hip_bfloat16 fold in T, rounding every step.
template <typename T>
struct OpMax {
  using EltType = T;
  __device__ T operator()(T const& a, T const& b) const { return a < b ? b : a; }
};
template <typename T>
struct OpUserSum {
  using EltType = T;
  __device__ T operator()(T const& a, T const& b) const { return a + b; }
};
template <typename T, typename RedOp>
__global__ void __launch_bounds__(256) rcUserOpKernel(T* const* srcTable, int nSrc, T* const* dstTable, int nDst,
                                                      size_t count) {
  ncclLsaReduceLsaCopy<T>(ncclCoopCta(), [=](int i) -> T* { return srcTable[i]; }, nSrc,
                          [=](int i) -> T* { return dstTable[i]; }, nDst, RedOp{}, count);
}
template <typename T, typename RedOp>
static int launchUserOp(void* const* srcTable, int nSrc, void* const* dstTable, int nDst, size_t count,
                        hipStream_t stream) {
  hipLaunchKernelGGL((rcUserOpKernel<T, RedOp>), dim3(1), dim3(256), 0, stream, (T* const*)srcTable, nSrc,
                     (T* const*)dstTable, nDst, count);
  return (int)hipGetLastError();
}
// type: 2 int32, 6 float, 7 double, 8 __half, 9 __hip_bfloat16
DEVAPI int rc_max(int type, void* const* srcTable, int nSrc, void* const* dstTable, int nDst, size_t count,
                  hipStream_t stream) {
  switch (type) {
    case 2: return launchUserOp<int32_t, OpMax<int32_t>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 6: return launchUserOp<float, OpMax<float>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 7: return launchUserOp<double, OpMax<double>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 8: return launchUserOp<__half, OpMax<__half>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 9: return launchUserOp<__hip_bfloat16, OpMax<__hip_bfloat16>>(srcTable, nSrc, dstTable, nDst, count, stream);
  }
  return -1;
}
// type: 6 float, 7 double, 8 __half, 9 __hip_bfloat16
DEVAPI int rc_usersum(int type, void* const* srcTable, int nSrc, void* const* dstTable, int nDst, size_t count,
                      hipStream_t stream) {
  switch (type) {
    case 6: return launchUserOp<float, OpUserSum<float>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 7: return launchUserOp<double, OpUserSum<double>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 8: return launchUserOp<__half, OpUserSum<__half>>(srcTable, nSrc, dstTable, nDst, count, stream);
    case 9:
      return launchUserOp<__hip_bfloat16, OpUserSum<__hip_bfloat16>>(srcTable, nSrc, dstTable, nDst, count, stream);
  }
  return -1;
}

// ---- LSA forms across ranks. One kernel per case: acquire-sync, the call under test on this CTA's contiguous slice,
// release-sync. One barrier per CTA. `send` / `recv` are symmetric windows, the payloads at sendOff / recvOff.
//   forms 0-4   ncclLsaReduceSum: every rank sums all ranks' send payloads into its own recv payload
//               (0 lambda, 1 ncclSymPtr + team, 2 ncclSymPtr + devComm, 3 window + team, 4 window + devComm)
//   forms 5-9   ncclLsaCopy: every rank copies its send payload into block `rank` of every rank's recv payload
//               (an AllGather; 5 lambda, 6-9 as above)
//   forms 10-13 ncclLsaReduceSumCopy, one team: the AllReduce; rank r reduces part r of the elements from all ranks'
//               send payloads into all ranks' recv payloads (10 ncclSymPtr + team, 11 + devComm, 12 windows + team,
//               13 windows + devComm). send == recv with equal offsets is the in-place case.
//   form 14     ncclLsaReduceSumCopy, two teams: sources are this rank's run of `inner` consecutive ranks, destinations
//               the world: part r of every rank's recv payload is the sum over r's run
//   form 15     ncclLsaReduceSumLsaCopy (lambdas), the AllReduce of forms 10-13
struct Slice {
  size_t start, len;
};
__device__ __forceinline__ Slice sliceOf(size_t count, size_t unit, size_t units) {
  const size_t per = (count + units - 1) / units;
  Slice s;
  s.start = unit * per < count ? unit * per : count;
  s.len = count - s.start < per ? count - s.start : per;
  return s;
}

template <typename T>
__global__ void __launch_bounds__(256) rcLsaKernel(ncclDevComm dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv,
                                                   size_t recvOff, size_t count, int form, int inner) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  bar.sync(cta, std::memory_order_acquire);
  const int n = dc.lsaSize, me = dc.lsaRank;
  const ncclTeam world = ncclTeamWorld(dc);
  if (form < 5) {
    const Slice s = sliceOf(count, blockIdx.x, gridDim.x);
    T* dst = (T*)ncclGetLocalPointer(recv, recvOff) + s.start;
    const ncclSymPtr<T> src = ncclSymPtr<T>(send, sendOff) + s.start;
    if (form == 0)
      ncclLsaReduceSum<T>(cta, [=](int i) -> T* { return (T*)ncclGetLsaPointer(send, sendOff, i) + s.start; }, n, dst,
                          s.len);
    else if (form == 1) ncclLsaReduceSum<T>(cta, src, dst, s.len, world);
    else if (form == 2) ncclLsaReduceSum<T>(cta, src, dst, s.len, dc);
    else if (form == 3) ncclLsaReduceSum<T>(cta, src.window, src.offset, dst, s.len, world);
    else ncclLsaReduceSum<T>(cta, src.window, src.offset, dst, s.len, dc);
  } else if (form < 10) {
    const Slice s = sliceOf(count, blockIdx.x, gridDim.x);
    T* src = (T*)ncclGetLocalPointer(send, sendOff) + s.start;
    const size_t block = (size_t)me * count + s.start; /* in elements, from recvOff */
    const ncclSymPtr<T> dst = ncclSymPtr<T>(recv, recvOff) + block;
    if (form == 5)
      ncclLsaCopy<T>(cta, src, [=](int i) -> T* { return (T*)ncclGetLsaPointer(recv, recvOff, i) + block; }, n, s.len);
    else if (form == 6) ncclLsaCopy<T>(cta, src, dst, s.len, world);
    else if (form == 7) ncclLsaCopy<T>(cta, src, dst, s.len, dc);
    else if (form == 8) ncclLsaCopy<T>(cta, src, dst.window, dst.offset, s.len, world);
    else ncclLsaCopy<T>(cta, src, dst.window, dst.offset, s.len, dc);
  } else {
    const Slice s = sliceOf(count, (size_t)me * gridDim.x + blockIdx.x, (size_t)n * gridDim.x);
    const ncclSymPtr<T> src = ncclSymPtr<T>(send, sendOff) + s.start;
    const ncclSymPtr<T> dst = ncclSymPtr<T>(recv, recvOff) + s.start;
    if (form == 10) ncclLsaReduceSumCopy<T>(cta, src, dst, s.len, world);
    else if (form == 11) ncclLsaReduceSumCopy<T>(cta, src, dst, s.len, dc);
    else if (form == 12) ncclLsaReduceSumCopy<T>(cta, src.window, src.offset, dst.window, dst.offset, s.len, world);
    else if (form == 13) ncclLsaReduceSumCopy<T>(cta, src.window, src.offset, dst.window, dst.offset, s.len, dc);
    else if (form == 14) ncclLsaReduceSumCopy<T>(cta, src, ncclTeamInnerFactor(world, inner), dst, world, s.len);
    else
      ncclLsaReduceSumLsaCopy<T>(cta, [=](int i) -> T* { return src.lsaPtr(i); }, n,
                                 [=](int i) -> T* { return dst.lsaPtr(i); }, n, s.len);
  }
  bar.sync(cta, std::memory_order_release);
}

// type: 3 uint32, 6 float, 8 __half, 9 __hip_bfloat16
DEVAPI int rc_lsa(int type, const ncclDevComm* dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv, size_t recvOff,
                  size_t count, int form, int inner, int grid, hipStream_t stream) {
#define RC_T(T)                                                                                                    \
  hipLaunchKernelGGL(rcLsaKernel<T>, dim3(grid), dim3(256), 0, stream, *dc, send, sendOff, recv, recvOff, count, form, \
                     inner);                                                                                       \
  return (int)hipGetLastError()
  switch (type) {
    case 3: RC_T(uint32_t);
    case 6: RC_T(float);
    case 8: RC_T(__half);
    case 9: RC_T(__hip_bfloat16);
  }
#undef RC_T
  return -1;
}
