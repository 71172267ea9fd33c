// Test kernels of the device API, written against include/nccl.h + include/nccl_device.h only (libdevapi_kernels.so,
// driven through ctypes by tests/test_gpu_device_api.py). Every launcher enqueues one kernel on `stream` and returns
// the launch's hipError_t; the caller guarantees that offsets and counts lie inside the windows it passes.
#include <hip/hip_runtime.h>

#include "nccl.h"
#include "nccl_device.h"

#define DEVAPI extern "C" __attribute__((visibility("default")))

// ---- LSA AllReduce (sum): acquire-sync; every rank reduces its strided share of the elements from all peers' send
// windows in peer order 0..n-1 and writes the result into every peer's recv window; release-sync. One barrier per CTA.
template <typename T>
__global__ void lsaAllReduceKernel(ncclDevComm dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv, size_t recvOff,
                                   size_t count) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  bar.sync(cta, std::memory_order_acquire);
  const int n = dc.lsaSize;
  const size_t first = ((size_t)blockIdx.x * n + dc.lsaRank) * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * n * blockDim.x;
  for (size_t i = first; i < count; i += step) {
    T acc = ((const T*)ncclGetLsaPointer(send, sendOff, 0))[i];
    for (int p = 1; p < n; p++) acc += ((const T*)ncclGetLsaPointer(send, sendOff, p))[i];
    for (int p = 0; p < n; p++) ((T*)ncclGetLsaPointer(recv, recvOff, p))[i] = acc;
  }
  bar.sync(cta, std::memory_order_release);
}

template <typename T>
static int launchAllReduce(const ncclDevComm* dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv, size_t recvOff,
                           size_t count, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(lsaAllReduceKernel<T>, dim3(grid), dim3(512), 0, stream, *dc, send, sendOff, recv, recvOff, count);
  return (int)hipGetLastError();
}
DEVAPI int lsa_allreduce_u32(const ncclDevComm* dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv,
                             size_t recvOff, size_t count, int grid, hipStream_t stream) {
  return launchAllReduce<uint32_t>(dc, send, sendOff, recv, recvOff, count, grid, stream);
}
DEVAPI int lsa_allreduce_f32(const ncclDevComm* dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv,
                             size_t recvOff, size_t count, int grid, hipStream_t stream) {
  return launchAllReduce<float>(dc, send, sendOff, recv, recvOff, count, grid, stream);
}

// ---- store-based AlltoAll: rank r writes block p of its send window into block r of peer p's recv window.
__global__ void lsaAlltoAllKernel(ncclDevComm dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv, size_t recvOff,
                                  size_t blockBytes) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  bar.sync(cta, std::memory_order_acquire);
  const int n = dc.lsaSize, me = dc.lsaRank;
  const char* src = (const char*)ncclGetLocalPointer(send, sendOff);
  const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  for (int p = 0; p < n; p++) {
    char* dst = (char*)ncclGetLsaPointer(recv, recvOff, p) + (size_t)me * blockBytes;
    for (size_t i = first; i < blockBytes; i += step) dst[i] = src[(size_t)p * blockBytes + i];
  }
  bar.sync(cta, std::memory_order_release);
}
DEVAPI int lsa_alltoall(const ncclDevComm* dc, ncclWindow_t send, size_t sendOff, ncclWindow_t recv, size_t recvOff,
                        size_t blockBytes, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(lsaAlltoAllKernel, dim3(grid), dim3(512), 0, stream, *dc, send, sendOff, recv, recvOff, blockBytes);
  return (int)hipGetLastError();
}

// ---- barrier rounds: `rounds` rounds per unit (a CTA, or a wave in the ncclCoopWarp variant; unit u uses barrier u).
// Round k: store firstRound + k into slot[me][u] of every peer's resource buffer `h` (uint32 [nRanks][units]),
// sync, check that every peer's slot in the own buffer holds that value, sync. The syncs are acq_rel around plain
// slot accesses, or — `relaxed` — memory_order_relaxed (no fence) around system-scope relaxed atomic slot accesses,
// which the barrier's own drain orders before its inbox stores (the resource buffer is uncached memory).
template <typename Coop>
__device__ void barrierRounds(Coop coop, ncclDevComm const& dc, ncclDevResourceHandle h, uint32_t unit, uint32_t units,
                              uint32_t firstRound, int rounds, bool relaxed, unsigned int* mismatches) {
  ncclLsaBarrierSession<Coop> bar(coop, dc, ncclTeamTagLsa(), unit);
  const int n = dc.lsaSize, me = dc.lsaRank, t = coop.thread_rank();
  const uint32_t* mine = (const uint32_t*)ncclGetResourceBufferLocalPointer(dc, h);
  const std::memory_order order = relaxed ? std::memory_order_relaxed : std::memory_order_acq_rel;
  for (int k = 0; k < rounds; k++) {
    const uint32_t round = firstRound + (uint32_t)k;
    if (t < n) {
      uint32_t* slot = (uint32_t*)ncclGetResourceBufferLsaPointer(dc, h, t) + (size_t)me * units + unit;
      if (relaxed) __hip_atomic_store(slot, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else *slot = round;
    }
    bar.sync(coop, order);
    if (t < n) {
      const uint32_t* slot = mine + (size_t)t * units + unit;
      const uint32_t seen = relaxed ? __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *slot;
      if (seen != round) atomicAdd(mismatches, 1u);
    }
    bar.sync(coop, order);
  }
}
__global__ void barrierRoundsCtaKernel(ncclDevComm dc, ncclDevResourceHandle h, uint32_t firstRound, int rounds,
                                       int relaxed, unsigned int* mismatches) {
  barrierRounds(ncclCoopCta(), dc, h, blockIdx.x, gridDim.x, firstRound, rounds, relaxed != 0, mismatches);
}
__global__ void barrierRoundsWarpKernel(ncclDevComm dc, ncclDevResourceHandle h, uint32_t firstRound, int rounds,
                                        int relaxed, unsigned int* mismatches) {
  const uint32_t wavesPerCta = blockDim.x / 64;
  barrierRounds(ncclCoopWarp(), dc, h, blockIdx.x * wavesPerCta + threadIdx.x / 64, gridDim.x * wavesPerCta, firstRound,
                rounds, relaxed != 0, mismatches);
}
// warp != 0: 4 waves per CTA, one barrier each (4 * grid barriers and slots per rank); else 256 threads, one per CTA
DEVAPI int barrier_rounds(const ncclDevComm* dc, ncclDevResourceHandle h, unsigned int firstRound, int rounds,
                          unsigned int* mismatches, int grid, int warp, int relaxed, hipStream_t stream) {
  if (warp)
    hipLaunchKernelGGL(barrierRoundsWarpKernel, dim3(grid), dim3(256), 0, stream, *dc, h, firstRound, rounds, relaxed,
                       mismatches);
  else
    hipLaunchKernelGGL(barrierRoundsCtaKernel, dim3(grid), dim3(256), 0, stream, *dc, h, firstRound, rounds, relaxed,
                       mismatches);
  return (int)hipGetLastError();
}

// ---- resource buffers: buffer `h` of `bytes` bytes is cut into nRanks segments; between two syncs every rank writes
// its stamp into its segment of every peer's buffer, then checks every segment of its own buffer.
__device__ __forceinline__ unsigned char stampOf(int rank, size_t i, unsigned int seed) {
  return (unsigned char)(seed + 31u * (unsigned)rank + 7u * (unsigned)i + (unsigned)(i >> 8));
}
__global__ void resourceStampKernel(ncclDevComm dc, ncclDevResourceHandle h, size_t bytes, unsigned int seed,
                                    unsigned int* mismatches) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  const int n = dc.lsaSize, me = dc.lsaRank;
  const size_t seg = bytes / n;
  const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  bar.sync(cta, std::memory_order_acq_rel);  // nobody still checks an earlier launch's stamps
  for (int p = 0; p < n; p++) {
    unsigned char* dst = (unsigned char*)ncclGetResourceBufferPeerPointer(dc, h, ncclTeamWorld(dc), p) + me * seg;
    for (size_t i = first; i < seg; i += step) dst[i] = stampOf(me, i, seed);
  }
  bar.sync(cta, std::memory_order_acq_rel);
  const unsigned char* mine = (const unsigned char*)ncclGetResourceBufferLocalPointer(dc, h);
  for (int p = 0; p < n; p++)
    for (size_t i = first; i < seg; i += step)
      if (mine[p * seg + i] != stampOf(p, i, seed)) atomicAdd(mismatches, 1u);
}
DEVAPI int resource_stamp(const ncclDevComm* dc, ncclDevResourceHandle h, size_t bytes, unsigned int seed,
                          unsigned int* mismatches, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(resourceStampKernel, dim3(grid), dim3(256), 0, stream, *dc, h, bytes, seed, mismatches);
  return (int)hipGetLastError();
}

// ---- pointer dump: out[0..n) ncclGetLsaPointer, [n..2n) ncclGetPeerPointer(w, off, peer), [2n..3n) its team form
// (world team), [3n] ncclGetLocalPointer, [3n+1..4n+1) ncclGetResourceBufferLsaPointer, [4n+1] ...LocalPointer,
// [4n+2..5n+2) ...PeerPointer (world team), [5n+2] ncclGetResourceBufferOffset(h)
__global__ void pointerDumpKernel(ncclDevComm dc, ncclWindow_t w, size_t off, ncclDevResourceHandle h,
                                  unsigned long long* out) {
  const int n = dc.nRanks;
  const ncclTeam world = ncclTeamWorld(dc);
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    out[p] = (unsigned long long)ncclGetLsaPointer(w, off, p);
    out[n + p] = (unsigned long long)ncclGetPeerPointer(w, off, p);
    out[2 * n + p] = (unsigned long long)ncclGetPeerPointer(w, off, world, p);
    out[3 * n + 1 + p] = (unsigned long long)ncclGetResourceBufferLsaPointer(dc, h, p);
    out[4 * n + 2 + p] = (unsigned long long)ncclGetResourceBufferPeerPointer(dc, h, world, p);
  }
  if (threadIdx.x == 0) {
    out[3 * n] = (unsigned long long)ncclGetLocalPointer(w, off);
    out[4 * n + 1] = (unsigned long long)ncclGetResourceBufferLocalPointer(dc, h);
    out[5 * n + 2] = (unsigned long long)ncclGetResourceBufferOffset(h);
  }
}
DEVAPI int pointer_dump(const ncclDevComm* dc, ncclWindow_t w, size_t off, ncclDevResourceHandle h,
                        unsigned long long* out, hipStream_t stream) {
  hipLaunchKernelGGL(pointerDumpKernel, dim3(1), dim3(64), 0, stream, *dc, w, off, h, out);
  return (int)hipGetLastError();
}

// ---- one sync on barrier 0 by one CTA: timed (its ncclResult_t goes to *out) or untimed (*out = 0 afterwards)
__global__ void oneSyncKernel(ncclDevComm dc, int timed, unsigned long long timeoutCycles, unsigned int* out) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), 0);
  ncclResult_t rc = ncclSuccess;
  if (timed) rc = bar.sync(cta, std::memory_order_acq_rel, timeoutCycles);
  else bar.sync(cta, std::memory_order_acq_rel);
  if (threadIdx.x == 0) *out = (unsigned int)rc;
}
DEVAPI int timed_sync(const ncclDevComm* dc, int timed, unsigned long long timeoutCycles, unsigned int* out,
                      hipStream_t stream) {
  hipLaunchKernelGGL(oneSyncKernel, dim3(1), dim3(64), 0, stream, *dc, timed, timeoutCycles, out);
  return (int)hipGetLastError();
}

DEVAPI int devapi_sizeof_devcomm(void) { return (int)sizeof(ncclDevComm); }
