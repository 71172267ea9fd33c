// Test kernels of ncclLLA2ASession, written against include/nccl.h + include/nccl_device.h only
// (libdevapi_lla2a_kernels.so, driven through ctypes by tests/test_gpu_device_lla2a.py). Every launcher enqueues one
// kernel on `stream` and returns the launch's hipError_t; the caller guarantees that the handle's buffer holds the
// blocks and slots it names and that `out` holds what the kernel writes.
#include <hip/hip_runtime.h>

#include "nccl.h"
#include "nccl_device.h"

#define DEVAPI extern "C" __attribute__((visibility("default")))

template <int W>
struct Words {
  uint32_t w[W];
};

// ---- exchange: for `epochs` rounds every member sends m values of W words to every peer (itself included) into slot
// from * m + j, receives all n * m slots into out[blockIdx][round][slot][W], and ends the epoch. The coop's threads
// share the sends and the receives; session block = blockIdx.x. Word k (= 2 * piece + half) of element j that rank
// `from` sends to rank `to` in round seq on grid block b is b<<31 | from<<27 | to<<23 | (seq&255)<<15 | j<<8 | k.
template <typename Coop, int W>
__global__ void __launch_bounds__(128) exchangeKernel(ncclDevComm dc, ncclLLA2AHandle h, int m, int epochs, uint32_t seq,
                                                      uint32_t* out) {
  Coop coop;
  const int n = dc.lsaSize, slots = n * m;
  const uint32_t mine = blockIdx.x << 31 | (uint32_t)dc.lsaRank << 27;
  out += (size_t)blockIdx.x * epochs * slots * W;
  ncclLLA2ASession<Coop> a2a(coop, dc, ncclTeamLsa(dc), h, blockIdx.x, slots);
  for (int e = 0; e < epochs; e++) {
    for (int i = coop.thread_rank(); i < slots; i += coop.size()) {
      const int to = i / m, j = i % m;
      Words<W> v;
      for (int k = 0; k < W; k++) v.w[k] = mine | to << 23 | ((seq + e) & 0xff) << 15 | j << 8 | k;
      a2a.send(to, dc.lsaRank * m + j, v);
    }
    for (int i = coop.thread_rank(); i < slots; i += coop.size()) {
      const Words<W> v = a2a.template recv<Words<W>>(i);
      for (int k = 0; k < W; k++) out[((size_t)e * slots + i) * W + k] = v.w[k];
    }
    a2a.endEpoch(coop);
  }
}

// coop: 0 thread, 1 wave, 2 CTA of 128; words: 1, 2, 3, 4 or 6 (4 to 24 bytes); grid 2
DEVAPI int lla2a_exchange(const ncclDevComm* dc, unsigned bufHandle, unsigned nSlots, int coop, int words, int m,
                          int epochs, unsigned seq, uint32_t* out, hipStream_t stream) {
  const ncclLLA2AHandle h = {bufHandle, nSlots};
#define EXCHANGE(W)                                                                                                   \
  case W:                                                                                                             \
    if (coop == 0) hipLaunchKernelGGL((exchangeKernel<ncclCoopThread, W>), 2, 1, 0, stream, *dc, h, m, epochs, seq, out); \
    if (coop == 1) hipLaunchKernelGGL((exchangeKernel<ncclCoopWarp, W>), 2, 64, 0, stream, *dc, h, m, epochs, seq, out);  \
    if (coop == 2) hipLaunchKernelGGL((exchangeKernel<ncclCoopCta, W>), 2, 128, 0, stream, *dc, h, m, epochs, seq, out);  \
    break;
  switch (words) {
    EXCHANGE(1) EXCHANGE(2) EXCHANGE(3) EXCHANGE(4) EXCHANGE(6)
    default: return (int)hipErrorInvalidValue;
  }
#undef EXCHANGE
  return (int)hipGetLastError();
}

// ---- fused small AllReduce (sum), the reference's "all-gather over LL, reduce locally" shape: thread i < k bcasts
// in[i] to slot rank * k + i and folds slots i, i + k, ... (ranks 0 .. n-1, in that order) with recvReduce<4>.
// Grid block b works on elements [b * k, (b + 1) * k) with session block b; k <= 512.
template <typename T>
__global__ void __launch_bounds__(512) allReduceKernel(ncclDevComm dc, ncclLLA2AHandle h, const T* in, T* out, int k) {
  ncclCoopCta cta;
  const int n = dc.lsaSize, i = threadIdx.x;
  ncclLLA2ASession<ncclCoopCta> a2a(cta, dc, ncclTeamLsa(dc), h, blockIdx.x, n * k);
  if (i < k) {
    a2a.bcast(dc.lsaRank * k + i, in[(size_t)blockIdx.x * k + i]);
    out[(size_t)blockIdx.x * k + i] =
        a2a.template recvReduce<4, T>(i, n, k, [](T x) { return x; }, [](T a, T b) { return a + b; });
  }
  a2a.endEpoch(cta);
}
DEVAPI int lla2a_allreduce(const ncclDevComm* dc, unsigned bufHandle, unsigned nSlots, int f64, const void* in, void* out,
                           int k, int grid, hipStream_t stream) {
  const ncclLLA2AHandle h = {bufHandle, nSlots};
  const dim3 threads((k + 63) / 64 * 64);
  if (k < 1 || k > 512) return (int)hipErrorInvalidValue;
  if (f64) hipLaunchKernelGGL(allReduceKernel<double>, grid, threads, 0, stream, *dc, h, (const double*)in, (double*)out, k);
  else hipLaunchKernelGGL(allReduceKernel<float>, grid, threads, 0, stream, *dc, h, (const float*)in, (float*)out, k);
  return (int)hipGetLastError();
}

// ---- helper on this rank's own lines of session block `block`. fill != 0: set the stored epoch word to `stored` and
// fill every slot of the even parity with {payload, flagEven, payload, flagEven}, of the odd parity with flagOdd.
// Always: *word = the block's stored epoch word afterwards.
__global__ void blockKernel(ncclDevComm dc, ncclLLA2AHandle h, uint32_t block, int fill, uint32_t stored,
                            uint32_t flagEven, uint32_t flagOdd, uint32_t payload, uint32_t* word) {
  uint4* line = (uint4*)ncclGetResourceBufferLocalPointer(dc, h.bufHandle) + (size_t)block * (1 + 2 * h.nSlots);
  for (uint32_t i = threadIdx.x; fill && i < 2 * h.nSlots; i += blockDim.x) {
    const uint32_t flag = i < h.nSlots ? flagEven : flagOdd;
    line[1 + i] = uint4{payload, flag, payload, flag};
  }
  if (threadIdx.x == 0) {
    if (fill) line[0].x = stored;
    *word = line[0].x;
  }
}
DEVAPI int lla2a_block(const ncclDevComm* dc, unsigned bufHandle, unsigned nSlots, unsigned block, int fill,
                       unsigned stored, unsigned flagEven, unsigned flagOdd, unsigned payload, uint32_t* word,
                       hipStream_t stream) {
  const ncclLLA2AHandle h = {bufHandle, nSlots};
  hipLaunchKernelGGL(blockKernel, 1, 256, 0, stream, *dc, h, block, fill, stored, flagEven, flagOdd, payload, word);
  return (int)hipGetLastError();
}
