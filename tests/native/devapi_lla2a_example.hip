// ncclLLA2ASession against the C ABI: a fused small AllReduce (sum of floats) in ONE kernel of the caller's own, the
// reference's "all-gather over LL, reduce locally" shape. Thread i of a CTA broadcasts its element into slot
// rank * k + i of every rank's line area and folds the n values of slots i, i + k, ... in rank order; no barrier, no
// fence, no window of the caller's: the values travel inside flagged 16-byte lines of a DevComm resource buffer.
//
//   devapi_lla2a_example N          one pthread per rank (a forked process per rank above 4 ranks: a process has 4
//                                   hardware queues by default, and ranks that spin on each other need one each);
//                                   2 CTAs of 150 elements, 3 rounds in one kernel and a second launch; prints OK
//                                   when every element is the sum over the ranks
//   devapi_lla2a_example N bench    one forked process per rank; prints timings instead (profiles/README.md): per
//       round inside a running kernel (20 kernels of 1000 rounds) and per launch of a one-round kernel (200 launches),
//       at 8 bytes and 1 KiB; beside them one LSA barrier sync(acq_rel) round and ncclAllReduce of the same bytes.
// Ranks beyond the device count share devices (NCCL_MULTI_RANK_GPU_ENABLE is set for that); every rank's kernels run
// on a stream with a hardware queue of its own, since the ranks spin on each other.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <vector>

#include "nccl.h"
#include "nccl_device.h"

#define HIPCK(call)                                                                           \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));  \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)
#define NCCLCK(call)                                                                          \
  do {                                                                                        \
    ncclResult_t r_ = (call);                                                                 \
    if (r_ != ncclSuccess) {                                                                  \
      fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, ncclGetErrorString(r_)); \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)

constexpr int kCtas = 2, kMaxK = 256;  // session blocks (one per CTA) and elements per CTA the line area is sized for

// CTA b reduces elements [b * k, (b + 1) * k), `rounds` times over (each round is one epoch of its session block).
// Round r contributes in[i] + bias + r, so no two rounds carry the same values.
__global__ void __launch_bounds__(512) fusedAllReduceKernel(ncclDevComm dc, ncclLLA2AHandle handle, const float* in,
                                                            float* out, int k, int rounds, float bias) {
  ncclCoopCta cta;
  const int n = dc.lsaSize, i = threadIdx.x;
  ncclLLA2ASession<ncclCoopCta> a2a(cta, dc, ncclTeamLsa(dc), handle, blockIdx.x, /*maxElts=*/n * k);
  for (int r = 0; r < rounds; r++) {
    if (i < k) {
      a2a.bcast(dc.lsaRank * k + i, in[blockIdx.x * k + i] + bias + (float)r);
      out[blockIdx.x * k + i] = a2a.template recvReduce</*Unroll=*/4, float>(
          /*eltStart=*/i, /*eltCount=*/n, /*eltStride=*/k, [](float x) { return x; },
          [](float a, float b) { return a + b; });
    }
    a2a.endEpoch(cta);  // every peer was sent a line and a slot of every peer was received: the contract holds
  }
}

__global__ void barrierLoopKernel(ncclDevComm dc, int rounds) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), 0);
  for (int k = 0; k < rounds; k++) bar.sync(cta, std::memory_order_acq_rel);
}

static int run(int rank, int n, ncclUniqueId id, bool bench) {
  int ndev = 0;
  HIPCK(hipGetDeviceCount(&ndev));
  const int dev = rank % ndev;
  HIPCK(hipSetDevice(dev));
  int ncu = 0;
  HIPCK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  for (int cu = 0; cu < ncu; cu++) mask[cu / 32] |= 1u << (cu % 32);
  hipStream_t stream;
  HIPCK(hipExtStreamCreateWithCUMask(&stream, (uint32_t)mask.size(), mask.data()));

  ncclComm_t comm;
  NCCLCK(ncclCommInitRank(&comm, n, id, rank));

  // Buffers first: once the DevComm exists a peer's kernel may be spinning on this rank, and a call that waits for
  // the whole device or runs on the null stream (which waits for every stream of the process, the other ranks'
  // included, when ranks are threads) would wait for that kernel while it waits for this rank's. From then on
  // everything is ordered on this rank's own stream.
  const int count = kCtas * kMaxK;
  float *in, *out, *host;
  HIPCK(hipMalloc((void**)&in, count * sizeof(float)));
  HIPCK(hipMalloc((void**)&out, count * sizeof(float)));
  HIPCK(hipHostMalloc((void**)&host, count * sizeof(float), hipHostMallocDefault));
  for (int i = 0; i < count; i++) host[i] = (float)(1000 * rank + i);
  HIPCK(hipMemcpyAsync(in, host, count * sizeof(float), hipMemcpyHostToDevice, stream));
  HIPCK(hipStreamSynchronize(stream));

  // the line area: kCtas blocks of slots for n * kMaxK floats, asked for through the resource requirement list
  ncclLLA2AHandle_t handle;
  ncclDevResourceRequirements_t lines;
  NCCLCK(ncclLLA2ACreateRequirement(kCtas, ncclLLA2ACalcSlots(n * kMaxK, sizeof(float)), &handle, &lines));
  ncclDevCommRequirements_t reqs = NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER;
  reqs.lsaBarrierCount = 1;
  reqs.resourceRequirementsList = &lines;
  ncclDevComm devComm;
  NCCLCK(ncclDevCommCreate(comm, &reqs, &devComm));

  int rc = 0;
  const int k = 150;
  for (int launch = 0; launch < 2 && !rc; launch++) {  // the second launch continues the first one's epochs
    const int rounds = 3;
    const float bias = (float)(10 * launch);
    hipLaunchKernelGGL(fusedAllReduceKernel, dim3(kCtas), dim3(192), 0, stream, devComm, handle, in, out, k, rounds, bias);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(host, out, count * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    for (int i = 0; i < kCtas * k && !rc; i++) {  // what the last round left
      const float want = (float)(1000 * (n * (n - 1) / 2) + n * i) + (float)n * (bias + (float)(rounds - 1));
      if (host[i] != want) {
        fprintf(stderr, "rank %d launch %d: element %d is %g, expected %g\n", rank, launch, i, host[i], want);
        rc = 1;
      }
    }
  }
  ncclResult_t async = ncclSuccess;
  NCCLCK(ncclCommGetAsyncError(comm, &async));
  if (async != ncclSuccess) {
    fprintf(stderr, "rank %d: async error %s\n", rank, ncclGetErrorString(async));
    rc = 1;
  }

  if (bench && !rc) {
    hipEvent_t e0, e1;
    HIPCK(hipEventCreate(&e0));
    HIPCK(hipEventCreate(&e1));
    float ms = 0.f;
    const int rounds = 1000, launches = 20, iters = 200, warm = 20;
    // (a) one LSA barrier round trip
    hipLaunchKernelGGL(barrierLoopKernel, dim3(1), dim3(512), 0, stream, devComm, 100);
    HIPCK(hipEventRecord(e0, stream));
    for (int i = 0; i < launches; i++) hipLaunchKernelGGL(barrierLoopKernel, dim3(1), dim3(512), 0, stream, devComm, rounds);
    HIPCK(hipEventRecord(e1, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    const double barrierUs = ms * 1e3 / ((double)rounds * launches);
    // (b) the fused AllReduce, 1 CTA: per round inside a running kernel, per launch of a one-round kernel; and
    // (c) ncclAllReduce of the same bytes
    const int ks[2] = {2, kMaxK};  // 8 bytes, 1 KiB
    double roundUs[2], launchUs[2], libUs[2];
    for (int c = 0; c < 2; c++) {
      const dim3 threads((ks[c] + 63) / 64 * 64);
      hipLaunchKernelGGL(fusedAllReduceKernel, dim3(1), threads, 0, stream, devComm, handle, in, out, ks[c], 100, 0.f);
      HIPCK(hipEventRecord(e0, stream));
      for (int i = 0; i < launches; i++)
        hipLaunchKernelGGL(fusedAllReduceKernel, dim3(1), threads, 0, stream, devComm, handle, in, out, ks[c], rounds, 0.f);
      HIPCK(hipEventRecord(e1, stream));
      HIPCK(hipStreamSynchronize(stream));
      HIPCK(hipEventElapsedTime(&ms, e0, e1));
      roundUs[c] = ms * 1e3 / ((double)rounds * launches);
      for (int i = 0; i < warm + iters; i++) {
        if (i == warm) HIPCK(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(fusedAllReduceKernel, dim3(1), threads, 0, stream, devComm, handle, in, out, ks[c], 1, 0.f);
      }
      HIPCK(hipEventRecord(e1, stream));
      HIPCK(hipStreamSynchronize(stream));
      HIPCK(hipEventElapsedTime(&ms, e0, e1));
      launchUs[c] = ms * 1e3 / iters;
      for (int i = 0; i < warm + iters; i++) {
        if (i == warm) HIPCK(hipEventRecord(e0, stream));
        NCCLCK(ncclAllReduce(in, out, ks[c], ncclFloat32, ncclSum, comm, stream));
      }
      HIPCK(hipEventRecord(e1, stream));
      HIPCK(hipStreamSynchronize(stream));
      HIPCK(hipEventElapsedTime(&ms, e0, e1));
      libUs[c] = ms * 1e3 / iters;
    }
    NCCLCK(ncclCommGetAsyncError(comm, &async));
    if (async != ncclSuccess) rc = 1;
    if (rank == 0)
      printf("devapi_lla2a n=%d ranks_share_one_gpu=%d async_error=%d lsa_barrier_sync_us=%.2f "
             "lla2a_allreduce_8B_round_us=%.2f lla2a_allreduce_1KiB_round_us=%.2f lla2a_allreduce_8B_launch_us=%.2f "
             "lla2a_allreduce_1KiB_launch_us=%.2f nccl_allreduce_8B_us=%.2f nccl_allreduce_1KiB_us=%.2f\n",
             n, n > ndev ? 1 : 0, (int)async, barrierUs, roundUs[0], roundUs[1], launchUs[0], launchUs[1], libUs[0],
             libUs[1]);
    fflush(stdout);  // (a forked rank leaves through _exit)
    HIPCK(hipEventDestroy(e0));
    HIPCK(hipEventDestroy(e1));
  }

  NCCLCK(ncclDevCommDestroy(comm, &devComm));
  NCCLCK(ncclCommFinalize(comm));
  NCCLCK(ncclCommDestroy(comm));
  HIPCK(hipFree(in));
  HIPCK(hipFree(out));
  HIPCK(hipHostFree(host));
  HIPCK(hipStreamDestroy(stream));
  return rc;
}

struct ThreadArg {
  int rank, n, rc;
  ncclUniqueId id;
};
static void* threadMain(void* p) {
  ThreadArg* a = (ThreadArg*)p;
  a->rc = run(a->rank, a->n, a->id, false);
  return nullptr;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 2;
  const bool bench = argc > 2 && !strcmp(argv[2], "bench");
  if (n < 1 || n > 16) {
    fprintf(stderr, "usage: %s NRANKS(1..16) [bench]\n", argv[0]);
    return 2;
  }
  setenv("NCCL_MULTI_RANK_GPU_ENABLE", "1", 0);
  ncclUniqueId id;
  NCCLCK(ncclGetUniqueId(&id));  // (no HIP call yet: the ranks' processes are forked before the runtime starts)
  int failed = 0;
  if (bench || n > 4) {
    std::vector<pid_t> kids;
    for (int r = 0; r < n; r++) {
      const pid_t pid = fork();
      if (pid == 0) _exit(run(r, n, id, bench));
      kids.push_back(pid);
    }
    for (pid_t pid : kids) {
      int st = 0;
      if (waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) failed++;
    }
  } else {
    std::vector<pthread_t> th(n);
    std::vector<ThreadArg> args(n);
    for (int r = 0; r < n; r++) {
      args[r] = {r, n, 1, id};
      pthread_create(&th[r], nullptr, threadMain, &args[r]);
    }
    for (int r = 0; r < n; r++) {
      pthread_join(th[r], nullptr);
      failed += args[r].rc != 0;
    }
  }
  if (failed) {
    fprintf(stderr, "FAILED: %d rank(s)\n", failed);
    return 1;
  }
  if (!bench) printf("OK n=%d: every element is the sum over the ranks\n", n);
  return 0;
}
