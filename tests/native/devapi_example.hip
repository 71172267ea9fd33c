// The device API against the C ABI: an AllReduce kernel of the caller's own over LSA windows — the shape of the
// reference's docs/examples/06_device_api/01_allreduce_lsa, restated. Every rank registers a send and a recv window,
// creates a DevComm with one LSA barrier per CTA, and launches the kernel on a stream with a hardware queue of its own
// (ranks that share a GPU spin on each other: their kernels must run concurrently).
//
//   devapi_example N            one pthread per rank; prints OK when every element equals N(N-1)/2
//   devapi_example N procs      the same with one forked process per rank
//   devapi_example N bench      forked processes; prints timings instead (profiles/README.md):
//       the LSA barrier round trip (sync(acq_rel), 1 CTA, 20 kernels of 1000 rounds), the LSA AllReduce kernel and
//       ncclAllReduce on the same windows at 2^20 floats (200 launches each), and ncclAllReduce of 8 bytes (the
//       library's LL latency).
// Ranks beyond the device count share devices (NCCL_MULTI_RANK_GPU_ENABLE is set for that).
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

constexpr int kCtas = 4, kThreads = 512;

__global__ void allReduceKernel(ncclDevComm dc, ncclWindow_t send, ncclWindow_t recv, size_t count) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  bar.sync(cta, std::memory_order_acquire);  // every peer's kernel runs: its input is complete
  const int n = dc.lsaSize;
  const size_t first = ((size_t)blockIdx.x * n + dc.lsaRank) * blockDim.x + threadIdx.x;
  for (size_t i = first; i < count; i += (size_t)gridDim.x * n * blockDim.x) {
    float v = 0.f;
    for (int p = 0; p < n; p++) v += ((const float*)ncclGetLsaPointer(send, 0, p))[i];
    for (int p = 0; p < n; p++) ((float*)ncclGetLsaPointer(recv, 0, p))[i] = v;
  }
  bar.sync(cta, std::memory_order_release);  // every peer has written its share into this rank's recv window
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
  ncclCommProperties_t props = NCCL_COMM_PROPERTIES_INITIALIZER;
  NCCLCK(ncclCommQueryProperties(comm, &props));
  if (!props.deviceApiSupport || props.nRanks != n || props.rank != rank) {
    fprintf(stderr, "rank %d: unexpected communicator properties\n", rank);
    return 1;
  }

  const size_t count = bench ? (size_t)1 << 20 : 100003;
  float *send, *recv;
  NCCLCK(ncclMemAlloc((void**)&send, count * sizeof(float)));
  NCCLCK(ncclMemAlloc((void**)&recv, count * sizeof(float)));
  std::vector<float> host(count, (float)rank);
  HIPCK(hipMemcpy(send, host.data(), count * sizeof(float), hipMemcpyHostToDevice));
  HIPCK(hipMemset(recv, 0xff, count * sizeof(float)));
  ncclWindow_t sendWin, recvWin;
  NCCLCK(ncclCommWindowRegister(comm, send, count * sizeof(float), &sendWin, NCCL_WIN_COLL_SYMMETRIC));
  NCCLCK(ncclCommWindowRegister(comm, recv, count * sizeof(float), &recvWin, NCCL_WIN_COLL_SYMMETRIC));

  ncclDevCommRequirements_t reqs = NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER;
  reqs.lsaBarrierCount = kCtas;
  ncclDevComm devComm;
  NCCLCK(ncclDevCommCreate(comm, &reqs, &devComm));

  int rc = 0;
  hipLaunchKernelGGL(allReduceKernel, dim3(kCtas), dim3(kThreads), 0, stream, devComm, sendWin, recvWin, count);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipMemcpy(host.data(), recv, count * sizeof(float), hipMemcpyDeviceToHost));
  const float want = (float)(n * (n - 1) / 2);
  for (size_t i = 0; i < count && !rc; i++)
    if (host[i] != want) {
      fprintf(stderr, "rank %d: element %zu is %g, expected %g\n", rank, i, host[i], want);
      rc = 1;
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
    // (a) barrier round trip
    hipLaunchKernelGGL(barrierLoopKernel, dim3(1), dim3(kThreads), 0, stream, devComm, 100);
    HIPCK(hipEventRecord(e0, stream));
    for (int i = 0; i < launches; i++)
      hipLaunchKernelGGL(barrierLoopKernel, dim3(1), dim3(kThreads), 0, stream, devComm, rounds);
    HIPCK(hipEventRecord(e1, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    const double barrierUs = ms * 1e3 / ((double)rounds * launches);
    // (b) the LSA AllReduce kernel and ncclAllReduce on the same windows, 2^20 floats
    for (int i = 0; i < warm + iters; i++) {
      if (i == warm) HIPCK(hipEventRecord(e0, stream));
      hipLaunchKernelGGL(allReduceKernel, dim3(kCtas), dim3(kThreads), 0, stream, devComm, sendWin, recvWin, count);
    }
    HIPCK(hipEventRecord(e1, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    const double lsaUs = ms * 1e3 / iters;
    double libUs[2];
    const size_t counts[2] = {count, 2};  // 2 floats = 8 bytes: the LL protocol
    for (int c = 0; c < 2; c++) {
      for (int i = 0; i < warm + iters; i++) {
        if (i == warm) HIPCK(hipEventRecord(e0, stream));
        NCCLCK(ncclAllReduce(send, recv, counts[c], ncclFloat32, ncclSum, comm, stream));
      }
      HIPCK(hipEventRecord(e1, stream));
      HIPCK(hipStreamSynchronize(stream));
      HIPCK(hipEventElapsedTime(&ms, e0, e1));
      libUs[c] = ms * 1e3 / iters;
    }
    if (rank == 0)
      printf("devapi n=%d ranks_share_one_gpu=%d lsa_barrier_sync_us=%.2f lsa_allreduce_1Mi_f32_%dcta_us=%.1f "
             "nccl_allreduce_1Mi_f32_us=%.1f nccl_allreduce_8B_us=%.2f\n", n, n > ndev ? 1 : 0, barrierUs, kCtas, lsaUs,
             libUs[0], libUs[1]);
    fflush(stdout);  // (a forked rank leaves through _exit)
    HIPCK(hipEventDestroy(e0));
    HIPCK(hipEventDestroy(e1));
  }

  NCCLCK(ncclDevCommDestroy(comm, &devComm));
  NCCLCK(ncclCommWindowDeregister(comm, sendWin));
  NCCLCK(ncclCommWindowDeregister(comm, recvWin));
  NCCLCK(ncclCommFinalize(comm));
  NCCLCK(ncclCommDestroy(comm));
  NCCLCK(ncclMemFree(send));
  NCCLCK(ncclMemFree(recv));
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
  const bool procs = bench || (argc > 2 && !strcmp(argv[2], "procs"));
  if (n < 1 || n > 16) {
    fprintf(stderr, "usage: %s NRANKS(1..16) [procs|bench]\n", argv[0]);
    return 2;
  }
  setenv("NCCL_MULTI_RANK_GPU_ENABLE", "1", 0);
  ncclUniqueId id;
  NCCLCK(ncclGetUniqueId(&id));  // (no HIP call yet: the ranks' processes are forked before the runtime starts)
  int failed = 0;
  if (procs) {
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
  if (!bench) printf("OK n=%d: every element %d\n", n, n * (n - 1) / 2);
  return 0;
}
