// An in-place-capable LSA AllReduce written with the device API's reduce-copy family (include/nccl_device_reduce_copy.h):
// barrier acquire, one ncclLsaReduceSumCopy over this rank's and CTA's contiguous slice of the windows, barrier release.
// The setup is devapi_example.hip's: every rank registers a send and a recv window, creates a DevComm with one LSA
// barrier per CTA, and launches on a stream with a hardware queue of its own.
//
//   devapi_rc_example N         one pthread per rank; send -> recv, then in place on the send window; prints OK when
//                               every element equals the sum over the ranks
//   devapi_rc_example N procs   the same with one forked process per rank
//   devapi_rc_example N bench   forked processes; prints timings instead (profiles/README.md), devapi_example's method:
//       the kernel at 2^20 floats with 4 CTAs and then with 32 CTAs, and ncclAllReduce on the same windows
//       (200 launches each after 20 warm-ups).
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

constexpr int kCtas = 4, kMaxCtas = 32, kThreads = 512;

// Rank r's CTA b owns slice r * gridDim.x + b of the elements (whole 16-byte packs, so every slice starts aligned):
// it sums the slice from every rank's send window and writes it into every rank's recv window. send == recv is the
// in-place AllReduce: nobody else touches this slice, and a thread reads all sources of an element before it writes.
__global__ void __launch_bounds__(kThreads) allReduceKernel(ncclDevComm dc, ncclWindow_t send, ncclWindow_t recv,
                                                            size_t count) {
  ncclCoopCta cta;
  ncclLsaBarrierSession<ncclCoopCta> bar(cta, dc, ncclTeamTagLsa(), blockIdx.x);
  bar.sync(cta, std::memory_order_acquire);  // every peer's kernel runs: its input is complete
  const size_t units = (size_t)dc.lsaSize * gridDim.x, unit = (size_t)dc.lsaRank * gridDim.x + blockIdx.x;
  const size_t per = ((count + units - 1) / units + 3) / 4 * 4;
  const size_t start = unit * per < count ? unit * per : count;
  const size_t len = count - start < per ? count - start : per;
  ncclLsaReduceSumCopy(cta, ncclSymPtr<float>(send, 0) + start, ncclSymPtr<float>(recv, 0) + start, len, dc);
  bar.sync(cta, std::memory_order_release);  // every peer has written its share into this rank's recv window
}

static float inputOf(int rank, size_t i) { return (float)(rank + (int)(i % 7)); }

static int check(int rank, int n, const float* dev, size_t count, std::vector<float>& host, const char* what) {
  HIPCK(hipMemcpy(host.data(), dev, count * sizeof(float), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < count; i++) {
    const float want = (float)(n * (n - 1) / 2 + n * (int)(i % 7));
    if (host[i] != want) {
      fprintf(stderr, "rank %d %s: element %zu is %g, expected %g\n", rank, what, i, host[i], want);
      return 1;
    }
  }
  return 0;
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
  std::vector<float> host(count);
  for (size_t i = 0; i < count; i++) host[i] = inputOf(rank, i);
  HIPCK(hipMemcpy(send, host.data(), count * sizeof(float), hipMemcpyHostToDevice));
  HIPCK(hipMemset(recv, 0xff, count * sizeof(float)));
  ncclWindow_t sendWin, recvWin;
  NCCLCK(ncclCommWindowRegister(comm, send, count * sizeof(float), &sendWin, NCCL_WIN_COLL_SYMMETRIC));
  NCCLCK(ncclCommWindowRegister(comm, recv, count * sizeof(float), &recvWin, NCCL_WIN_COLL_SYMMETRIC));

  ncclDevCommRequirements_t reqs = NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER;
  reqs.lsaBarrierCount = kMaxCtas;
  ncclDevComm devComm;
  NCCLCK(ncclDevCommCreate(comm, &reqs, &devComm));

  int rc = 0;
  hipLaunchKernelGGL(allReduceKernel, dim3(kCtas), dim3(kThreads), 0, stream, devComm, sendWin, recvWin, count);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(stream));
  rc = check(rank, n, recv, count, host, "send -> recv");
  if (!rc && !bench) {  // in place on the send window
    hipLaunchKernelGGL(allReduceKernel, dim3(kCtas), dim3(kThreads), 0, stream, devComm, sendWin, sendWin, count);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(stream));
    rc = check(rank, n, send, count, host, "in place");
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
    const int iters = 200, warm = 20;
    const int grids[2] = {kCtas, kMaxCtas};
    double rcUs[2], libUs = 0;
    for (int g = 0; g < 2; g++) {
      for (int i = 0; i < warm + iters; i++) {
        if (i == warm) HIPCK(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(allReduceKernel, dim3(grids[g]), dim3(kThreads), 0, stream, devComm, sendWin, recvWin, count);
      }
      HIPCK(hipEventRecord(e1, stream));
      HIPCK(hipStreamSynchronize(stream));
      HIPCK(hipEventElapsedTime(&ms, e0, e1));
      rcUs[g] = ms * 1e3 / iters;
    }
    for (int i = 0; i < warm + iters; i++) {
      if (i == warm) HIPCK(hipEventRecord(e0, stream));
      NCCLCK(ncclAllReduce(send, recv, count, ncclFloat32, ncclSum, comm, stream));
    }
    HIPCK(hipEventRecord(e1, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    libUs = ms * 1e3 / iters;
    if (rank == 0)
      printf("devapi_rc n=%d ranks_share_one_gpu=%d rc_allreduce_1Mi_f32_%dcta_us=%.1f rc_allreduce_1Mi_f32_%dcta_us=%.1f "
             "nccl_allreduce_1Mi_f32_us=%.1f\n", n, n > ndev ? 1 : 0, kCtas, rcUs[0], kMaxCtas, rcUs[1], libUs);
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
  if (!bench) printf("OK n=%d: out of place and in place\n", n);
  return 0;
}
