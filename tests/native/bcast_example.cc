// bcast_example.cc — a C-ABI caller of ncclBroadcast / ncclBcast written against include/nccl.h alone (the link-time
// proof that a program using them links with -lnccl):
//
//   bcast_example N ROOT [BYTES]
//
// ncclCommInitAll over N ranks from one thread, rank i on device i % ndev (N > ndev puts several ranks on one GPU:
// set NCCL_MULTI_RANK_GPU_ENABLE=1). The root's buffer holds a known byte pattern; one ncclBroadcast (out of place,
// every other rank's sendbuff NULL) and one ncclBcast (in place) must leave it in every rank's buffer. BYTES
// defaults to 1 MiB + 3 (the staged kernel, a ragged tail); try 1000 for the LL kernel. Exit 0 and "OK" on success.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "nccl.h"

static int gFailures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      gFailures++;                  \
    }                               \
  } while (0)
#define HIPOK(x) CHECK((x) == hipSuccess, "line %d: %s failed", __LINE__, #x)
#define NCCLOK(x)                                                                             \
  do {                                                                                        \
    ncclResult_t _r = (x);                                                                    \
    CHECK(_r == ncclSuccess, "line %d: %s: %s", __LINE__, #x, ncclGetErrorString(_r));        \
  } while (0)

static unsigned char pattern(size_t i, int salt) { return (unsigned char)((i * 131 + (i >> 8) * 7 + salt) & 0xff); }

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: bcast_example N ROOT [BYTES]\n");
    return 2;
  }
  const int n = atoi(argv[1]), root = atoi(argv[2]);
  const size_t bytes = argc > 3 ? strtoull(argv[3], nullptr, 0) : (1u << 20) + 3;
  int ndev = 0;
  HIPOK(hipGetDeviceCount(&ndev));
  if (n < 1 || root < 0 || root >= n || ndev < 1 || bytes == 0) {
    fprintf(stderr, "bad arguments (N %d ROOT %d BYTES %zu, %d devices)\n", n, root, bytes, ndev);
    return 2;
  }
  std::vector<int> devs(n);
  for (int r = 0; r < n; r++) devs[r] = r % ndev;
  std::vector<ncclComm_t> comms(n);
  NCCLOK(ncclCommInitAll(comms.data(), n, devs.data()));
  if (gFailures) return 1;

  std::vector<unsigned char*> send(n, nullptr), recv(n, nullptr);
  std::vector<hipStream_t> streams(n);
  std::vector<unsigned char> host(bytes), back(bytes);
  for (int r = 0; r < n; r++) {
    HIPOK(hipSetDevice(devs[r]));
    HIPOK(hipStreamCreateWithFlags(&streams[r], hipStreamNonBlocking));
    HIPOK(hipMalloc(&recv[r], bytes));
    HIPOK(hipMemset(recv[r], 0, bytes));
  }
  HIPOK(hipSetDevice(devs[root]));
  HIPOK(hipMalloc(&send[root], bytes));
  for (int pass = 0; pass < 2 && !gFailures; pass++) {
    // pass 0: ncclBroadcast out of place from send[root]; pass 1: ncclBcast in place on recv[]
    for (size_t i = 0; i < bytes; i++) host[i] = pattern(i, 17 + pass);
    HIPOK(hipSetDevice(devs[root]));
    HIPOK(hipMemcpy(pass == 0 ? send[root] : recv[root], host.data(), bytes, hipMemcpyHostToDevice));
    HIPOK(hipDeviceSynchronize());
    NCCLOK(ncclGroupStart());
    for (int r = 0; r < n; r++) {
      if (pass == 0) NCCLOK(ncclBroadcast(send[r], recv[r], bytes, ncclUint8, root, comms[r], streams[r]));
      else NCCLOK(ncclBcast(recv[r], bytes, ncclUint8, root, comms[r], streams[r]));
    }
    NCCLOK(ncclGroupEnd());
    for (int r = 0; r < n; r++) {
      HIPOK(hipSetDevice(devs[r]));
      HIPOK(hipStreamSynchronize(streams[r]));
      ncclResult_t async = ncclSuccess;
      NCCLOK(ncclCommGetAsyncError(comms[r], &async));
      CHECK(async == ncclSuccess, "rank %d: async error %s", r, ncclGetErrorString(async));
      HIPOK(hipMemcpy(back.data(), recv[r], bytes, hipMemcpyDeviceToHost));
      size_t bad = 0;
      for (size_t i = 0; i < bytes; i++) bad += back[i] != host[i];
      CHECK(bad == 0, "%s: rank %d: %zu of %zu bytes differ", pass == 0 ? "ncclBroadcast" : "ncclBcast", r, bad, bytes);
    }
  }
  for (int r = 0; r < n; r++) {
    HIPOK(hipSetDevice(devs[r]));
    NCCLOK(ncclCommDestroy(comms[r]));
    HIPOK(hipFree(recv[r]));
    HIPOK(hipStreamDestroy(streams[r]));
  }
  HIPOK(hipFree(send[root]));
  if (gFailures) return 1;
  printf("OK broadcast of %zu bytes from rank %d to %d ranks\n", bytes, root, n);
  return 0;
}
