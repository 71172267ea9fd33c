// sendrecv_example.cc — a C-ABI caller of ncclSend / ncclRecv / ncclAlltoAll written against include/nccl.h alone (the
// link-time proof that a program using them links with -lnccl):
//
//   sendrecv_example N [BYTES]
//
// ncclCommInitAll over N ranks from one thread, rank i on device i % ndev (N > ndev puts several ranks on one GPU:
// set NCCL_MULTI_RANK_GPU_ENABLE=1). A ring shift (every rank sends BYTES to rank + 1 and receives from rank - 1 in
// one group), then one ncclAlltoAll of BYTES per rank pair. Every byte carries its source rank, destination rank and
// offset, so a block that landed in the wrong place or came from the wrong rank is seen. BYTES defaults to
// 300001 (several channel parts, a ragged tail). Exit 0 and "OK" on success.
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

static unsigned char pattern(size_t i, int src, int dst) {
  return (unsigned char)((i * 131 + (i >> 8) * 7 + (size_t)src * 29 + (size_t)dst * 53 + 11) & 0xff);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: sendrecv_example N [BYTES]\n");
    return 2;
  }
  const int n = atoi(argv[1]);
  const size_t bytes = argc > 2 ? strtoull(argv[2], nullptr, 0) : 300001;
  int ndev = 0;
  HIPOK(hipGetDeviceCount(&ndev));
  if (n < 1 || ndev < 1 || bytes == 0) {
    fprintf(stderr, "bad arguments (N %d BYTES %zu, %d devices)\n", n, bytes, ndev);
    return 2;
  }
  std::vector<int> devs(n);
  for (int r = 0; r < n; r++) devs[r] = r % ndev;
  std::vector<ncclComm_t> comms(n);
  NCCLOK(ncclCommInitAll(comms.data(), n, devs.data()));
  if (gFailures) return 1;

  std::vector<unsigned char*> send(n, nullptr), recv(n, nullptr);
  std::vector<hipStream_t> streams(n);
  std::vector<unsigned char> host(bytes * n), back(bytes * n);
  for (int r = 0; r < n; r++) {
    HIPOK(hipSetDevice(devs[r]));
    HIPOK(hipStreamCreateWithFlags(&streams[r], hipStreamNonBlocking));
    HIPOK(hipMalloc(&send[r], bytes * n));
    HIPOK(hipMalloc(&recv[r], bytes * n));
  }
  for (int pass = 0; pass < 2 && !gFailures; pass++) {
    // pass 0: ring shift of block 0; pass 1: ncclAlltoAll of n blocks
    for (int r = 0; r < n; r++) {
      for (int d = 0; d < n; d++)
        for (size_t i = 0; i < bytes; i++) host[d * bytes + i] = pattern(i, r, pass == 0 ? (r + 1) % n : d);
      HIPOK(hipSetDevice(devs[r]));
      HIPOK(hipMemcpy(send[r], host.data(), bytes * n, hipMemcpyHostToDevice));
      HIPOK(hipMemset(recv[r], 0, bytes * n));
      HIPOK(hipDeviceSynchronize());
    }
    NCCLOK(ncclGroupStart());
    for (int r = 0; r < n; r++) {
      if (pass == 0) {
        NCCLOK(ncclSend(send[r], bytes, ncclUint8, (r + 1) % n, comms[r], streams[r]));
        NCCLOK(ncclRecv(recv[r], bytes, ncclUint8, (r + n - 1) % n, comms[r], streams[r]));
      } else {
        NCCLOK(ncclAlltoAll(send[r], recv[r], bytes, ncclUint8, comms[r], streams[r]));
      }
    }
    NCCLOK(ncclGroupEnd());
    for (int r = 0; r < n; r++) {
      HIPOK(hipSetDevice(devs[r]));
      HIPOK(hipStreamSynchronize(streams[r]));
      ncclResult_t async = ncclSuccess;
      NCCLOK(ncclCommGetAsyncError(comms[r], &async));
      CHECK(async == ncclSuccess, "rank %d: async error %s", r, ncclGetErrorString(async));
      HIPOK(hipMemcpy(back.data(), recv[r], bytes * n, hipMemcpyDeviceToHost));
      size_t bad = 0;
      const int blocks = pass == 0 ? 1 : n;
      for (int b = 0; b < blocks; b++)
        for (size_t i = 0; i < bytes; i++) bad += back[b * bytes + i] != pattern(i, pass == 0 ? (r + n - 1) % n : b, r);
      CHECK(bad == 0, "%s: rank %d: %zu of %zu bytes differ", pass == 0 ? "ring shift" : "ncclAlltoAll", r, bad, bytes * blocks);
    }
  }
  for (int r = 0; r < n; r++) {
    HIPOK(hipSetDevice(devs[r]));
    NCCLOK(ncclCommDestroy(comms[r]));
    HIPOK(hipFree(send[r]));
    HIPOK(hipFree(recv[r]));
    HIPOK(hipStreamDestroy(streams[r]));
  }
  if (gFailures) return 1;
  printf("OK ring shift and all-to-all of %zu bytes per pair over %d ranks\n", bytes, n);
  return 0;
}
