// bcast_plan_test.cc — CPU test driver of the Broadcast plan (enqueue.cc) and of the partition the Broadcast kernels
// walk. Compiled with the planning sources like plan_test (no GPU: launches and the few HIP calls are stubbed, plan_stubs.h), it
// slices every plan with the SAME host-callable functions the kernels call (device_abi.h blockLenOf / sliceBounds /
// llPartBounds), so nothing of the arithmetic is restated here.
//
//   bcast_plan_test matrix   NCCL_ALGO / NCCL_PROTO as loadTuning resolves them for Broadcast:
//                            "parse=<ncclResult_t>" and "func=broadcast algo=... noalgo=... ll= ll128= simple="
//   bcast_plan_test plan NRANKS BYTES [ROOT]
//                            one ncclBroadcast through the entry point: "result=<ncclResult_t>" and, when it launched,
//                            "algo=<direct|ll|ll128|copy> nch= part= slice= steps= chunk= root="
//   bcast_plan_test sweep    n in 2..8 x byte counts x slot sizes {4096, default} x NCCL_PROTO {unset, Simple, LL,
//                            LL128}: the (block, channel, step) slices of a direct plan tile [0, bytes) exactly once, an
//                            empty block is owned but moves nothing, and the parts of an LL / LL64 plan tile the payload
//                            units with no empty channel. Prints "OK cases=<n> direct=<n> ll=<n> ll128=<n>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define PLAN_STUBS_NO_GROUP
#include "plan_stubs.h"

using namespace ncclamd;

// Broadcast never plans a zero-copy kernel: a zero-copy launch is an error, and the buffers count as registered
// (regLookup and regCovers answer true), so that a plan that stayed staged did so for being a Broadcast's
static void initComm(ncclComm& comm, int n, size_t slotBytes) {
  gStubs.refuseSymLaunch = gStubs.regLookupAlways = gStubs.regCoversAnswer = true;
  stubComm(comm, n, 0, slotBytes, 256);
  resolveLinkChannels(&comm.tune, n, getenv("NCCL_MAX_CTAS") != nullptr);
}

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, "FAIL: ");    \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return false;                 \
    }                               \
  } while (0)

// One Broadcast of `bytes` on n ranks: plan it through the entry point and check the partition. kind: 0 direct, 1 LL, 2 LL64.
static bool checkOne(int n, size_t bytes, size_t slotBytes, const char* proto, int* kind) {
  ncclComm comm;
  initComm(comm, n, slotBytes);
  gStubs.launches = 0;
  const ncclResult_t r = ncclBroadcast((const void*)0x10000000ull, (void*)0x20000000ull, bytes, ncclUint8, (int)(bytes % n),
                                       &comm, nullptr);
  REQUIRE(r == ncclSuccess && gStubs.launches == 1, "n %d bytes %zu proto %s: result %d, %d launches", n, bytes, proto, (int)r, gStubs.launches);
  const LaunchPlan& p = gStubs.plan;
  REQUIRE(p.func == FUNC_BROADCAST && p.eltSize == 1, "n %d bytes %zu: func %d eltSize %d", n, bytes, (int)p.func, p.eltSize);
  if (p.algo == ALGO_LL) {
    const LLOp& o = p.ll.ops[0];
    const bool ll64 = o.proto == LLP_LL64;
    *kind = ll64 ? 2 : 1;
    const uint64_t units = ll64 ? (bytes + kLL64Payload - 1) / kLL64Payload : (bytes + 7) / 8;
    REQUIRE(o.coll == LL_BCAST && o.count == bytes && o.nch == p.nChannels && o.nch >= 1 && o.nch <= comm.llChannels,
            "n %d bytes %zu %s: coll %d count %lu nch %d grid %d", n, bytes, proto, o.coll, (unsigned long)o.count, o.nch, p.nChannels);
    REQUIRE(o.part * (ll64 ? 64 : 16) <= comm.llBytes, "n %d bytes %zu: part %lu overflows the line area", n, bytes, (unsigned long)o.part);
    uint64_t next = 0;
    for (int j = 0; j < o.nch; j++) {
      uint64_t lo, hi;
      llPartBounds(o.part, j, units, lo, hi);
      REQUIRE(lo == next && hi > lo, "n %d bytes %zu %s: channel %d of %d holds [%lu, %lu), expected to start at %lu and be non-empty",
              n, bytes, proto, j, o.nch, (unsigned long)lo, (unsigned long)hi, (unsigned long)next);
      next = hi;
    }
    REQUIRE(next == units, "n %d bytes %zu %s: parts end at %lu of %lu units", n, bytes, proto, (unsigned long)next, (unsigned long)units);
    return true;
  }
  *kind = 0;
  REQUIRE(p.algo == ALGO_DIRECT, "n %d bytes %zu %s: algo %d", n, bytes, proto, p.algo);
  const CollArgs& a = p.args;
  REQUIRE(a.count == bytes && a.chunk % 16 == 0 && a.chunk * n >= bytes && a.part % 16 == 0 && a.slice % 16 == 0 && a.slice > 0 &&
              a.slice * 1 <= comm.slotBytes && p.nChannels >= 1 && p.nChannels <= comm.chanCap,
          "n %d bytes %zu: count %lu chunk %lu part %lu slice %lu nch %d", n, bytes, (unsigned long)a.count,
          (unsigned long)a.chunk, (unsigned long)a.part, (unsigned long)a.slice, p.nChannels);
  std::vector<unsigned char> seen(bytes, 0);
  for (int b = 0; b < n; b++) {  // block b is owned by rank b, whatever it holds
    const uint64_t len = blockLenOf(a.count, a.chunk, b);
    uint64_t moved = 0;
    for (int c = 0; c < p.nChannels; c++)
      for (int s = 0; s < a.nSteps; s++) {
        uint64_t lo, hi;
        sliceBounds(a.part, a.slice, c, s, len, lo, hi);
        REQUIRE(lo <= hi && hi <= len && hi - lo <= a.slice, "n %d bytes %zu: block %d channel %d step %d: [%lu, %lu) of %lu",
                n, bytes, b, c, s, (unsigned long)lo, (unsigned long)hi, (unsigned long)len);
        REQUIRE(lo % 16 == 0, "n %d bytes %zu: block %d channel %d step %d starts at %lu", n, bytes, b, c, s, (unsigned long)lo);
        for (uint64_t x = (uint64_t)b * a.chunk + lo; x < (uint64_t)b * a.chunk + hi; x++) {
          REQUIRE(x < bytes && !seen[x], "n %d bytes %zu: byte %lu %s", n, bytes, (unsigned long)x, x < bytes ? "moved twice" : "past the end");
          seen[x] = 1;
        }
        moved += hi - lo;
      }
    REQUIRE(moved == len, "n %d bytes %zu: block %d moves %lu of its %lu bytes", n, bytes, b, (unsigned long)moved, (unsigned long)len);
  }
  for (size_t x = 0; x < bytes; x++) REQUIRE(seen[x], "n %d bytes %zu: byte %zu never moved", n, bytes, x);
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "matrix")) {
    CommTuning t;
    loadTuning(&t);
    const FuncTuning& ft = t.fn[FUNC_BROADCAST];
    const char* force[] = {"none", "oneshot", "direct", "ring", "tree"};
    printf("parse=%d\n", t.parseError);
    printf("func=broadcast algo=%s oneshot=%d direct=%d noalgo=%d ll=%d ll128=%d simple=%d\n", force[ft.algo], ft.oneShotOk,
           ft.directOk, ft.noAlgo, ft.llOn, ft.ll128On, ft.simpleOn);
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "plan")) {
    const int n = atoi(argv[2]);
    const size_t bytes = strtoull(argv[3], nullptr, 0);
    const int root = argc > 4 ? atoi(argv[4]) : 0;
    ncclComm comm;
    initComm(comm, n, 0);
    const ncclResult_t r = ncclBroadcast((const void*)0x10000000ull, (void*)0x20000000ull, bytes, ncclUint8, root, &comm, nullptr);
    printf("result=%d launches=%d\n", (int)r, gStubs.launches);
    if (r != ncclSuccess || gStubs.launches == 0) return 0;
    const LaunchPlan& p = gStubs.plan;
    if (p.algo == ALGO_LL)
      printf("algo=%s nch=%d part=%lu root=%d\n", p.ll.ops[0].proto == LLP_LL64 ? "ll128" : "ll", p.nChannels,
             (unsigned long)p.ll.ops[0].part, p.ll.ops[0].root);
    else
      printf("algo=%s nch=%d part=%lu slice=%lu steps=%d chunk=%lu root=%d\n", p.algo == ALGO_COPY ? "copy" : "direct",
             p.nChannels, (unsigned long)p.args.part, (unsigned long)p.args.slice, p.args.nSteps, (unsigned long)p.args.chunk,
             p.args.root);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "sweep")) {
    const char* protos[] = {nullptr, "Simple", "LL", "LL128"};
    int cases = 0, kinds[3] = {0, 0, 0};
    for (const char* proto : protos) {
      if (proto) setenv("NCCL_PROTO", proto, 1);
      else unsetenv("NCCL_PROTO");
      for (int n = 2; n <= 8; n++) {
        const size_t sizes[] = {1, 15, 16, 17, (size_t)16 * n - 1, (size_t)16 * n, (size_t)16 * n + 1, 4099, 300001, ((size_t)1 << 20) | 3};
        for (size_t bytes : sizes)
          for (size_t slot : {(size_t)4096, (size_t)0}) {
            int kind = -1;
            if (!checkOne(n, bytes, slot, proto ? proto : "(unset)", &kind)) return 1;
            // the protocol NCCL_PROTO leaves is the one planned, wherever the line area holds the payload
            if (proto && !strcmp(proto, "Simple") && kind != 0) return fprintf(stderr, "FAIL: Simple planned kind %d\n", kind), 1;
            if (proto && !strcmp(proto, "LL") && bytes <= 4099 && kind != 1) return fprintf(stderr, "FAIL: LL planned kind %d\n", kind), 1;
            if (proto && !strcmp(proto, "LL128") && bytes <= 300001 && kind != 2) return fprintf(stderr, "FAIL: LL128 planned kind %d\n", kind), 1;
            cases++;
            kinds[kind]++;
          }
      }
    }
    printf("OK cases=%d direct=%d ll=%d ll128=%d\n", cases, kinds[0], kinds[1], kinds[2]);
    return 0;
  }
  fprintf(stderr, "usage: bcast_plan_test matrix | plan NRANKS BYTES [ROOT] | sweep\n");
  return 2;
}
