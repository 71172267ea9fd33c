// Host-only test of what ncclCommSplit / ncclCommShrink do before any GPU is touched: the
// membership rules and the inherited GPU occupancy (nccl_amd/csrc/split.h), and the bootstrap rounds they rendezvous
// with (nccl_amd/csrc/bootstrap.cc) — subset rounds over a real root thread, a rank that hangs up, a silent rank, a
// round that names a departed rank, the two-round split rendezvous and the one-round shrink rendezvous. Ranks are
// threads of this process (the form the TSan build checks). Mode "pure" runs the first half only, "bootstrap" the second,
// "timeout" the silent-rank case.
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#define PLAN_STUBS_NO_GROUP
#include "plan_stubs.h"  // enqueue.cc is linked for coResidentChannelCap: its HIP calls and launches are stubbed

#include "../../nccl_amd/csrc/split.h"
using namespace ncclamd;

static int gFail = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      gFail++;                                                   \
    }                                                            \
  } while (0)

static std::vector<int> V(std::initializer_list<int> l) { return std::vector<int>(l); }

// the reference's insertion rule (src/init.cc:1789-1799), to compare splitMembers with on generated inputs
static std::vector<int> referenceInsertion(const std::vector<int>& colors, const std::vector<int>& keys, int color) {
  std::vector<int> out;
  for (int i = 0; i < (int)colors.size(); i++) {
    if (colors[i] != color) continue;
    size_t insert = 0;
    while (insert < out.size() && keys[out[insert]] <= keys[i]) insert++;
    out.insert(out.begin() + insert, i);
  }
  return out;
}

static void testMembership() {
  {  // by hand: parent ranks 0..4, colours (0,1,0,1,0), keys (5,0,5,-1,1)
    const int colors[5] = {0, 1, 0, 1, 0}, keys[5] = {5, 0, 5, -1, 1};
    EXPECT(splitMembers(colors, keys, 5, 0) == V({4, 0, 2}));
    EXPECT(splitMembers(colors, keys, 5, 1) == V({3, 1}));
    EXPECT(splitMembers(colors, keys, 5, 2).empty());
  }
  {  // NOCOLOR ranks belong to nothing; another negative colour is a colour
    const int colors[4] = {NCCL_SPLIT_NOCOLOR, 7, NCCL_SPLIT_NOCOLOR, -5}, keys[4] = {0, 0, 0, 0};
    EXPECT(splitMembers(colors, keys, 4, NCCL_SPLIT_NOCOLOR).empty());
    EXPECT(splitMembers(colors, keys, 4, 7) == V({1}));
    EXPECT(splitMembers(colors, keys, 4, -5) == V({3}));
  }
  uint64_t x = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int n = 1; n <= 16; n++)
    for (int rep = 0; rep < 50; rep++) {
      std::vector<int> colors(n), keys(n);
      for (int r = 0; r < n; r++) {
        colors[r] = (int)(rnd() % 4) - 1;  // -1 = NOCOLOR, 0..2
        keys[r] = (int)(rnd() % 5) - 2;    // ties and negative keys
      }
      std::vector<int> seen(n, 0);
      for (int color = 0; color <= 2; color++) {
        const std::vector<int> m = splitMembers(colors.data(), keys.data(), n, color);
        EXPECT(m == referenceInsertion(colors, keys, color));
        for (size_t i = 0; i < m.size(); i++) {
          seen[m[i]]++;
          EXPECT(colors[m[i]] == color);
          if (i) EXPECT(keys[m[i - 1]] < keys[m[i]] || (keys[m[i - 1]] == keys[m[i]] && m[i - 1] < m[i]));
        }
      }
      for (int r = 0; r < n; r++) EXPECT(seen[r] == (colors[r] == NCCL_SPLIT_NOCOLOR ? 0 : 1));
      // shrink: an unsorted list of distinct ranks, never all of them
      std::vector<int> ex;
      for (int r = n - 1; r >= 1; r--)
        if (rnd() % 3 == 0) ex.push_back(r);
      if (ex.size() > 1) std::swap(ex[0], ex[ex.size() - 1]);
      const std::vector<int> kept = shrinkMembers(n, ex.data(), (int)ex.size());
      EXPECT(kept.size() == (size_t)n - ex.size());
      for (size_t i = 0; i < kept.size(); i++) {
        if (i) EXPECT(kept[i - 1] < kept[i]);
        for (int e : ex) EXPECT(kept[i] != e);
      }
    }
  {
    const int ex[2] = {3, 1};
    EXPECT(shrinkMembers(4, ex, 2) == V({0, 2}));
    const int ex2[1] = {2};
    EXPECT(shrinkMembers(4, ex2, 1) == V({0, 1, 3}));
  }
}

static std::vector<PeerInfo> table(int n, bool oneGpu) {
  std::vector<PeerInfo> t(n);
  memset(t.data(), 0, n * sizeof(PeerInfo));
  for (int r = 0; r < n; r++) {
    t[r].rank = r;
    t[r].numCUs = 256;
    snprintf(t[r].busId, sizeof(t[r].busId), "0000:%02x:00.0", oneGpu ? 5 : 5 + r);
  }
  return t;
}

static void testOccupancy() {
  const std::vector<PeerInfo> parent = table(8, true);
  const std::vector<GpuOccupancy> occ = gpuOccupancy(parent.data(), parent.size());
  EXPECT(occ.size() == 1 && occ[0].ranks == 8);
  EXPECT(ranksPerGpu(occ, parent.data(), parent.size()) == 8);
  // a child of 2 of them: counted alone it would see 2 ranks on the GPU and take 128 workgroups per launch
  std::vector<PeerInfo> child = {parent[6], parent[1]};
  EXPECT(ranksPerGpu(gpuOccupancy(child.data(), 2), child.data(), 2) == 2);
  EXPECT(ranksPerGpu(occ, child.data(), 2) == 8);
  EXPECT(coResidentChannelCap(256, ranksPerGpu(occ, child.data(), 2)) == 32);
  EXPECT(coResidentChannelCap(256, 2) == 128);
  // a grandchild (the child copied its parent's table) keeps 8
  const std::vector<GpuOccupancy> childOcc = occ;
  std::vector<PeerInfo> grand = {child[1]};
  EXPECT(ranksPerGpu(childOcc, grand.data(), 1) == 8);
  // one rank per GPU: nothing changes, for the parent and for any child
  const std::vector<PeerInfo> spread = table(8, false);
  const std::vector<GpuOccupancy> occ8 = gpuOccupancy(spread.data(), spread.size());
  EXPECT(occ8.size() == 8);
  EXPECT(ranksPerGpu(occ8, spread.data(), spread.size()) == 1);
  std::vector<PeerInfo> pair = {spread[7], spread[2]};
  EXPECT(ranksPerGpu(occ8, pair.data(), 2) == 1);
  EXPECT(coResidentChannelCap(256, 1) == 512);
  // 2 GPUs with 3 + 1 ranks: a child on the quiet GPU alone is not throttled by the crowded one
  std::vector<PeerInfo> mixed = table(4, true);
  snprintf(mixed[3].busId, sizeof(mixed[3].busId), "0000:99:00.0");
  const std::vector<GpuOccupancy> occM = gpuOccupancy(mixed.data(), 4);
  EXPECT(ranksPerGpu(occM, mixed.data(), 4) == 3);
  EXPECT(ranksPerGpu(occM, &mixed[3], 1) == 1);
  EXPECT(ranksPerGpu(occM, &mixed[1], 1) == 3);
}

// ---------------------------------------------------------------- bootstrap rounds, ranks as threads

static void runRanks(int n, const std::function<void(int)>& body) {
  std::vector<std::thread> ts;
  for (int r = 0; r < n; r++) ts.emplace_back(body, r);
  for (auto& t : ts) t.join();
}

static bool subsetRound(Bootstrap* b, int me, uint32_t mask, int tag, ncclResult_t* res) {
  const int cnt = __builtin_popcount(mask);
  std::vector<uint64_t> v(cnt * 2, 0);
  const int at = __builtin_popcount(mask & ((1u << me) - 1));
  v[2 * at] = 1000ull * me + tag;
  v[2 * at + 1] = ~(uint64_t)me;
  *res = bootstrapAllGatherSubset(b, mask, v.data(), 2 * sizeof(uint64_t));
  if (*res != ncclSuccess) return false;
  int i = 0;
  for (int q = 0; q < 32; q++) {
    if (!((mask >> q) & 1)) continue;
    if (v[2 * i] != 1000ull * q + tag || v[2 * i + 1] != ~(uint64_t)q) return false;
    i++;
  }
  return true;
}

static void testRounds() {
  const int n = 4;
  ncclUniqueId id;
  EXPECT(bootstrapGetUniqueId(&id) == ncclSuccess);
  std::vector<Bootstrap*> bs(n, nullptr);
  std::vector<int> bad(n, 0);
  auto step = [&](const std::function<void(int)>& f) { runRanks(n, f); };
  step([&](int r) { bad[r] += bootstrapInit(&id, r, n, &bs[r]) != ncclSuccess; });
  // a full round
  step([&](int r) {
    std::vector<uint64_t> v(n, 0);
    v[r] = 77 + r;
    bad[r] += bootstrapAllGather(bs[r], v.data(), sizeof(uint64_t)) != ncclSuccess;
    for (int q = 0; q < n; q++) bad[r] += v[q] != (uint64_t)(77 + q);
    bad[r] += bootstrapBarrier(bs[r]) != ncclSuccess;
  });
  // rank 2 closes; the service goes on for the others
  bootstrapClose(bs[2]);
  bs[2] = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  step([&](int r) {
    if (r == 2) return;
    ncclResult_t res;
    bad[r] += !subsetRound(bs[r], r, 0xb, 1, &res);  // {0, 1, 3}
  });
  // {0, 3} while rank 1 stays silent
  step([&](int r) {
    if (r != 0 && r != 3) return;
    ncclResult_t res;
    bad[r] += !subsetRound(bs[r], r, 0x9, 2, &res);
  });
  // a round that names the departed rank fails on every participant with ncclRemoteError, a full one too
  step([&](int r) {
    if (r == 2) return;
    ncclResult_t res = ncclSuccess;
    bad[r] += subsetRound(bs[r], r, 0xf, 3, &res) || res != ncclRemoteError;
    bad[r] += bootstrapBarrier(bs[r]) != ncclRemoteError;
  });
  // participants that disagree on the mask fail too
  step([&](int r) {
    if (r != 0 && r != 1) return;
    ncclResult_t res = ncclSuccess;
    bad[r] += subsetRound(bs[r], r, r == 0 ? 0x3 : 0xb, 4, &res) || res != ncclRemoteError;
  });
  // a mask without the caller, or beyond the ranks, is refused before anything is sent
  {
    uint64_t v[8] = {};
    EXPECT(bootstrapAllGatherSubset(bs[0], 0xa, v, 8) == ncclInvalidArgument);
    EXPECT(bootstrapAllGatherSubset(bs[0], 0x11, v, 8) == ncclInvalidArgument);
  }
  // ... and a valid subset round afterwards still works
  step([&](int r) {
    if (r == 2) return;
    ncclResult_t res;
    bad[r] += !subsetRound(bs[r], r, 0xb, 5, &res);
  });
  const auto took = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
  const char* lim = getenv("NCCL_AMD_BOOTSTRAP_TIMEOUT_MS");
  EXPECT(took < (lim ? atol(lim) : 600000));
  // the shrink rendezvous without rank 2: the three meet on the id rank 0 made, in parent order
  step([&](int r) {
    if (r == 2) return;
    ncclUniqueId cid;
    int cr = -1, cn = -1;
    if (bootstrapShrink(bs[r], 1u << 2, &cid, &cr, &cn) != ncclSuccess || cn != 3 || cr != (r == 3 ? 2 : r)) {
      bad[r]++;
      return;
    }
    Bootstrap* cb = nullptr;
    if (bootstrapInit(&cid, cr, cn, &cb) != ncclSuccess) {
      bad[r]++;
      return;
    }
    std::vector<int> v(cn, -1);
    v[cr] = r;
    bad[r] += bootstrapAllGather(cb, v.data(), sizeof(int)) != ncclSuccess;
    bad[r] += !(v[0] == 0 && v[1] == 1 && v[2] == 3);
    bootstrapClose(cb);
  });
  for (Bootstrap* b : bs) bootstrapClose(b);
  for (int r = 0; r < n; r++) EXPECT(bad[r] == 0);
}

// the two-round split rendezvous: 5 ranks, the by-hand case, rank 4 also exercised as NOCOLOR in a second split
static void testSplitRendezvous() {
  const int n = 5;
  ncclUniqueId id;
  EXPECT(bootstrapGetUniqueId(&id) == ncclSuccess);
  std::vector<Bootstrap*> bs(n, nullptr);
  std::vector<int> bad(n, 0);
  runRanks(n, [&](int r) { bad[r] += bootstrapInit(&id, r, n, &bs[r]) != ncclSuccess; });
  const int colors[5] = {0, 1, 0, 1, 0}, keys[5] = {5, 0, 5, -1, 1};
  const std::vector<int> want[2] = {V({4, 0, 2}), V({3, 1})};
  for (int pass = 0; pass < 2; pass++)
    runRanks(n, [&](int r) {
      const int color = pass == 1 && r == 4 ? NCCL_SPLIT_NOCOLOR : colors[r];
      std::vector<int> expect = want[colors[r]];
      if (pass == 1 && colors[r] == 0) expect = V({0, 2});
      ncclUniqueId cid;
      int cr = -1, cn = -1;
      std::vector<int> mem;
      if (bootstrapSplit(bs[r], color, keys[r], &cid, &cr, &cn, &mem) != ncclSuccess) {
        bad[r]++;
        return;
      }
      if (color == NCCL_SPLIT_NOCOLOR) {
        bad[r] += cn != 0;
        return;
      }
      if (mem != expect || cn != (int)expect.size() || expect[cr] != r) {
        bad[r]++;
        return;
      }
      // the members meet on the child's id, in child-rank order
      Bootstrap* cb = nullptr;
      if (bootstrapInit(&cid, cr, cn, &cb) != ncclSuccess) {
        bad[r]++;
        return;
      }
      std::vector<int> v(cn, -1);
      v[cr] = r;
      bad[r] += bootstrapAllGather(cb, v.data(), sizeof(int)) != ncclSuccess;
      bad[r] += v != expect;
      bootstrapClose(cb);
    });
  for (Bootstrap* b : bs) bootstrapClose(b);
  for (int r = 0; r < n; r++) EXPECT(bad[r] == 0);
}

// Mode "timeout" (on its own, not part of "all": it waits for the limit, so tests/test_comm_split_cpu.py runs it with
// NCCL_AMD_BOOTSTRAP_TIMEOUT_MS=300): a subset round that names a rank which is connected but never joins fails at the
// root when the limit passes, and the next valid round works.
static void testSilentRankTimesOut() {
  const int n = 3;
  ncclUniqueId id;
  EXPECT(bootstrapGetUniqueId(&id) == ncclSuccess);
  std::vector<Bootstrap*> bs(n, nullptr);
  std::vector<int> bad(n, 0);
  runRanks(n, [&](int r) { bad[r] += bootstrapInit(&id, r, n, &bs[r]) != ncclSuccess; });
  runRanks(n, [&](int r) {
    if (r == 1) return;
    ncclResult_t res = ncclSuccess;
    bad[r] += subsetRound(bs[r], r, 0x7, 1, &res) || res != ncclRemoteError;
    bad[r] += !subsetRound(bs[r], r, 0x5, 2, &res);
  });
  for (Bootstrap* b : bs) bootstrapClose(b);
  for (int r = 0; r < n; r++) EXPECT(bad[r] == 0);
}

static void testNoRootsLeft() {
  // every rank has hung up: the roots (the parents' and every child's) end on their own
  const auto t0 = std::chrono::steady_clock::now();
  while (bootstrapLiveRoots() != 0 && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(10)) std::this_thread::yield();
  EXPECT(bootstrapLiveRoots() == 0);
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "all";
  const bool pure = !strcmp(mode, "all") || !strcmp(mode, "pure");
  const bool boot = !strcmp(mode, "all") || !strcmp(mode, "bootstrap");
  if (pure) {
    testMembership();
    testOccupancy();
  }
  if (boot) {
    testRounds();
    testSplitRendezvous();
    testNoRootsLeft();
  }
  if (!strcmp(mode, "timeout")) {
    testSilentRankTimesOut();
    testNoRootsLeft();
  }
  printf("comm_split_test %s failures=%d roots_left=%d\n", mode, gFail, bootstrapLiveRoots());
  return gFail ? 1 : 0;
}
