// CPU test of the device API's pure host/device functions (include/nccl_device.h): the resource layout of a DevComm,
// the team functions against brute-force enumeration of the rank sets, and the wrap-safe epoch compare. A stand-alone
// host program built under ASan+UBSan (tests/test_device_api_cpu.py runs it). Prints the struct sizes the Python
// mirrors must match, then OK.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "nccl.h"
#include "nccl_device.h"

static int gFailures = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      if (gFailures++ < 20) {                   \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                    \
        printf("\n");                           \
      }                                         \
    }                                           \
  } while (0)

struct Region {
  size_t lo, hi, align;
};

static void layoutCase(int n, int nb, const std::vector<std::pair<size_t, size_t>>& bufs) {
  std::vector<size_t> sizes, aligns, offs(bufs.size(), ~(size_t)0), offs2(bufs.size(), 0);
  for (auto& b : bufs) sizes.push_back(b.first), aligns.push_back(b.second);
  const ncclDevResourceLayout l =
      ncclDevCommResourceLayout(n, nb, (int)bufs.size(), sizes.data(), aligns.data(), offs.data());
  // the function takes no rank: every rank computes the same layout; and it is deterministic
  const ncclDevResourceLayout l2 =
      ncclDevCommResourceLayout(n, nb, (int)bufs.size(), sizes.data(), aligns.data(), offs2.data());
  EXPECT(l.epochOffset == l2.epochOffset && l.inboxOffset == l2.inboxOffset && l.totalBytes == l2.totalBytes &&
             offs == offs2, "n=%d nb=%d: layout differs between two calls", n, nb);
  EXPECT(l.inboxOffset == ncclLsaBarrierInboxOffset(nb), "n=%d nb=%d: inbox offset", n, nb);
  std::vector<Region> rs;
  rs.push_back({l.epochOffset, l.epochOffset + (size_t)nb * 4, NCCL_DEVICE_RESOURCE_GRANULE});
  rs.push_back({l.inboxOffset, l.inboxOffset + (size_t)nb * n * 4, NCCL_DEVICE_RESOURCE_GRANULE});
  for (size_t k = 0; k < bufs.size(); k++) {
    rs.push_back({offs[k], offs[k] + sizes[k], std::max<size_t>(aligns[k], NCCL_DEVICE_RESOURCE_GRANULE)});
    EXPECT(ncclGetResourceBufferOffset((ncclDevResourceHandle)(offs[k] / NCCL_DEVICE_RESOURCE_GRANULE)) == offs[k],
           "n=%d nb=%d buffer %zu: offset %zu has no handle", n, nb, k, offs[k]);
  }
  EXPECT(l.totalBytes % 4096 == 0 && l.totalBytes > 0, "n=%d nb=%d: total %zu", n, nb, l.totalBytes);
  for (size_t i = 0; i < rs.size(); i++) {
    EXPECT(rs[i].lo % rs[i].align == 0, "n=%d nb=%d region %zu at %zu: alignment %zu", n, nb, i, rs[i].lo, rs[i].align);
    EXPECT(rs[i].hi <= l.totalBytes, "n=%d nb=%d region %zu ends at %zu beyond %zu", n, nb, i, rs[i].hi, l.totalBytes);
    for (size_t j = i + 1; j < rs.size(); j++)
      EXPECT(rs[i].hi <= rs[j].lo || rs[j].hi <= rs[i].lo, "n=%d nb=%d regions %zu and %zu overlap", n, nb, i, j);
  }
}

static std::vector<int> membersOf(const ncclDevComm& dc, ncclTeam t) {
  std::vector<int> m;
  for (int i = 0; i < t.nRanks; i++) m.push_back(ncclTeamRankToWorld(dc, t, i));
  return m;
}

static void teamCase(int n, int inner, int me) {
  ncclDevComm dc = {};
  dc.rank = dc.lsaRank = me;
  dc.nRanks = dc.lsaSize = n;
  const ncclTeam world = ncclTeamWorld(dc), lsa = ncclTeamLsa(dc);
  EXPECT(world.nRanks == n && world.rank == me && world.stride == 1, "world team of rank %d / %d", me, n);
  EXPECT(lsa.nRanks == n && lsa.rank == me && lsa.stride == 1, "lsa team of rank %d / %d", me, n);
  // brute force: the rank sets
  std::vector<int> wantWorld, wantInner, wantOuter;
  for (int w = 0; w < n; w++) {
    wantWorld.push_back(w);
    if (w / inner == me / inner) wantInner.push_back(w);
    if (w % inner == me % inner) wantOuter.push_back(w);
  }
  const ncclTeam in = ncclTeamInnerFactor(world, inner), out = ncclTeamOuterFactor(world, inner);
  struct Named {
    const char* name;
    ncclTeam team;
    std::vector<int> want;
  } teams[3] = {{"world", world, wantWorld}, {"inner", in, wantInner}, {"outer", out, wantOuter}};
  for (const Named& a : teams) {
    EXPECT(membersOf(dc, a.team) == a.want, "n=%d inner=%d me=%d: members of the %s team", n, inner, me, a.name);
    EXPECT(a.team.rank >= 0 && a.team.rank < (int)a.want.size() && a.want[a.team.rank] == me,
           "n=%d inner=%d me=%d: own rank in the %s team", n, inner, me, a.name);
    for (int i = 0; i < a.team.nRanks; i++)
      EXPECT(ncclTeamRankToLsa(dc, a.team, i) == ncclTeamRankToWorld(dc, a.team, i), "lsa rank != world rank");
    for (const Named& b : teams)
      for (int i = 0; i < b.team.nRanks; i++) {
        const int w = b.want[i];
        const auto it = std::find(a.want.begin(), a.want.end(), w);
        const bool member = it != a.want.end();
        EXPECT(ncclTeamRankIsMember(a.team, b.team, i) == member, "n=%d inner=%d me=%d: is %s[%d] (world %d) in %s",
               n, inner, me, b.name, i, w, a.name);
        if (member)
          EXPECT(ncclTeamRankToTeam(a.team, b.team, i) == (int)(it - a.want.begin()),
                 "n=%d inner=%d me=%d: %s[%d] as a rank of %s", n, inner, me, b.name, i, a.name);
      }
  }
  // parent minus subset, for the two factors of the world team (parent ranks of the world team are world ranks)
  for (int s = 1; s <= 2; s++) {
    std::vector<int> diff;
    for (int w = 0; w < n; w++)
      if (std::find(teams[s].want.begin(), teams[s].want.end(), w) == teams[s].want.end()) diff.push_back(w);
    for (int i = 0; i < (int)diff.size(); i++)
      EXPECT(ncclTeamRankInDifference(world, teams[s].team, i) == diff[i],
             "n=%d inner=%d me=%d: element %d of world minus %s: got %d want %d", n, inner, me, i, teams[s].name,
             ncclTeamRankInDifference(world, teams[s].team, i), diff[i]);
  }
}

int main() {
  const int caps[] = {0, 1, 7, 64, NCCL_DEVICE_MAX_LSA_BARRIERS};
  const std::vector<std::vector<std::pair<size_t, size_t>>> lists = {
      {}, {{1, 1}}, {{1000, 256}}, {{65536, 4096}}, {{1, 1}, {1000, 256}, {65536, 4096}},
      {{65536, 4096}, {1, 1}, {1, 1}, {1000, 256}}, {{0, 0}, {3, 2}, {4097, 4096}}};
  for (int n = 1; n <= 8; n++)
    for (int nb : caps)
      for (const auto& bufs : lists) layoutCase(n, nb, bufs);

  for (int n = 1; n <= 8; n++)
    for (int inner = 1; inner <= n; inner++)
      if (n % inner == 0)
        for (int me = 0; me < n; me++) teamCase(n, inner, me);

  const uint32_t epochs[] = {0u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu};
  for (uint32_t e : epochs) {
    const uint32_t want = e + 1u;  // wraps to 0 after 2^32 - 1
    EXPECT(!ncclLsaEpochReached(e, want), "epoch %u: a peer still at the epoch counts as arrived", e);
    EXPECT(!ncclLsaEpochReached(e - 1u, want), "epoch %u: a peer one behind counts as arrived", e);
    EXPECT(ncclLsaEpochReached(want, want), "epoch %u: a peer that arrived does not count", e);
    EXPECT(ncclLsaEpochReached(want + 1u, want), "epoch %u: a peer one ahead does not count", e);
  }

  printf("sizeof ncclDevComm=%zu ncclDevCommRequirements=%zu ncclCommProperties=%zu ncclDevResourceRequirements=%zu\n",
         sizeof(ncclDevComm), sizeof(ncclDevCommRequirements), sizeof(ncclCommProperties),
         sizeof(ncclDevResourceRequirements));
  if (gFailures) {
    printf("%d failures\n", gFailures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
