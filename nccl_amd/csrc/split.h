// split.h — the pure parts of ncclCommSplit / ncclCommShrink (init.cc, bootstrap.cc): who belongs to
// a child and in which order, and how many ranks share a GPU once a communicator has ancestors. No HIP call, no
// socket: tests/native/comm_split_test.cc drives these on the CPU.
//
// Reference: src/init.cc:1772-1813 (commGetSplitInfo's insertion rule), :1815-1829 (getParentRanks, on a sorted list).
#pragma once

#include <string.h>

#include <algorithm>
#include <vector>

#include "core.h"

namespace ncclamd {

// The parent ranks of the child of colour `color`, in child-rank order: ascending key, ties by parent rank.
inline std::vector<int> splitMembers(const int* colors, const int* keys, int n, int color) {
  std::vector<int> mem;
  if (color == NCCL_SPLIT_NOCOLOR) return mem;
  for (int r = 0; r < n; r++)
    if (colors[r] == color) mem.push_back(r);
  std::stable_sort(mem.begin(), mem.end(), [&](int a, int b) { return keys[a] < keys[b]; });
  return mem;
}

// The parent ranks a shrink keeps, in parent order; `exclude` need not be sorted (the reference sorts it first).
inline std::vector<int> shrinkMembers(int n, const int* exclude, int count) {
  std::vector<int> ex(exclude, exclude + (count > 0 ? count : 0));
  std::sort(ex.begin(), ex.end());
  std::vector<int> mem;
  size_t j = 0;
  for (int r = 0; r < n; r++) {
    while (j < ex.size() && ex[j] < r) j++;
    if (j < ex.size() && ex[j] == r) continue;
    mem.push_back(r);
  }
  return mem;
}

// How many ranks of a peer table sit on each GPU (by PCI bus id).
inline std::vector<GpuOccupancy> gpuOccupancy(const PeerInfo* peers, size_t n) {
  std::vector<GpuOccupancy> occ;
  for (size_t i = 0; i < n; i++) {
    size_t k = 0;
    while (k < occ.size() && strcmp(occ[k].busId, peers[i].busId)) k++;
    if (k == occ.size()) {
      GpuOccupancy g;
      memset(&g, 0, sizeof(g));
      memcpy(g.busId, peers[i].busId, sizeof(g.busId));
      occ.push_back(g);
    }
    occ[k].ranks++;
  }
  return occ;
}

// The ranks-per-GPU figure of a communicator's channel cap: the most crowded GPU it touches, counted in `occ` — its
// own table's occupancy for a communicator made by ncclCommInitRank / ncclCommInitAll, its oldest ancestor's for a
// child, whose siblings launch on the same GPUs at the same time. A GPU `occ` does not list counts as its own table has it.
inline int ranksPerGpu(const std::vector<GpuOccupancy>& occ, const PeerInfo* peers, size_t n) {
  const std::vector<GpuOccupancy> own = gpuOccupancy(peers, n);
  int most = 1;
  for (const GpuOccupancy& g : own) {
    int ranks = g.ranks;
    for (const GpuOccupancy& o : occ)
      if (!strcmp(o.busId, g.busId) && o.ranks > ranks) ranks = o.ranks;
    if (ranks > most) most = ranks;
  }
  return most;
}

}  // namespace ncclamd
