// ptz_tracks.h -- the contract of the device tracks (ptz_tracks.hip): the connected components of the match table, and which of
// them are feature tracks.  One header for host and device, all integer.  A host build (tests/cpu_harness/tracks_harness.cc) gives
// the device's arrays and numpy restates them (tests/tracks_util.py).
//
// NODES.  Feature `feat` of image `img` is node feat_ptr[img] + feat, image-major: order-isomorphic to the host TracksBuilder's rank
//   of (image, feature) among the matched features (host/tracks.cc).  Fewer than 2^31 features in all.
// EDGES.  Match m of pair p, match_ptr[p] <= m < match_ptr[p + 1], joins (img_a[p], idx_a[m]) and (img_b[p], idx_b[m]): the layout of
//   ptz_desc_matches.  Duplicates, a pair listed twice or reversed, img_a == img_b and an edge from a node to itself are allowed; an
//   edge with an image or a feature out of range is no edge (trk_edge_nodes; the host form of the entry point refuses it first).
// COMPONENTS.  The label of a matched node is the SMALLEST node of its connected component; unmatched features belong to nothing.
//   trk_hook hangs the larger of two roots under the smaller node, so parent[x] <= x always, a root is the smallest node of its tree,
//   and once every edge has been hooked a tree is a component -- whatever the order or the interleaving of the hooks.
// TRACKS.  A component is a track when no image occurs twice among its nodes and it has at least min_len >= 2 nodes: what Build +
//   Filter(min_len) + ExportFlat of host/tracks.cc keep.  trk_verdict: the repeat test comes first, so a component with both defects
//   counts as repeated.  A component of more than n_img nodes repeats an image by pigeonhole and is never laid out.
// ORDER.  Tracks in ascending label; the views of a track in ascending node (trk_rank: ranking by counting), which is ascending
//   image, so a repeat shows between neighbours.
// COUNTS.  Matched nodes, components, components dropped for a repeated image, components dropped as short.
// BOUNDS.  Every walk up a parent chain and every retry loop stops after `cap` (the node count) steps and reports it; no loop waits
//   for anything another lane has yet to do.
#pragma once

#include <stdint.h>

#if !defined(PTZ_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTZ_HD __host__ __device__ __forceinline__
#else
#define PTZ_HD inline
#endif
#endif

namespace ptz {

constexpr int32_t TRK_KEEP = 0, TRK_REPEAT = 1, TRK_SHORT = 2;
constexpr int32_t TRK_NONE = 0, TRK_SEGMENT = 1, TRK_PIGEON = 2, TRK_SINGLE = 3;  // trk_class

// the last index i in [0, n) with ptr[i] <= x, for an offset table ptr [n + 1] with ptr[0] <= x < ptr[n]: the image of a node, the
// pair of a match (empty images and pairs are stepped over)
PTZ_HD int32_t trk_owner(const int64_t* ptr, int32_t n, int64_t x)
{
  int32_t lo = 0, hi = n;  // ptr[lo] <= x < ptr[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (ptr[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the two nodes of an edge; false: an image or a feature out of range
PTZ_HD bool trk_edge_nodes(int32_t n_img, const int64_t* feat_ptr, int32_t ia, int32_t ib, int32_t fa, int32_t fb, int32_t* u, int32_t* v)
{
  if (ia < 0 || ia >= n_img || ib < 0 || ib >= n_img || fa < 0 || fb < 0) return false;
  const int64_t a0 = feat_ptr[ia], b0 = feat_ptr[ib];
  if (fa >= feat_ptr[ia + 1] - a0 || fb >= feat_ptr[ib + 1] - b0) return false;
  *u = (int32_t)(a0 + fa);
  *v = (int32_t)(b0 + fb);
  return true;
}

// How the parent array is reached.  The hook launch of the device reads and writes it with agent-scope atomics only (workgroups on
// different XCDs hook into the same array); every later launch, and the host, read it plainly.
struct TrkPlainMem {
  PTZ_HD int32_t load(const int32_t* p) const { return *p; }
  PTZ_HD void store(int32_t* p, int32_t v) const { *p = v; }
  // true: *p was `expect` and is now `v`; false: *seen is what it held
  PTZ_HD bool cas(int32_t* p, int32_t expect, int32_t v, int32_t* seen) const
  {
    if (*p != expect) { *seen = *p; return false; }
    *p = v;
    return true;
  }
};

// the root of x, halving the path on the way (a node's parent becomes its grandparent: an ancestor then and ever after, so a
// halving store that races another one or a hook leaves a correct tree); -1 after `cap` steps
template <class Mem> PTZ_HD int32_t trk_find(const Mem& mem, int32_t* parent, int32_t x, int64_t cap)
{
  for (int64_t step = 0; step <= cap; ++step) {
    const int32_t p = mem.load(parent + x);
    if (p == x) return x;
    const int32_t g = mem.load(parent + p);
    if (g != p) mem.store(parent + x, g);
    x = g;
  }
  return -1;
}

// the root of x without a write: the launches after the hooks
PTZ_HD int32_t trk_root(const int32_t* parent, int32_t x, int64_t cap)
{
  for (int64_t step = 0; step <= cap; ++step) {
    const int32_t p = parent[x];
    if (p == x) return x;
    x = p;
  }
  return -1;
}

// one edge: the larger root goes under the smaller one by a compare-and-swap on parent[larger]; a swap that lost goes on from what it
// saw.  false: a cap was reached.
template <class Mem> PTZ_HD bool trk_hook(const Mem& mem, int32_t* parent, int32_t u, int32_t v, int64_t cap)
{
  for (int64_t turn = 0; turn <= cap; ++turn) {
    u = trk_find(mem, parent, u, cap);
    v = trk_find(mem, parent, v, cap);
    if (u < 0 || v < 0) return false;
    if (u == v) return true;
    const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
    int32_t seen = hi;
    if (mem.cas(parent + hi, hi, lo, &seen)) return true;
    u = seen;  // hi has a parent now: smaller than hi, in the same tree
    v = lo;
  }
  return false;
}

// what becomes of a root with `count` nodes: a component of one node (a self edge) is short, one of more than n_img nodes repeats an
// image, the others are laid out as segments and judged by trk_verdict
PTZ_HD int32_t trk_class(int32_t count, int32_t n_img)
{
  if (count <= 0) return TRK_NONE;
  if (count == 1) return TRK_SINGLE;
  return count > n_img ? TRK_PIGEON : TRK_SEGMENT;
}

// the position of seg[i] among the len distinct nodes of a segment in ascending order
PTZ_HD int32_t trk_rank(const int32_t* seg, int32_t len, int32_t i)
{
  const int32_t x = seg[i];
  int32_t r = 0;
  for (int32_t j = 0; j < len; ++j) r += seg[j] < x ? 1 : 0;
  return r;
}

PTZ_HD int32_t trk_verdict(bool repeat, int32_t len, int32_t min_len) { return repeat ? TRK_REPEAT : (len < min_len ? TRK_SHORT : TRK_KEEP); }

}  // namespace ptz
