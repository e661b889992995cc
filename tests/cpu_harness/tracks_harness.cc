// tracks_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the device tracks' contract in ptz-calib_amd/csrc/ptz_tracks.h
// (what ptz_tracks.hip spreads over lanes, waves and launches): the edges hooked one by one in a scrambled order with plain memory
// in the place of the agent-scope atomics, the labels, the counts, the segments through cursors in a scrambled node order, the
// ranking by counting, the verdicts and the compaction -- so it can be held to a numpy restatement without a GPU.  Never part of the
// product library.  With TRACKS_HARNESS_MAIN it is a stand-alone program (for a sanitizer build): generated graphs, two scrambles
// of each, against a plain breadth-first labelling; returns 0 if they agree.
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_tracks.h"

using namespace ptz;

namespace {

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

template <class T> void scramble(std::vector<T>& v, Rng& r)
{
  for (size_t k = v.size(); k > 1; --k) std::swap(v[k - 1], v[r.next() % k]);
}

}  // namespace

extern "C" {
// The arrays of ptz_tracks_build_device from host arrays: trk_ptr (room for n_feat / 2 + 2), trk_img / trk_feat / trk_node (n_feat),
// trk_uv (2 n_feat), sizes [8].  kp [2 n_feat] or NULL.  An edge out of range is ignored.  0, or -7 when a bounded loop hit its cap.
int32_t h_tracks_build(int32_t n_img, const int64_t* feat_ptr, const float* kp, int32_t n_pair, const int32_t* img_a, const int32_t* img_b,
                       const int64_t* match_ptr, const int32_t* idx_a, const int32_t* idx_b, int32_t min_len, uint64_t seed, int64_t* trk_ptr,
                       int32_t* trk_img, int32_t* trk_feat, int32_t* trk_node, float* trk_uv, int64_t* sizes)
{
  Rng rng(seed);
  const int64_t n = feat_ptr[n_img], n_match = n_pair > 0 ? match_ptr[n_pair] : 0;
  for (int k = 0; k < 8; ++k) sizes[k] = 0;
  trk_ptr[0] = 0;
  if (n <= 0) return 0;
  std::vector<int32_t> parent((size_t)n), label((size_t)n), cnt((size_t)n, 0), cursor((size_t)n, 0);
  std::vector<uint8_t> matched((size_t)n, 0);
  for (int64_t k = 0; k < n; ++k) parent[k] = (int32_t)k;
  // the hook pass: one edge at a time, in any order
  std::vector<int64_t> order((size_t)n_match);
  for (int64_t m = 0; m < n_match; ++m) order[m] = m;
  scramble(order, rng);
  const TrkPlainMem mem;
  for (const int64_t m : order) {
    const int32_t p = trk_owner(match_ptr, n_pair, m);
    int32_t u, v;
    if (!trk_edge_nodes(n_img, feat_ptr, img_a[p], img_b[p], idx_a[m], idx_b[m], &u, &v)) continue;
    matched[u] = matched[v] = 1;
    if (u == v) continue;
    if (!trk_hook(mem, parent.data(), u, v, n)) return -7;
  }
  for (int64_t k = 0; k < n; ++k) {
    label[k] = -1;
    if (!matched[k]) continue;
    label[k] = trk_root(parent.data(), (int32_t)k, n);
    if (label[k] < 0) return -7;
    ++cnt[label[k]];
  }
  // roots by class; the segments in node order, which is ascending label
  std::vector<int64_t> seg_ptr(1, 0), seg_of((size_t)n, -1);
  for (int64_t k = 0; k < n; ++k) {
    if (label[k] < 0) continue;
    ++sizes[2];
    if (label[k] != k) continue;
    ++sizes[3];
    const int32_t cls = trk_class(cnt[k], n_img);
    if (cls == TRK_PIGEON) ++sizes[4];
    if (cls == TRK_SINGLE) ++sizes[5];
    if (cls != TRK_SEGMENT) continue;
    seg_of[k] = (int64_t)seg_ptr.size() - 1;
    seg_ptr.push_back(seg_ptr.back() + cnt[k]);
  }
  const int64_t n_seg = (int64_t)seg_ptr.size() - 1;
  // the scatter through the roots' cursors, in a scrambled node order
  std::vector<int32_t> tmp((size_t)seg_ptr.back() + 1), sorted((size_t)seg_ptr.back() + 1);
  std::vector<int32_t> nodes((size_t)n);
  for (int64_t k = 0; k < n; ++k) nodes[k] = (int32_t)k;
  scramble(nodes, rng);
  for (const int32_t k : nodes) {
    const int32_t r = label[k];
    if (r < 0 || seg_of[r] < 0) continue;
    tmp[seg_ptr[seg_of[r]] + cursor[r]++] = k;
  }
  int64_t n_track = 0, n_view = 0;
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t start = seg_ptr[s];
    const int32_t len = (int32_t)(seg_ptr[s + 1] - start);
    for (int32_t i = 0; i < len; ++i) sorted[start + trk_rank(tmp.data() + start, len, i)] = tmp[start + i];
    bool rep = false;
    for (int32_t i = 0; i + 1 < len; ++i)
      rep = rep || trk_owner(feat_ptr, n_img, sorted[start + i]) == trk_owner(feat_ptr, n_img, sorted[start + i + 1]);
    const int32_t verdict = trk_verdict(rep, len, min_len);
    if (verdict == TRK_REPEAT) ++sizes[4];
    if (verdict == TRK_SHORT) ++sizes[5];
    if (verdict != TRK_KEEP) continue;
    for (int32_t i = 0; i < len; ++i) {
      const int32_t node = sorted[start + i], img = trk_owner(feat_ptr, n_img, node);
      trk_node[n_view + i] = node;
      trk_img[n_view + i] = img;
      trk_feat[n_view + i] = (int32_t)(node - feat_ptr[img]);
      trk_uv[2 * (n_view + i)] = kp ? kp[2 * (int64_t)node] : 0.f;
      trk_uv[2 * (n_view + i) + 1] = kp ? kp[2 * (int64_t)node + 1] : 0.f;
    }
    n_view += len;
    trk_ptr[++n_track] = n_view;
  }
  sizes[0] = n_track;
  sizes[1] = n_view;
  return 0;
}
}

#ifdef TRACKS_HARNESS_MAIN
int main()
{
  Rng rng(5);
  int bad = 0;
  for (int n_img : {1, 2, 7, 33})
    for (int per : {0, 1, 5, 40})
      for (int n_pair : {0, 1, 9, 60}) {
        std::vector<int64_t> fp((size_t)n_img + 1, 0);
        for (int i = 0; i < n_img; ++i) fp[i + 1] = fp[i] + (per ? rng.next() % (per + 1) : 0);
        const int64_t n = fp[n_img];
        std::vector<int32_t> ia, ib, xa, xb;
        std::vector<int64_t> mp(1, 0);
        for (int p = 0; p < n_pair; ++p) {
          ia.push_back((int32_t)(rng.next() % n_img));
          ib.push_back((int32_t)(rng.next() % n_img));
          const int k = (int)(rng.next() % 12);
          for (int m = 0; m < k; ++m) {
            const int32_t t = (int32_t)(rng.next() % (per + 1));  // (sometimes out of range: ignored)
            xa.push_back(t);
            xb.push_back(rng.next() % 10 ? t : (int32_t)(rng.next() % (per + 1)));
          }
          mp.push_back((int64_t)xa.size());
        }
        xa.push_back(0); xb.push_back(0); ia.push_back(0); ib.push_back(0);
        std::vector<int64_t> tp[2];
        std::vector<int32_t> tn[2];
        int64_t sz[2][8];
        for (int run = 0; run < 2; ++run) {
          tp[run].assign((size_t)n / 2 + 2, 0);
          tn[run].assign((size_t)n + 1, 0);
          std::vector<int32_t> ti((size_t)n + 1), tf((size_t)n + 1);
          std::vector<float> tu(2 * (size_t)n + 2);
          if (h_tracks_build(n_img, fp.data(), nullptr, n_pair, ia.data(), ib.data(), mp.data(), xa.data(), xb.data(), 2, 11 + run, tp[run].data(),
                             ti.data(), tf.data(), tn[run].data(), tu.data(), sz[run]) != 0) { printf("cap reached\n"); ++bad; }
        }
        if (tp[0] != tp[1] || tn[0] != tn[1] || !std::equal(sz[0], sz[0] + 8, sz[1])) { printf("two scrambles differ at %d %d %d\n", n_img, per, n_pair); ++bad; }
        // a plain labelling: the first node of every kept track is the smallest of its component
        std::vector<int32_t> lab((size_t)n + 1);
        for (int64_t k = 0; k < n; ++k) lab[k] = (int32_t)k;
        for (bool moved = true; moved;) {
          moved = false;
          for (int p = 0; p < n_pair; ++p)
            for (int64_t m = mp[p]; m < mp[p + 1]; ++m) {
              int32_t u, v;
              if (!trk_edge_nodes(n_img, fp.data(), ia[p], ib[p], xa[m], xb[m], &u, &v)) continue;
              const int32_t low = std::min(lab[u], lab[v]);
              if (lab[u] != low || lab[v] != low) { lab[u] = lab[v] = low; moved = true; }
            }
        }
        for (int64_t t = 0; t < sz[0][0]; ++t)
          for (int64_t e = tp[0][t]; e < tp[0][t + 1]; ++e)
            if (lab[tn[0][e]] != tn[0][tp[0][t]]) { printf("label differs at %d %d %d\n", n_img, per, n_pair); ++bad; e = tp[0][t + 1]; }
      }
  printf("tracks_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
