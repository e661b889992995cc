// ptz_desc_sweep.h -- the streamed top-2 sweep of the descriptor kernels (device only): k_desc_top2 (ptz_desc_match.hip) and
// k_desc_votes (ptz_desc_shortlist.hip) are outer shapes around it.  The matcher's tie rule -- the lowest j -- lives here and
// nowhere else, so a shortlist vote is a bit of the matcher's top-2 by construction.
//
//   pack      a byte xor 0x80 is (a - 128) as int8; the bias cancels in a - b, so d2 = |a'|^2 + |b'|^2 - 2 a'.b'.  Rows are padded
//             with zeros to DP = 64 KS bytes, images to a multiple of 64 rows (zero rows, norm INT32_MAX: the dot product of a
//             padding row is exactly 0, its key INT32_MAX, and it never beats the empty state).
//   sweep     a wave holds QT tiles of 16 queries for the whole DP in registers (the B operand of v_mfma_i32_16x16x64_i8) and
//             streams the other image in tiles of 16 rows (the A operand) straight from global memory, one tile ahead; the tile
//             ahead of the last one is the last one again, so no load leaves the image's padded rows and the loop has no branch.
//             Lane l of the result holds C[row 4 (l >> 4) + r][col l & 15]: ONE query per lane, four candidates per step.  The
//             DP x n product is never written: every (query tile, key, j) goes to the caller, key = d2 less the query's norm,
//             which every candidate of a query shares.
//   top-2     the running (best, best j, second) of a lane's query is three registers.  Candidates reach a lane in ascending j, so
//             `<` keeps the lowest j there; the four lanes of a query are merged once at the end with ptz_desc_match.h's rule.
#pragma once

#include "ptz_common.h"
#include "ptz_desc_match.h"

namespace ptz {

typedef int v4i __attribute__((ext_vector_type(4)));

// the 16 bytes of k-step s of a packed row that lane group g feeds to the MFMA
template <int KS>
__device__ __forceinline__ v4i desc_frag(const int8_t* __restrict__ desc, int64_t row, int s, int g)
{
  return *reinterpret_cast<const v4i*>(desc + row * (KS * 64) + s * 64 + g * 16);
}

// one lane's running top-2 over candidates that arrive in ascending j
struct DescRun {
  int32_t bd = kDescNone, bj = kDescNone, sd = kDescNone;
  __device__ __forceinline__ void take(int32_t key, int32_t j)
  {
    sd = min(sd, max(bd, key));
    bj = key < bd ? j : bj;
    bd = min(bd, key);
  }
};

// f(t, key, j) for every candidate j of the image at (desc, norm), ns features, and the query this lane holds of tile t;
// c = lane & 15, g = lane >> 4.  Rows up to 16 ceil(ns / 16) are read: inside the image's padded rows.
template <int KS, int QT, class F>
__device__ __forceinline__ void desc_sweep(const v4i (&qf)[QT][KS], const int8_t* __restrict__ desc, const int32_t* __restrict__ norm, int ns,
                                           int c, int g, F&& f)
{
  const int nt = (ns + 15) >> 4;
  if (nt == 0) return;
  v4i sf[KS], nf[KS], skey, nkey;
#pragma unroll
  for (int s = 0; s < KS; ++s) sf[s] = desc_frag<KS>(desc, c, s, g);
  skey = *reinterpret_cast<const v4i*>(norm + 4 * g);
  for (int jt = 0; jt < nt; ++jt) {
    const int jn = min(jt + 1, nt - 1);
#pragma unroll
    for (int s = 0; s < KS; ++s) nf[s] = desc_frag<KS>(desc, 16 * jn + c, s, g);
    nkey = *reinterpret_cast<const v4i*>(norm + 16 * jn + 4 * g);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      v4i acc = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(sf[s], qf[t][s], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) f(t, skey[r] - 2 * acc[r], 16 * jt + 4 * g + r);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) sf[s] = nf[s];
    skey = nkey;
  }
}

// the query's top-2 from its four lanes' runs (every lane of the wave calls this); qnorm turns keys into d2
__device__ __forceinline__ DescTop2 desc_run_finish(const DescRun& r, int32_t qnorm)
{
  DescTop2 T;
  T.d = r.bd == kDescNone ? kDescNone : r.bd + qnorm;
  T.j = r.bj;
  T.s = r.sd == kDescNone ? kDescNone : r.sd + qnorm;
#pragma unroll
  for (int d = 16; d <= 32; d <<= 1) {
    DescTop2 O;
    O.d = __shfl_xor(T.d, d);
    O.j = __shfl_xor(T.j, d);
    O.s = __shfl_xor(T.s, d);
    T = desc_top2_merge(T, O);
  }
  return T;
}

// `...` with K a constant expression equal to ks (a set's KS: 1 .. kDescMaxDim / 64)
#define PTZ_DESC_KS_CASE(K_, ...) case K_: { constexpr int K = K_; __VA_ARGS__; } break;
#define PTZ_DESC_FOR_KS(ks, ...) \
  switch (ks) { \
    PTZ_DESC_KS_CASE(1, __VA_ARGS__) PTZ_DESC_KS_CASE(2, __VA_ARGS__) PTZ_DESC_KS_CASE(3, __VA_ARGS__) PTZ_DESC_KS_CASE(4, __VA_ARGS__) \
    PTZ_DESC_KS_CASE(5, __VA_ARGS__) PTZ_DESC_KS_CASE(6, __VA_ARGS__) PTZ_DESC_KS_CASE(7, __VA_ARGS__) PTZ_DESC_KS_CASE(8, __VA_ARGS__) \
  }

}  // namespace ptz
