// ptz_desc_match.hip -- the match table from features: mutual nearest neighbours of uint8 descriptors under Lowe's ratio test for a
// batch of image pairs (ptz_desc_match_pairs).  The contract is ptz_desc_match.h; everything here is integer arithmetic, so a
// pair's matches are the bits of the brute-force restatement whatever the batch, the tiling or the chunking.
//
//   pack      k_desc_pack writes the rows ptz_desc_sweep.h describes.
//   top-2     one workgroup = (pair, direction, 128 query rows): each of its four waves holds two tiles of 16 queries and runs
//             ptz_desc_sweep.h's sweep over the other image; the g == 0 lanes store the finished top-2.
//   guided    ptz_desc_match_pairs_guided: the same running top-2 over the candidates within a radius of where the pair's
//             homography puts the feature (the header's predicate) -- a radius search over positions staged in LDS, one query per
//             lane, the exact d2 from the packed rows only on a hit; the state, and everything behind it, is the dense pass's.
//   grid      ptz_desc_match_pairs_guided_grid: the guided contract again (ptz_desc_grid.h), selectable and off by default -- the
//             searched positions sorted into the cells of a grid in LDS, a query testing only the cells its reach touches, the
//             d2 of a hit computed by the wave; the same state bit for bit.
//   join      the acceptance rule per feature of A -> a keep byte; counting, scan and scatter are ptz_gate_compact.h's kernels
//             (min_matches as `need`); a gather writes indices, distances and the pixels of the resident key points.
#include <cmath>
#include <memory>
#include <vector>

#include "ptz_common.h"
#include "ptz_desc_grid.h"
#include "ptz_desc_match.h"
#include "ptz_desc_set.h"
#include "ptz_desc_sweep.h"
#include "ptz_gate_compact.h"
#include "ptz_host_batch.h"

namespace ptz {
namespace {

constexpr int DESC_WG = 256;     // four waves
constexpr int DESC_QT = 2;       // query tiles of 16 per wave
constexpr int DESC_WG_Q = (DESC_WG / WAVE) * DESC_QT * 16;  // 128 queries per workgroup
constexpr int DESC_G_TILE = 1024; // positions of the other image a guided workgroup stages in LDS at a time (8 KB)
constexpr int DESC_G_UNROLL = 8;  // candidates a lane tests between two looks for a hit (divides DESC_G_TILE)
constexpr int DESC_CHUNK_PAIRS = 1 << 20;  // most pairs of a chunk: its launches have a workgroup row per pair and direction

struct DescPair {
  int64_t row_a, row_b;  // first packed row of the two images
  int64_t kp_a, kp_b;    // first key point
  int64_t soff;          // first top-2 state of the pair in its chunk: A's n_a, then B's n_b
  int64_t aoff;          // first keep byte (position of A's feature 0 in the chunk's list of A features)
  int32_t n_a, n_b;
};

// one thread per packed row of image blockIdx.x (the last "image" is the slack behind the set: no features, 64 rows)
__global__ __launch_bounds__(256) void k_desc_pack(const int64_t* __restrict__ feat_ptr, const int64_t* __restrict__ row_off,
                                                   const uint8_t* __restrict__ raw, int D, int DP, uint32_t* __restrict__ desc,
                                                   int32_t* __restrict__ norm)
{
  const int m = blockIdx.x;
  const int64_t f0 = feat_ptr[m], n = feat_ptr[m + 1] - f0, r0 = row_off[m], np = row_off[m + 1] - r0;
  for (int64_t r = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; r < np; r += (int64_t)gridDim.y * blockDim.x) {
    uint32_t* o = desc + (r0 + r) * (DP / 4);
    int32_t sum = INT32_MAX;
    if (r < n) {
      const uint8_t* src = raw + (f0 + r) * D;
      sum = 0;
      for (int k = 0; k < DP; k += 4) {
        uint32_t w = 0;
        for (int b = 0; b < 4; ++b) {
          const int v = k + b < D ? (int)src[k + b] - 128 : 0;
          w |= (uint32_t)(v & 255) << (8 * b);
          sum += v * v;
        }
        o[k / 4] = w;
      }
    }
    else {
      for (int k = 0; k < DP; k += 4) o[k / 4] = 0u;
    }
    norm[r0 + r] = sum;
  }
}

// blockIdx.x = pair * dirs + direction (0: A's features ask B, 1: B's ask A), blockIdx.y (strided) = tile of 128 queries.
// DUMP: the distances themselves to dump [n_q, n_s] instead of the top-2 (ptz_debug_desc_dist2: the same fragments, the same map).
template <int KS, bool DUMP>
__global__ __launch_bounds__(DESC_WG) void k_desc_top2(const DescPair* __restrict__ pairs, int dirs, const int8_t* __restrict__ desc_a,
                                                       const int32_t* __restrict__ norm_a, const int8_t* __restrict__ desc_b,
                                                       const int32_t* __restrict__ norm_b, DescTop2* __restrict__ state,
                                                       int32_t* __restrict__ dump)
{
  constexpr int DP = KS * 64;
  const DescPair P = pairs[blockIdx.x / dirs];
  const int dir = blockIdx.x % dirs;
  const int nq = dir ? P.n_b : P.n_a, ns = dir ? P.n_a : P.n_b;
  const int8_t* qd = dir ? desc_b + P.row_b * DP : desc_a + P.row_a * DP;
  const int32_t* qn = dir ? norm_b + P.row_b : norm_a + P.row_a;
  const int8_t* sdp = dir ? desc_a + P.row_a * DP : desc_b + P.row_b * DP;
  const int32_t* sn = dir ? norm_a + P.row_a : norm_b + P.row_b;
  DescTop2* out = DUMP ? nullptr : state + P.soff + (dir ? P.n_a : 0);
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, c = lane & 15, g = lane >> 4;

  for (int64_t tile = blockIdx.y; tile * DESC_WG_Q < nq; tile += gridDim.y) {
    const int q0 = (int)(tile * DESC_WG_Q) + wave * (DESC_QT * 16);
    if (q0 >= nq) continue;  // (one value per wave; rows q0 .. q0 + 31 lie inside the image's padded rows)
    v4i qf[DESC_QT][KS];
#pragma unroll
    for (int t = 0; t < DESC_QT; ++t)
#pragma unroll
      for (int s = 0; s < KS; ++s) qf[t][s] = desc_frag<KS>(qd, q0 + 16 * t + c, s, g);
    if (DUMP) {
      desc_sweep<KS, DESC_QT>(qf, sdp, sn, ns, c, g, [&](int t, int32_t key, int32_t jj) {
        const int q = q0 + 16 * t + c;
        if (q < nq && jj < ns) dump[(int64_t)q * ns + jj] = key + qn[q];
      });
      continue;
    }
    DescRun run[DESC_QT];
    desc_sweep<KS, DESC_QT>(qf, sdp, sn, ns, c, g, [&](int t, int32_t key, int32_t jj) { run[t].take(key, jj); });
#pragma unroll
    for (int t = 0; t < DESC_QT; ++t) {
      const int q = q0 + 16 * t + c;
      const DescTop2 T = desc_run_finish(run[t], q < nq ? qn[q] : 0);  // (a padding row's result is not stored)
      if (g == 0 && q < nq) out[q] = T;
    }
  }
}

// The guided pass: the top-2 over the candidates a pair homography admits (the header's predicate), a radius search instead of a
// masked product -- at a few pixels' radius about one candidate per query is admissible.  The grid of k_desc_top2 (blockIdx.x =
// pair * dirs + direction, blockIdx.y strided over query tiles), ONE query per thread.  The workgroup stages the other image's
// positions through LDS in tiles of DESC_G_TILE -- direction 0: B's key points as they are, the query is A's warped point;
// direction 1: A's warped points (NaN where the warp is not ok: never admissible), the query is B's key point -- and every lane scans
// them in ascending index, all lanes reading one address.  On a hit the lane forms the exact d2 from the two packed rows and their
// norms; candidates arrive in ascending j, so the dense kernel's update keeps the lowest j on a tie.  Key points are indexed by
// FEATURE (d_kp is not padded).  A pair whose found is not 1 and a query whose warp is not ok get the empty state: the chunk's state
// array is reused and k_desc_join reads all of it.  No thread leaves the tile loop before its last barrier.
__global__ __launch_bounds__(DESC_WG) void k_desc_top2_guided(const DescPair* __restrict__ pairs, int dirs, int DPW,
                                                              const uint32_t* __restrict__ desc_a, const int32_t* __restrict__ norm_a,
                                                              const uint32_t* __restrict__ desc_b, const int32_t* __restrict__ norm_b,
                                                              const float2* __restrict__ kp_a, const float2* __restrict__ kp_b,
                                                              const double* __restrict__ Hs, const int32_t* __restrict__ found, float r2f,
                                                              DescTop2* __restrict__ state)
{
  __shared__ float2 pos[DESC_G_TILE];
  const int p = blockIdx.x / dirs, dir = blockIdx.x % dirs;
  const DescPair P = pairs[p];
  const int nq = dir ? P.n_b : P.n_a, ns = dir ? P.n_a : P.n_b;
  DescTop2* out = state + P.soff + (dir ? P.n_a : 0);
  // one value per workgroup, before any barrier
  if ((found && found[p] != 1) || ns == 0) {
    for (int64_t q = (int64_t)blockIdx.y * DESC_WG + threadIdx.x; q < nq; q += (int64_t)gridDim.y * DESC_WG) out[q] = desc_top2_empty();
    return;
  }
  double H[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = Hs[9 * (int64_t)p + k];
  const uint32_t* qd = dir ? desc_b + P.row_b * DPW : desc_a + P.row_a * DPW;
  const int32_t* qn = dir ? norm_b + P.row_b : norm_a + P.row_a;
  const uint32_t* sdp = dir ? desc_a + P.row_a * DPW : desc_b + P.row_b * DPW;
  const int32_t* sn = dir ? norm_a + P.row_a : norm_b + P.row_b;
  const float2* ka = kp_a + P.kp_a;
  const float2* kb = kp_b + P.kp_b;
  const float qnan = __int_as_float(0x7fc00000);

  for (int64_t tile = blockIdx.y; tile * DESC_WG < nq; tile += gridDim.y) {
    const int64_t q = tile * DESC_WG + threadIdx.x;
    bool scan = q < nq;  // (a lane without a query, or whose warp is not ok, stages and waits with the others)
    float qx = 0.f, qy = 0.f;
    if (scan) {
      if (dir == 0) {
        const float2 a = ka[q];
        const DescWarp w = desc_guide_warp(H, a.x, a.y);
        scan = w.ok; qx = w.x; qy = w.y;
      }
      else {
        const float2 b = kb[q];
        qx = b.x; qy = b.y;
      }
    }
    DescRun run;
    for (int s0 = 0; s0 < ns; s0 += DESC_G_TILE) {
      const int cnt = min(DESC_G_TILE, ns - s0), cntu = (cnt + DESC_G_UNROLL - 1) & ~(DESC_G_UNROLL - 1);  // the tail: never admissible
      __syncthreads();  // the tile before this one has been scanned
      for (int k = threadIdx.x; k < cntu; k += DESC_WG) {
        float2 v = make_float2(qnan, qnan);
        if (k < cnt) {
          if (dir == 0) v = kb[s0 + k];
          else {
            const float2 a = ka[s0 + k];
            const DescWarp w = desc_guide_warp(H, a.x, a.y);
            if (w.ok) v = make_float2(w.x, w.y);
          }
        }
        pos[k] = v;
      }
      __syncthreads();
      if (scan) {
        for (int k0 = 0; k0 < cntu; k0 += DESC_G_UNROLL) {
          float e2[DESC_G_UNROLL], least = __int_as_float(0x7f800000);  // +inf
#pragma unroll
          for (int u = 0; u < DESC_G_UNROLL; ++u) {
            // one form for both directions: (q - c) is exactly -(c - q), so the squares and their sum are the header's bits
            // whichever of the two is the warped point -- and the loop has no branch on the direction
            const float2 c = pos[k0 + u];
            e2[u] = desc_guide_err2(qx, qy, c.x, c.y);
            least = fminf(least, e2[u]);  // (fminf drops a NaN: an error that is NaN never looks like a hit)
          }
          if (!(least <= r2f)) continue;  // no hit among these: the common case costs one comparison, not one per candidate
#pragma unroll
          for (int u = 0; u < DESC_G_UNROLL; ++u) {
            if (!(e2[u] <= r2f)) continue;
            const int32_t j = s0 + k0 + u;
            const uint32_t* x = qd + q * DPW;
            const uint32_t* y = sdp + (int64_t)j * DPW;
            int32_t dot = 0;
            for (int w = 0; w < DPW; ++w) dot += desc_dot_i8x4(x[w], y[w]);
            run.take(qn[q] + sn[j] - 2 * dot, j);
          }
        }
      }
    }
    if (q < nq) out[q] = DescTop2{run.bd, run.bj, run.sd};
  }
}

// The guided pass over a grid (ptz_desc_grid.h): the contract, the launch grid and the empty states of k_desc_top2_guided, but a
// query tests only the candidates of the cells its reach touches, and the distance of a hit is computed by the wave.
//   index   per slab of at most kDescGridSlab searched positions (direction 0: B's key points, direction 1: A's warped points, NaN
//           where the warp is not ok): every thread keeps its DESC_GRID_PER positions in registers, the workgroup reduces the
//           bounding box of the finite ones, counts them per cell with LDS integer adds, scans the counts in place and scatters
//           (x, y, feature) into cell order; after the scatter cur[c] is the END of cell c, so the cells cx0 .. cx1 of a grid row are
//           the run [cur[row G + cx0 - 1], cur[row G + cx1]).  With one slab (the common case) the index is built once per workgroup.
//   search  one query per lane.  A lane walks its runs up to its next admissible candidate (the header's predicate) and stops; the
//           wave ballots the pending hits and takes them DESC_GRID_HITS(L) at a time, L = 16, 32 or 64 lanes per hit: the lanes of a
//           group read the owner's query row and candidate by lane broadcast, load the words lane, lane + L, ... of the two packed
//           rows, form desc_dot_i8x4 and sum over the group (integers: any order is exact); the owner applies
//           desc_top2_take_keyed(qn + sn - 2 dot, j).  The update is order-free, so a lane's state simply runs on through the slabs.
// Every lane of a wave takes part in every ballot and shuffle (a lane without a query, or out of candidates, has nothing pending),
// and every wave reaches every barrier: nothing between two barriers depends on a thread's own query.
constexpr int DESC_GRID_PER = kDescGridSlab / DESC_WG;  // positions of a slab per thread
constexpr int DESC_GRID_CELLS = kDescGridG * kDescGridG;
constexpr unsigned DESC_GRID_ROWS_FULL = 4096;  // rows of the launch grid from which one workgroup per row takes all its query tiles
static_assert(kDescGridSlab % DESC_WG == 0 && DESC_GRID_CELLS % DESC_WG == 0, "a slab and the cells divide among the threads");

template <int L>  // lanes per hit
__global__ __launch_bounds__(DESC_WG) void k_desc_top2_guided_grid(const DescPair* __restrict__ pairs, int dirs, int DPW,
                                                                   const uint32_t* __restrict__ desc_a, const int32_t* __restrict__ norm_a,
                                                                   const uint32_t* __restrict__ desc_b, const int32_t* __restrict__ norm_b,
                                                                   const float2* __restrict__ kp_a, const float2* __restrict__ kp_b,
                                                                   const double* __restrict__ Hs, const int32_t* __restrict__ found, float r2f,
                                                                   double reach, DescTop2* __restrict__ state)
{
  constexpr int HITS = WAVE / L;                  // hits of one wave step
  constexpr int CPT = DESC_GRID_CELLS / DESC_WG;  // cells per thread in the scan
  __shared__ float2 pos[kDescGridSlab];           // the slab's finite positions in cell order
  __shared__ int32_t feat[kDescGridSlab];         // their features
  __shared__ int32_t cur[DESC_GRID_CELLS];        // counts -> starts -> ends
  __shared__ float box[4][DESC_WG / WAVE];
  __shared__ int32_t wsum[DESC_WG / WAVE];
  const int p = blockIdx.x / dirs, dir = blockIdx.x % dirs;
  const DescPair P = pairs[p];
  const int nq = dir ? P.n_b : P.n_a, ns = dir ? P.n_a : P.n_b;
  DescTop2* out = state + P.soff + (dir ? P.n_a : 0);
  // one value per workgroup, before any barrier
  if ((found && found[p] != 1) || ns == 0) {
    for (int64_t q = (int64_t)blockIdx.y * DESC_WG + threadIdx.x; q < nq; q += (int64_t)gridDim.y * DESC_WG) out[q] = desc_top2_empty();
    return;
  }
  double H[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = Hs[9 * (int64_t)p + k];
  const uint32_t* qd = dir ? desc_b + P.row_b * DPW : desc_a + P.row_a * DPW;
  const int32_t* qn = dir ? norm_b + P.row_b : norm_a + P.row_a;
  const uint32_t* sdp = dir ? desc_a + P.row_a * DPW : desc_b + P.row_b * DPW;
  const int32_t* sn = dir ? norm_a + P.row_a : norm_b + P.row_b;
  const float2* ka = kp_a + P.kp_a;
  const float2* kb = kp_b + P.kp_b;
  const float qnan = __int_as_float(0x7fc00000), finf = __int_as_float(0x7f800000);
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, sub = lane / L, wl = lane % L;
  const bool one_slab = ns <= kDescGridSlab;
  DescGridFrame F;
  bool built = false;

  for (int64_t tile = blockIdx.y; tile * DESC_WG < nq; tile += gridDim.y) {
    const int64_t q = tile * DESC_WG + threadIdx.x;
    bool ask = q < nq;  // (a lane without a query, or whose warp is not ok, builds the index and answers the ballots with the others)
    float qx = 0.f, qy = 0.f;
    if (ask) {
      if (dir == 0) {
        const float2 a = ka[q];
        const DescWarp w = desc_guide_warp(H, a.x, a.y);
        ask = w.ok; qx = w.x; qy = w.y;
      }
      else {
        const float2 b = kb[q];
        qx = b.x; qy = b.y;
      }
      ask = ask && desc_grid_indexed(qx, qy);
    }
    const int32_t my_qn = q < nq ? qn[q] : 0;
    DescTop2 T = desc_top2_empty();
    for (int s0 = 0; s0 < ns; s0 += kDescGridSlab) {
      if (!(one_slab && built)) {
        const int cnt = min(kDescGridSlab, ns - s0);
        // the slab's positions, DESC_GRID_PER per thread in registers; the bounding box of the finite ones
        float px[DESC_GRID_PER], py[DESC_GRID_PER];
        float x0 = finf, x1 = -finf, y0 = finf, y1 = -finf;
#pragma unroll
        for (int u = 0; u < DESC_GRID_PER; ++u) {
          const int k = u * DESC_WG + threadIdx.x;
          float2 v = make_float2(qnan, qnan);
          if (k < cnt) {
            if (dir == 0) v = kb[s0 + k];
            else {
              const float2 a = ka[s0 + k];
              const DescWarp w = desc_guide_warp(H, a.x, a.y);
              if (w.ok) v = make_float2(w.x, w.y);
            }
          }
          if (!desc_grid_indexed(v.x, v.y)) v.x = qnan;  // px is NaN <=> the position is not indexed
          px[u] = v.x; py[u] = v.y;
          if (v.x == v.x) { x0 = fminf(x0, v.x); x1 = fmaxf(x1, v.x); y0 = fminf(y0, v.y); y1 = fmaxf(y1, v.y); }
        }
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
          x0 = fminf(x0, __shfl_xor(x0, d)); x1 = fmaxf(x1, __shfl_xor(x1, d));
          y0 = fminf(y0, __shfl_xor(y0, d)); y1 = fmaxf(y1, __shfl_xor(y1, d));
        }
        __syncthreads();  // the slab before this one has been searched
        if (lane == 0) { box[0][wave] = x0; box[1][wave] = x1; box[2][wave] = y0; box[3][wave] = y1; }
#pragma unroll
        for (int u = 0; u < CPT; ++u) cur[u * DESC_WG + threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < DESC_WG / WAVE; ++w) {
          x0 = fminf(x0, box[0][w]); x1 = fmaxf(x1, box[1][w]); y0 = fminf(y0, box[2][w]); y1 = fmaxf(y1, box[3][w]);
        }
        F = desc_grid_frame(x0, x1, y0, y1, reach);
        // counts per cell
        int cell[DESC_GRID_PER];
#pragma unroll
        for (int u = 0; u < DESC_GRID_PER; ++u) {
          cell[u] = -1;
          if (px[u] == px[u]) {
            cell[u] = desc_grid_cell(F, 1, (double)py[u]) * kDescGridG + desc_grid_cell(F, 0, (double)px[u]);
            atomicAdd(&cur[cell[u]], 1);
          }
        }
        __syncthreads();
        // exclusive scan in place: thread t owns the cells CPT t .. CPT t + CPT - 1
        int c[CPT], sum = 0;
#pragma unroll
        for (int u = 0; u < CPT; ++u) { c[u] = cur[CPT * threadIdx.x + u]; sum += c[u]; }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
          const int o = __shfl_up(incl, d);
          if (lane >= d) incl += o;
        }
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        int at = incl - sum;
        for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
        for (int u = 0; u < CPT; ++u) { cur[CPT * threadIdx.x + u] = at; at += c[u]; }
        __syncthreads();
        // scatter: a cell's cursor ends at the cell's end
#pragma unroll
        for (int u = 0; u < DESC_GRID_PER; ++u)
          if (cell[u] >= 0) {
            const int at = atomicAdd(&cur[cell[u]], 1);
            pos[at] = make_float2(px[u], py[u]);
            feat[at] = s0 + u * DESC_WG + threadIdx.x;
          }
        __syncthreads();
        built = true;
      }
      // ---- search: lane state = (grid row gy, position k in its run, the run's end e) --------------------------------------------
      DescGridRange R = {0, 0, 1, 0};  // (cy0 > cy1: no row)
      if (ask && !F.empty) R = desc_grid_range(F, qx, qy, reach);
      int gy = R.cy0, k = 0, e = 0;
      bool fresh = true;  // the run of row gy has not been opened
      for (;;) {
        // up to this lane's next hit
        int32_t hit_j = -1;
        while (gy <= R.cy1) {
          if (fresh) {
            const int c0 = gy * kDescGridG + R.cx0;
            k = c0 > 0 ? cur[c0 - 1] : 0;
            e = cur[gy * kDescGridG + R.cx1];
            fresh = false;
          }
          while (k < e) {
            const float2 v = pos[k];
            const int at = k++;
            if (desc_guide_err2(qx, qy, v.x, v.y) <= r2f) { hit_j = feat[at]; break; }
          }
          if (hit_j >= 0) break;
          ++gy;
          fresh = true;
        }
        uint64_t pending = __ballot(hit_j >= 0);
        if (pending == 0) break;  // one value per wave
        while (pending) {
          // the owners of this step's groups
          int own = -1, mine = -1;  // the owner of this lane's group; the group that works for this lane
#pragma unroll
          for (int h = 0; h < HITS; ++h)
            if (pending) {
              const int o = __builtin_ctzll(pending);
              pending &= pending - 1;
              if (sub == h) own = o;
              if (lane == o) mine = h;
            }
          const int src = own >= 0 ? own : 0;
          const int64_t oq = __shfl((int)q, src);  // (q < nq <= INT32_MAX for an owner)
          const int32_t oj = __shfl(hit_j, src);
          int32_t dot = 0;
          if (own >= 0) {
            const uint32_t* x = qd + oq * DPW;
            const uint32_t* y = sdp + (int64_t)oj * DPW;
            for (int w = wl; w < DPW; w += L) dot += desc_dot_i8x4(x[w], y[w]);
          }
#pragma unroll
          for (int d = 1; d < L; d <<= 1) dot += __shfl_xor(dot, d);
          const int32_t got = __shfl(dot, (mine >= 0 ? mine : 0) * L);
          if (mine >= 0) desc_top2_take_keyed(T, my_qn + sn[hit_j] - 2 * got, hit_j);
        }
      }
    }
    if (q < nq) out[q] = T;
  }
}

// the keep byte of every feature of A
__global__ __launch_bounds__(256) void k_desc_join(const DescPair* __restrict__ pairs, const DescTop2* __restrict__ state, DescRule rule,
                                                   uint8_t* __restrict__ keep)
{
  const DescPair P = pairs[blockIdx.x];
  const DescTop2* sa = state + P.soff;
  const DescTop2* sb = sa + P.n_a;
  for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < P.n_a; i += (int64_t)gridDim.y * blockDim.x) {
    const DescTop2 ta = sa[i];
    DescTop2 tb = desc_top2_empty();
    if (rule.cross_check && ta.j != kDescNone) tb = sb[ta.j];
    keep[P.aoff + i] = desc_accept(rule, (int32_t)i, ta, tb) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_desc_fill(int n, int32_t v, int32_t* __restrict__ x)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}

// one thread per kept match of the chunk: its pair by bisection of the chunk's offsets, then the match's five outputs
__global__ __launch_bounds__(256) void k_desc_gather(int n_pair, const DescPair* __restrict__ pairs, const int64_t* __restrict__ out_ptr,
                                                     const int32_t* __restrict__ out_index, const DescTop2* __restrict__ state,
                                                     const float2* __restrict__ kp_a, const float2* __restrict__ kp_b,
                                                     int32_t* __restrict__ idx_a, int32_t* __restrict__ idx_b, int32_t* __restrict__ dist2,
                                                     float2* __restrict__ uv_a, float2* __restrict__ uv_b)
{
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= out_ptr[n_pair]) return;
  int lo = 0, hi = n_pair;  // the last p with out_ptr[p] <= o
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_ptr[mid] <= o) lo = mid;
    else hi = mid;
  }
  const DescPair P = pairs[lo];
  const int32_t i = (int32_t)(out_index[o] - P.aoff);
  const DescTop2 ta = state[P.soff + i];
  idx_a[o] = i;
  idx_b[o] = ta.j;
  dist2[o] = ta.d;
  if (uv_a) {
    uv_a[o] = kp_a[P.kp_a + i];
    uv_b[o] = kp_b[P.kp_b + ta.j];
  }
}

template <bool DUMP>
void launch_top2(int KS, dim3 grid, hipStream_t st, const DescPair* pairs, int dirs, const int8_t* da, const int32_t* na, const int8_t* db,
                 const int32_t* nb, DescTop2* state, int32_t* dump)
{
  PTZ_DESC_FOR_KS(KS, hipLaunchKernelGGL((k_desc_top2<K, DUMP>), grid, dim3(DESC_WG), 0, st, pairs, dirs, da, na, db, nb, state, dump));
}

inline unsigned tiles_y(int64_t n, int per) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n + per - 1) / per, 1), 65535); }

// the five arrays of n matches as slots of a block (a chunk's part, the result): the pixels only where both sets have key points
struct MatchArrays {
  size_t o_ia, o_ib, o_d2, o_ua, o_ub;
  bool has_uv;
  MatchArrays(BlockLayout& b, int64_t n, bool uv) : has_uv(uv)
  {
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    o_ia = b.take(sizeof(int32_t) * m); o_ib = b.take(sizeof(int32_t) * m); o_d2 = b.take(sizeof(int32_t) * m);
    o_ua = b.take(uv ? sizeof(float2) * m : 0); o_ub = b.take(uv ? sizeof(float2) * m : 0);
  }
  int32_t* idx_a(char* p) const { return (int32_t*)(p + o_ia); }
  int32_t* idx_b(char* p) const { return (int32_t*)(p + o_ib); }
  int32_t* dist2(char* p) const { return (int32_t*)(p + o_d2); }
  float2* uv_a(char* p) const { return has_uv ? (float2*)(p + o_ua) : nullptr; }
  float2* uv_b(char* p) const { return has_uv ? (float2*)(p + o_ub) : nullptr; }
};

}  // namespace
}  // namespace ptz

struct ptz_desc_matches {
  int device = 0;
  int32_t n_pair = 0, n_chunks = 0;
  int64_t n_match = 0;
  double device_ms = 0;
  bool has_uv = false;
  std::vector<int64_t> match_ptr;  // [n_pair + 1]
  ptz::PoolBlock blk;
  int64_t* d_match_ptr = nullptr;
  int32_t *d_idx_a = nullptr, *d_idx_b = nullptr, *d_dist2 = nullptr;
  float2 *d_uv_a = nullptr, *d_uv_b = nullptr;
};

extern "C" void ptz_desc_options_default(ptz_desc_options* o)
{
  if (!o) return;
  o->ratio = 0.8;
  o->max_dist2 = 0;
  o->cross_check = 1;
  o->min_matches = 0;
  o->device_id = 0;
  o->workspace_bytes = (int64_t)256 << 20;
}

extern "C" int32_t ptz_desc_set_create(int32_t n_img, const int64_t* feat_ptr, const uint8_t* desc, int32_t D, const float* kp_xy,
                                       int32_t device_id, ptz_desc_set** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (n_img < 0 || !feat_ptr || feat_ptr[0] != 0 || D < 1 || D > kDescMaxDim || device_id < 0) return PTZ_EINVAL;
  for (int m = 0; m < n_img; ++m)
    if (feat_ptr[m + 1] < feat_ptr[m]) return PTZ_EINVAL;
  for (int m = 0; m < n_img; ++m)
    if (feat_ptr[m + 1] - feat_ptr[m] > INT32_MAX) return PTZ_ELIMIT;
  const int64_t nf = feat_ptr[n_img];
  if (nf > 0 && !desc) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);

  std::unique_ptr<ptz_desc_set> s(new ptz_desc_set());
  s->device = device_id; s->n_img = n_img; s->D = D; s->KS = (D + 63) / 64; s->n_feat = nf;
  s->feat_ptr.assign(feat_ptr, feat_ptr + n_img + 1);
  s->row_off.resize(n_img + 1);
  s->row_off[0] = 0;
  for (int m = 0; m < n_img; ++m)
    s->row_off[m + 1] = s->row_off[m] + (feat_ptr[m + 1] - feat_ptr[m] + DESC_ROW_PAD - 1) / DESC_ROW_PAD * DESC_ROW_PAD;
  const int DP = 64 * s->KS;
  const size_t rows = (size_t)s->row_off[n_img] + DESC_ROW_PAD;  // the slack is the pack kernel's image n_img
  BlockLayout b;
  const size_t o_desc = b.take(rows * DP), o_norm = b.take(rows * sizeof(int32_t)), o_kp = b.take(kp_xy ? (size_t)nf * sizeof(float2) : 0),
               o_fp = b.take(sizeof(int64_t) * ((size_t)n_img + 2)), o_ro = b.take(sizeof(int64_t) * ((size_t)n_img + 2));
  if (s->blk.get(device_id, b.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  s->d_desc = (int8_t*)(s->blk.p + o_desc);
  s->d_norm = (int32_t*)(s->blk.p + o_norm);
  s->d_kp = kp_xy ? (float2*)(s->blk.p + o_kp) : nullptr;
  s->d_feat_ptr = (const int64_t*)(s->blk.p + o_fp);
  s->d_row_off = (const int64_t*)(s->blk.p + o_ro);

  // the two offset tables stay with the set (the pack kernel's "image" n_img is the slack); the raw bytes are the pack kernel's only
  std::vector<int64_t> fp(s->feat_ptr), ro(s->row_off);
  fp.push_back(nf);
  ro.push_back((int64_t)rows);
  CallHeld h;  // (declared after the set: the stream is waited for before a set that is not returned gives its block back)
  if (const int32_t rc = h.acquire(device_id, (size_t)nf * D)) { (void)hipGetLastError(); return rc; }
  PTZ_HIP_TRY(hipMemcpyAsync(s->blk.p + o_fp, fp.data(), sizeof(int64_t) * fp.size(), hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(s->blk.p + o_ro, ro.data(), sizeof(int64_t) * ro.size(), hipMemcpyHostToDevice, h.st));
  if (nf > 0) PTZ_HIP_TRY(hipMemcpyAsync(h.base, desc, (size_t)nf * D, hipMemcpyHostToDevice, h.st));
  if (nf > 0 && kp_xy) PTZ_HIP_TRY(hipMemcpyAsync(s->d_kp, kp_xy, (size_t)nf * sizeof(float2), hipMemcpyHostToDevice, h.st));
  int64_t most = DESC_ROW_PAD;
  for (int m = 0; m < n_img; ++m) most = std::max(most, s->row_off[m + 1] - s->row_off[m]);
  hipLaunchKernelGGL(k_desc_pack, dim3(n_img + 1, tiles_y(most, 256)), dim3(256), 0, h.st, s->d_feat_ptr, s->d_row_off,
                     (const uint8_t*)h.base, D, DP, (uint32_t*)s->d_desc, s->d_norm);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(stream_wait(h.st));
  *out = s.release();
  return PTZ_OK;
}

extern "C" void ptz_desc_set_destroy(ptz_desc_set* s)
{
  if (!s) return;
  ptz::DeviceGuard g(s->device);
  delete s;
}

namespace ptz {
namespace {

// the guide of ptz_desc_match_pairs_guided: one H per pair, found nullable (all 1), host or device arrays
struct DescGuide {
  const double* H;
  const int32_t* found;
  bool on_device;
  double radius_px;
  bool grid;  // k_desc_top2_guided_grid in place of k_desc_top2_guided: the same arrays
};

// lanes per hit from the words of a packed row: a row of 16 or 32 words leaves room for four or two hits in one wave step
void launch_guided_grid(int DPW, dim3 grid, hipStream_t st, const DescPair* pairs, int dirs, const uint32_t* da, const int32_t* na,
                        const uint32_t* db, const int32_t* nb, const float2* ka, const float2* kb, const double* H, const int32_t* found,
                        float r2f, double reach, DescTop2* state)
{
  if (DPW <= 16)
    hipLaunchKernelGGL(k_desc_top2_guided_grid<16>, grid, dim3(DESC_WG), 0, st, pairs, dirs, DPW, da, na, db, nb, ka, kb, H, found, r2f, reach, state);
  else if (DPW <= 32)
    hipLaunchKernelGGL(k_desc_top2_guided_grid<32>, grid, dim3(DESC_WG), 0, st, pairs, dirs, DPW, da, na, db, nb, ka, kb, H, found, r2f, reach, state);
  else
    hipLaunchKernelGGL(k_desc_top2_guided_grid<64>, grid, dim3(DESC_WG), 0, st, pairs, dirs, DPW, da, na, db, nb, ka, kb, H, found, r2f, reach, state);
}

// the chunk loop of both matchers; guide = nullptr: the dense pass
int32_t desc_match_run(const char* who, const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair, const int32_t* img_a,
                       const int32_t* img_b, const DescGuide* guide, const ptz_desc_options* opt, ptz_desc_matches** out)
{
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  ptz_desc_options o;
  if (const int32_t rc = desc_options_check(A, B, opt, &o)) return rc;
  if (n_pair < 0 || (n_pair > 0 && (!img_a || !img_b))) return PTZ_EINVAL;
  for (int p = 0; p < n_pair; ++p)
    if (img_a[p] < 0 || img_a[p] >= A->n_img || img_b[p] < 0 || img_b[p] >= B->n_img) return PTZ_EINVAL;
  if (guide) {
    if ((A->n_feat > 0 && !A->d_kp) || (B->n_feat > 0 && !B->d_kp) || (n_pair > 0 && !guide->H)) return PTZ_EINVAL;
    if (!(std::isfinite(guide->radius_px) && guide->radius_px > 0)) return PTZ_EINVAL;
  }
  const float r2f = guide ? (float)(guide->radius_px * guide->radius_px) : 0.f;
  // (an r2f that is not finite admits every pair whose error is not NaN, infinite positions included: no grid serves that)
  const bool grid = guide && guide->grid && std::isfinite(r2f);
  clear_stale_error(who);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= A->device) return PTZ_ENODEVICE;
  const int dev = A->device;
  PTZ_DEVICE_GUARD(dev);

  std::unique_ptr<ptz_desc_matches> res(new ptz_desc_matches());
  res->device = dev; res->n_pair = n_pair; res->has_uv = A->d_kp && B->d_kp;
  res->match_ptr.assign((size_t)n_pair + 1, 0);
  const DescRule rule = {o.ratio * o.ratio, o.max_dist2, o.cross_check ? 1 : 0};
  const int dirs = rule.cross_check ? 2 : 1;

  // the pair table, offsets relative to each pair's chunk; chunks = runs of pairs whose state and keep bytes stay under the bound
  std::vector<DescPair> tab((size_t)n_pair);
  struct Chunk { int p0, p1; int64_t n_state, n_a; int most_q; };
  std::vector<Chunk> chunks;
  {
    Chunk c = {0, 0, 0, 0, 0};
    int64_t bytes = 0;
    for (int p = 0; p < n_pair; ++p) {
      const int ia = img_a[p], ib = img_b[p];
      const int64_t na = A->feat_ptr[ia + 1] - A->feat_ptr[ia], nb = B->feat_ptr[ib + 1] - B->feat_ptr[ib];
      const int64_t cost = (int64_t)sizeof(DescTop2) * (na + nb) + na;
      if (c.p1 > c.p0 && (bytes + cost > o.workspace_bytes || c.n_a + na > INT32_MAX || c.p1 - c.p0 >= DESC_CHUNK_PAIRS)) {
        chunks.push_back(c);
        c = {p, p, 0, 0, 0};
        bytes = 0;
      }
      tab[p] = DescPair{A->row_off[ia], B->row_off[ib], A->feat_ptr[ia], B->feat_ptr[ib], c.n_state, c.n_a, (int32_t)na, (int32_t)nb};
      c.n_state += na + nb;
      c.n_a += na;
      c.most_q = (int)std::max<int64_t>(c.most_q, std::max(na, nb));
      c.p1 = p + 1;
      bytes += cost;
    }
    if (c.p1 > c.p0) chunks.push_back(c);
  }
  res->n_chunks = (int32_t)chunks.size();
  int64_t ws_state = 1, ws_a = 1;
  int ws_pairs = 1;
  for (const Chunk& c : chunks) {
    ws_state = std::max(ws_state, c.n_state);
    ws_a = std::max(ws_a, c.n_a);
    ws_pairs = std::max(ws_pairs, c.p1 - c.p0);
  }

  const bool host_guide = guide && !guide->on_device;
  BlockLayout wl;
  const size_t o_tab = wl.take(sizeof(DescPair) * std::max<size_t>(tab.size(), 1)), o_state = wl.take(sizeof(DescTop2) * ws_state),
               o_keep = wl.take(ws_a), o_index = wl.take(sizeof(int32_t) * ws_a), o_aptr = wl.take(sizeof(int64_t) * (ws_pairs + 1)),
               o_found = wl.take(sizeof(int32_t) * ws_pairs), o_cnt = wl.take(sizeof(int32_t) * ws_pairs),
               o_optr = wl.take(sizeof(int64_t) * (ws_pairs + 1)),
               o_gh = wl.take(host_guide ? sizeof(double) * 9 * (size_t)n_pair : 0),  // a host guide's copy: H, then found, of ALL pairs
               o_gf = wl.take(host_guide && guide->found ? sizeof(int32_t) * (size_t)n_pair : 0);
  // a chunk's matches wait in a block of their own until the total is known
  struct Part { PoolBlock blk; int64_t n; };
  // The ordering rule: on every return the stream is waited for before any block its kernels write goes back to the pool.  h's
  // destructor waits and then releases the workspace; the parts and the result (res, above) are declared before h, so they go after.
  std::vector<Part> parts;
  std::vector<int64_t> aptr, optr;  // a chunk's offsets, up and down
  CallHeld h;
  if (const int32_t rc = h.acquire(dev, wl.total())) { (void)hipGetLastError(); return rc; }
  char* const ws = h.base;
  DescPair* d_tab = (DescPair*)(ws + o_tab);
  DescTop2* d_state = (DescTop2*)(ws + o_state);
  uint8_t* d_keep = (uint8_t*)(ws + o_keep);
  int32_t* d_index = (int32_t*)(ws + o_index);
  int64_t* d_aptr = (int64_t*)(ws + o_aptr);
  int32_t* d_found = (int32_t*)(ws + o_found);
  int32_t* d_cnt = (int32_t*)(ws + o_cnt);
  int64_t* d_optr = (int64_t*)(ws + o_optr);
  if (n_pair > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof(DescPair) * tab.size(), hipMemcpyHostToDevice, h.st));
    hipLaunchKernelGGL(k_desc_fill, dim3((ws_pairs + 255) / 256), dim3(256), 0, h.st, ws_pairs, 1, d_found);
  }
  const double* g_H = guide ? guide->H : nullptr;
  const int32_t* g_found = guide ? guide->found : nullptr;
  if (host_guide && n_pair > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(ws + o_gh, guide->H, sizeof(double) * 9 * (size_t)n_pair, hipMemcpyHostToDevice, h.st));
    g_H = (const double*)(ws + o_gh);
    if (guide->found) {
      PTZ_HIP_TRY(hipMemcpyAsync(ws + o_gf, guide->found, sizeof(int32_t) * (size_t)n_pair, hipMemcpyHostToDevice, h.st));
      g_found = (const int32_t*)(ws + o_gf);
    }
  }

  double ms_sum = 0;
  for (const Chunk& c : chunks) {
    const int npc = c.p1 - c.p0;
    aptr.resize(npc + 1);
    for (int p = 0; p < npc; ++p) aptr[p] = tab[c.p0 + p].aoff;
    aptr[npc] = c.n_a;
    PTZ_HIP_TRY(hipMemcpyAsync(d_aptr, aptr.data(), sizeof(int64_t) * (npc + 1), hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
    if (grid) {
      // the index of a (pair, direction) is built by every workgroup of its column: few of them once the rows fill the device
      const unsigned rows = (unsigned)npc * dirs, gy = std::min(tiles_y(c.most_q, DESC_WG), std::max(1u, DESC_GRID_ROWS_FULL / rows));
      launch_guided_grid(16 * A->KS, dim3(rows, gy), h.st, (const DescPair*)(d_tab + c.p0), dirs, (const uint32_t*)A->d_desc,
                         (const int32_t*)A->d_norm, (const uint32_t*)B->d_desc, (const int32_t*)B->d_norm, (const float2*)A->d_kp,
                         (const float2*)B->d_kp, g_H + 9 * (size_t)c.p0, g_found ? g_found + c.p0 : nullptr, r2f,
                         desc_grid_reach(guide->radius_px), d_state);
    }
    else if (guide)
      hipLaunchKernelGGL(k_desc_top2_guided, dim3((unsigned)npc * dirs, tiles_y(c.most_q, DESC_WG)), dim3(DESC_WG), 0, h.st,
                         (const DescPair*)(d_tab + c.p0), dirs, 16 * A->KS, (const uint32_t*)A->d_desc, (const int32_t*)A->d_norm,
                         (const uint32_t*)B->d_desc, (const int32_t*)B->d_norm, (const float2*)A->d_kp, (const float2*)B->d_kp,
                         g_H + 9 * (size_t)c.p0, g_found ? g_found + c.p0 : nullptr, r2f, d_state);
    else
      launch_top2<false>(A->KS, dim3((unsigned)npc * dirs, tiles_y(c.most_q, DESC_WG_Q)), h.st, d_tab + c.p0, dirs, A->d_desc, A->d_norm,
                         B->d_desc, B->d_norm, d_state, nullptr);
    hipLaunchKernelGGL(k_desc_join, dim3(npc, tiles_y(c.most_q, 256)), dim3(256), 0, h.st, (const DescPair*)(d_tab + c.p0),
                       (const DescTop2*)d_state, rule, d_keep);
    enqueue_compact(npc, d_aptr, d_found, d_keep, o.min_matches, d_cnt, d_optr, nullptr, nullptr, nullptr, nullptr, d_index, h.st);
    PTZ_HIP_TRY(hipGetLastError());
    PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
    optr.resize(npc + 1);
    PTZ_HIP_TRY(hipMemcpyAsync(optr.data(), d_optr, sizeof(int64_t) * (npc + 1), hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(stream_wait(h.st));
    ms_sum += h.elapsed_ms();
    const int64_t nc = optr[npc], base = res->match_ptr[c.p0];
    for (int p = 0; p < npc; ++p) res->match_ptr[c.p0 + p + 1] = base + optr[p + 1];
    parts.emplace_back();
    Part& part = parts.back();
    part.n = nc;
    BlockLayout pl;
    const MatchArrays pa(pl, nc, res->has_uv);
    if (part.blk.get(dev, pl.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
    if (nc > 0) {
      char* const pp = part.blk.p;
      PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
      hipLaunchKernelGGL(k_desc_gather, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h.st, npc, (const DescPair*)(d_tab + c.p0),
                         (const int64_t*)d_optr, (const int32_t*)d_index, (const DescTop2*)d_state, (const float2*)A->d_kp,
                         (const float2*)B->d_kp, pa.idx_a(pp), pa.idx_b(pp), pa.dist2(pp), pa.uv_a(pp), pa.uv_b(pp));
      PTZ_HIP_TRY(hipGetLastError());
      PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
      PTZ_HIP_TRY(stream_wait(h.st));
      ms_sum += h.elapsed_ms();
    }
  }

  // one block behind the result: the offsets, then the five arrays, chunk after chunk
  const int64_t nm = res->match_ptr[n_pair];
  res->n_match = nm;
  res->device_ms = ms_sum;
  BlockLayout rl;
  const size_t o_ptr = rl.take(sizeof(int64_t) * ((size_t)n_pair + 1));
  const MatchArrays ra(rl, nm, res->has_uv);
  if (res->blk.get(dev, rl.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  char* const rp = res->blk.p;
  res->d_match_ptr = (int64_t*)(rp + o_ptr);
  res->d_idx_a = ra.idx_a(rp); res->d_idx_b = ra.idx_b(rp); res->d_dist2 = ra.dist2(rp); res->d_uv_a = ra.uv_a(rp); res->d_uv_b = ra.uv_b(rp);
  PTZ_HIP_TRY(hipMemcpyAsync(res->d_match_ptr, res->match_ptr.data(), sizeof(int64_t) * ((size_t)n_pair + 1), hipMemcpyHostToDevice, h.st));
  int64_t at = 0;
  for (const Part& part : parts) {
    if (part.n == 0) continue;
    BlockLayout pl;
    const MatchArrays pa(pl, part.n, res->has_uv);
    char* const pp = part.blk.p;
    PTZ_HIP_TRY(hipMemcpyAsync(res->d_idx_a + at, pa.idx_a(pp), sizeof(int32_t) * part.n, hipMemcpyDeviceToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(res->d_idx_b + at, pa.idx_b(pp), sizeof(int32_t) * part.n, hipMemcpyDeviceToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(res->d_dist2 + at, pa.dist2(pp), sizeof(int32_t) * part.n, hipMemcpyDeviceToDevice, h.st));
    if (res->has_uv) {
      PTZ_HIP_TRY(hipMemcpyAsync(res->d_uv_a + at, pa.uv_a(pp), sizeof(float2) * part.n, hipMemcpyDeviceToDevice, h.st));
      PTZ_HIP_TRY(hipMemcpyAsync(res->d_uv_b + at, pa.uv_b(pp), sizeof(float2) * part.n, hipMemcpyDeviceToDevice, h.st));
    }
    at += part.n;
  }
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  *out = res.release();
  return PTZ_OK;
}

}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_desc_match_pairs(const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair, const int32_t* img_a,
                                        const int32_t* img_b, const ptz_desc_options* opt, ptz_desc_matches** out)
{
  return ptz::desc_match_run(__func__, A, B, n_pair, img_a, img_b, nullptr, opt, out);
}

extern "C" int32_t ptz_desc_match_pairs_guided(const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair, const int32_t* img_a,
                                               const int32_t* img_b, const double* H, const int32_t* found, double radius_px,
                                               const ptz_desc_options* opt, ptz_desc_matches** out)
{
  const ptz::DescGuide g = {H, found, false, radius_px, false};
  return ptz::desc_match_run(__func__, A, B, n_pair, img_a, img_b, &g, opt, out);
}

extern "C" int32_t ptz_desc_match_pairs_guided_grid(const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair, const int32_t* img_a,
                                                    const int32_t* img_b, const double* H, const int32_t* found, double radius_px,
                                                    const ptz_desc_options* opt, ptz_desc_matches** out)
{
  const ptz::DescGuide g = {H, found, false, radius_px, true};
  return ptz::desc_match_run(__func__, A, B, n_pair, img_a, img_b, &g, opt, out);
}

extern "C" int32_t ptz_desc_match_pairs_guided_device(const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair, const int32_t* img_a,
                                                      const int32_t* img_b, const double* d_H, const int32_t* d_found, double radius_px,
                                                      const ptz_desc_options* opt, ptz_desc_matches** out)
{
  const ptz::DescGuide g = {d_H, d_found, true, radius_px, false};
  return ptz::desc_match_run(__func__, A, B, n_pair, img_a, img_b, &g, opt, out);
}

extern "C" int32_t ptz_desc_match_pairs_guided_grid_device(const ptz_desc_set* A, const ptz_desc_set* B, int32_t n_pair,
                                                           const int32_t* img_a, const int32_t* img_b, const double* d_H,
                                                           const int32_t* d_found, double radius_px, const ptz_desc_options* opt,
                                                           ptz_desc_matches** out)
{
  const ptz::DescGuide g = {d_H, d_found, true, radius_px, true};
  return ptz::desc_match_run(__func__, A, B, n_pair, img_a, img_b, &g, opt, out);
}

extern "C" int64_t ptz_desc_matches_n_matches(const ptz_desc_matches* m) { return m ? m->n_match : 0; }
extern "C" int32_t ptz_desc_matches_n_pairs(const ptz_desc_matches* m) { return m ? m->n_pair : 0; }
extern "C" double ptz_desc_matches_device_ms(const ptz_desc_matches* m) { return m ? m->device_ms : 0.0; }
extern "C" int32_t ptz_desc_matches_n_chunks(const ptz_desc_matches* m) { return m ? m->n_chunks : 0; }

extern "C" int32_t ptz_desc_matches_download(const ptz_desc_matches* m, int64_t* match_ptr, int32_t* idx_a, int32_t* idx_b, int32_t* dist2,
                                             float* uv_a, float* uv_b)
{
  using namespace ptz;
  if (!m || ((uv_a || uv_b) && !m->has_uv)) return PTZ_EINVAL;
  if (match_ptr) memcpy(match_ptr, m->match_ptr.data(), sizeof(int64_t) * m->match_ptr.size());
  const int64_t n = m->n_match;
  if (n == 0 || !(idx_a || idx_b || dist2 || uv_a || uv_b)) return PTZ_OK;
  PTZ_DEVICE_GUARD(m->device);
  CallHeld h;
  if (const int32_t rc = h.open(m->device)) return rc;
  if (idx_a) PTZ_HIP_TRY(hipMemcpyAsync(idx_a, m->d_idx_a, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h.st));
  if (idx_b) PTZ_HIP_TRY(hipMemcpyAsync(idx_b, m->d_idx_b, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h.st));
  if (dist2) PTZ_HIP_TRY(hipMemcpyAsync(dist2, m->d_dist2, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h.st));
  if (uv_a) PTZ_HIP_TRY(hipMemcpyAsync(uv_a, m->d_uv_a, sizeof(float2) * n, hipMemcpyDeviceToHost, h.st));
  if (uv_b) PTZ_HIP_TRY(hipMemcpyAsync(uv_b, m->d_uv_b, sizeof(float2) * n, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  return PTZ_OK;
}

extern "C" int32_t ptz_desc_matches_device_ptrs(const ptz_desc_matches* m, const int64_t** d_match_ptr, const int32_t** d_idx_a,
                                                const int32_t** d_idx_b, const int32_t** d_dist2, const float** d_uv_a, const float** d_uv_b)
{
  if (!m) return PTZ_EINVAL;
  if (d_match_ptr) *d_match_ptr = m->d_match_ptr;
  if (d_idx_a) *d_idx_a = m->d_idx_a;
  if (d_idx_b) *d_idx_b = m->d_idx_b;
  if (d_dist2) *d_dist2 = m->d_dist2;
  if (d_uv_a) *d_uv_a = (const float*)m->d_uv_a;
  if (d_uv_b) *d_uv_b = (const float*)m->d_uv_b;
  return PTZ_OK;
}

extern "C" void ptz_desc_matches_destroy(ptz_desc_matches* m)
{
  if (!m) return;
  ptz::DeviceGuard g(m->device);
  delete m;
}

extern "C" int32_t ptz_debug_desc_dist2(const ptz_desc_set* A, int32_t img_a, const ptz_desc_set* B, int32_t img_b, int32_t* out)
{
  using namespace ptz;
  if (!A || !B || A->device != B->device || A->D != B->D) return PTZ_EINVAL;
  if (img_a < 0 || img_a >= A->n_img || img_b < 0 || img_b >= B->n_img) return PTZ_EINVAL;
  const int64_t na = A->feat_ptr[img_a + 1] - A->feat_ptr[img_a], nb = B->feat_ptr[img_b + 1] - B->feat_ptr[img_b];
  if (na * nb == 0) return PTZ_OK;
  if (!out) return PTZ_EINVAL;
  if (na * nb > INT32_MAX) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= A->device) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(A->device);
  const DescPair P = {A->row_off[img_a], B->row_off[img_b], 0, 0, 0, 0, (int32_t)na, (int32_t)nb};
  BlockLayout b;
  const size_t o_pair = b.take(sizeof(DescPair)), o_dump = b.take(sizeof(int32_t) * (size_t)(na * nb));
  CallHeld h;
  if (const int32_t rc = h.acquire(A->device, b.total())) { (void)hipGetLastError(); return rc; }
  char* const ws = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(ws + o_pair, &P, sizeof(P), hipMemcpyHostToDevice, h.st));
  launch_top2<true>(A->KS, dim3(1, tiles_y(na, DESC_WG_Q)), h.st, (const DescPair*)(ws + o_pair), 1, A->d_desc, A->d_norm, B->d_desc, B->d_norm,
                    nullptr, (int32_t*)(ws + o_dump));
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipMemcpyAsync(out, ws + o_dump, sizeof(int32_t) * (size_t)(na * nb), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  return PTZ_OK;
}
