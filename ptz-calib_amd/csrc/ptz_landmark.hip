// ptz_landmark.hip -- the landmark map on the device (gfx950): one unit ray and one aggregated descriptor per track of the resident
// reference set, and the assembly of (map, query) matches into the solve's inputs.  The contract is ptz_landmark.h (first include:
// its fp contract(off) must precede ptz_factor.h); this file adds the launch shapes and the C-ABI, nothing the result depends on.
//
//   k_landmark_build     one wave per track.  64 views a step: a lane decides ITS view's validity and ray once, the ballot and
//                        shuffles broadcast them; every lane adds the rays in CSR order (the contract's left-to-right sum, redundantly)
//                        and strides over the packed descriptor words of each valid view, int32 byte sums in registers (two words,
//                        eight sums a lane: D <= 512).  A second sweep scores the valid views against L for the home; the arg-max
//                        is a wave reduction on (z, -position).  Results go to per-track staging with a landmark flag byte.
//   (flag bytes -> lm_track: enqueue_compact of ptz_gate_compact.h over chunks of 1024 tracks: count, scan, ballot scatter)
//   k_landmark_gather    one wave per landmark: staging -> the compacted arrays
//   k_landmark_anchor    one wave per query: home votes with LDS integer adds into [n_ref] counters, a wave arg-max on the key
//                        (count, -index), the two cameras, and the keep byte of every match under the header's transfer rule
//   (keep bytes -> out_ptr and the kept matches' positions: enqueue_compact again, the ballot + prefix-popcount scatter of the gate)
//   k_landmark_transfer  one wave per query over its kept range: transfers the match once more and writes it where the scan put it
//
// Integer atomics on LDS only; no floating-point atomics, no scratch.  A track's and a query's outputs depend on their own inputs only.
#include "ptz_landmark.h"

#include <memory>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_gate_compact.h"
#include "ptz_host_batch.h"
#include "ptz_landmark_map.h"
#include "ptz_tracks_obj.h"

namespace ptz {
namespace {

constexpr int LM_WG = 256;        // four tracks (landmarks) a workgroup
constexpr int LM_CHUNK = 1024;    // tracks of one "pair" of the flag compaction
constexpr int LM_MAX_WORDS = 128; // 512 descriptor bytes

struct LmBuildIn {
  int n_ref, n_track, D, words, dist, min_views;  // words: uint32 of a packed row (16 KS)
  const int64_t *feat_ptr, *row_off;              // the set's device tables
  const uint32_t* desc;
  const float2* kp;
  const double *cams, *R;
  const int64_t* trk_ptr;
  const int32_t *trk_img, *trk_feat;
};

// view v of the CSR: valid or not; its reference, its packed row and its unit ray
__device__ __forceinline__ bool lm_view(const LmBuildIn& a, int64_t v, int32_t* r, int64_t* row, double* ray)
{
  *r = a.trk_img[v];
  if (*r < 0 || *r >= a.n_ref) return false;
  const int32_t f = a.trk_feat[v];
  const int64_t f0 = a.feat_ptr[*r];
  if (f < 0 || f >= a.feat_ptr[*r + 1] - f0) return false;
  *row = a.row_off[*r] + f;
  const float2 p = a.kp[f0 + f];
  return landmark_view_ray(a.cams + 15 * (int64_t)*r, a.R + 9 * (int64_t)*r, a.dist, p.x, p.y, ray);
}

__global__ __launch_bounds__(LM_WG) void k_landmark_build(LmBuildIn a, uint8_t* __restrict__ flag, double* __restrict__ ray_t,
                                                          int32_t* __restrict__ home_t, int32_t* __restrict__ views_t,
                                                          uint8_t* __restrict__ desc_t)
{
  const int t = blockIdx.x * (LM_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (t >= a.n_track) return;  // (one value in the wave)
  int64_t v0 = a.trk_ptr[t], v1 = a.trk_ptr[t + 1];
  if (v0 < 0 || v1 < v0) { v0 = 0; v1 = 0; }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int32_t S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int32_t n = 0, first_r = -1;
  const int used = (a.D + 3) / 4;  // words of a row that hold descriptor bytes
  for (int64_t c = v0; c < v1; c += WAVE) {
    const int64_t v = c + lane;
    int32_t r = -1;
    int64_t row = 0;
    double ray[3] = {0.0, 0.0, 0.0};
    const bool ok = v < v1 && lm_view(a, v, &r, &row, ray);
    unsigned long long m = __ballot(ok);
    if (first_r < 0 && m) first_r = __shfl(r, __ffsll((long long)m) - 1);
    while (m) {  // (one value in the wave) the valid views of this step in CSR order
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      s0 = s0 + __shfl(ray[0], j);
      s1 = s1 + __shfl(ray[1], j);
      s2 = s2 + __shfl(ray[2], j);
      const uint32_t* rowp = a.desc + (int64_t)__shfl((long long)row, j) * a.words;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int w = lane + WAVE * k;
        if (w < used) {
          const uint32_t x = rowp[w] ^ 0x80808080u;  // packed bytes are the descriptor's minus 128
#pragma unroll
          for (int b = 0; b < 4; ++b) S[4 * k + b] += (int32_t)((x >> (8 * b)) & 255u);
        }
      }
      ++n;
    }
  }
  const double s[3] = {s0, s1, s2};
  double L[3];
  const bool lm = n >= a.min_views && n >= 1 && landmark_unit(s, L);
  if (lane == 0) flag[t] = lm ? 1 : 0;
  if (!lm) return;

  // the home: the valid view with the largest (R_r L)_z, the first in CSR order on a tie
  double bz = -__builtin_huge_val();
  int32_t bi = 0x7fffffff, br = -1;
  for (int64_t c = v0; c < v1; c += WAVE) {
    const int64_t v = c + lane;
    int32_t r = -1;
    int64_t row = 0;
    double ray[3];
    if (v < v1 && lm_view(a, v, &r, &row, ray)) {
      const double z = landmark_home_z(a.R + 9 * (int64_t)r, L);
      if (z > bz) { bz = z; bi = (int32_t)(v - v0); br = r; }
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const double oz = __shfl_xor(bz, d);
    const int32_t oi = __shfl_xor(bi, d), orr = __shfl_xor(br, d);
    if (oz > bz || (oz == bz && oi < bi)) { bz = oz; bi = oi; br = orr; }
  }
  if (lane == 0) {
    ray_t[3 * (int64_t)t] = L[0]; ray_t[3 * (int64_t)t + 1] = L[1]; ray_t[3 * (int64_t)t + 2] = L[2];
    home_t[t] = bi != 0x7fffffff ? br : first_r;
    views_t[t] = n;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = lane + WAVE * k;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (4 * w + b < a.D) desc_t[(int64_t)t * a.D + 4 * w + b] = landmark_desc_byte(S[4 * k + b], n);
  }
}

__global__ __launch_bounds__(LM_WG) void k_landmark_gather(int D, const int64_t* __restrict__ n_lm, const int32_t* __restrict__ lm_track,
                                                           const double* __restrict__ ray_t, const int32_t* __restrict__ home_t,
                                                           const int32_t* __restrict__ views_t, const uint8_t* __restrict__ desc_t,
                                                           double* __restrict__ lm_ray, int32_t* __restrict__ lm_home,
                                                           int32_t* __restrict__ lm_views, uint8_t* __restrict__ lm_desc)
{
  const int64_t j = (int64_t)blockIdx.x * (LM_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= *n_lm) return;
  const int64_t t = lm_track[j];
  if (lane < 3) lm_ray[3 * j + lane] = ray_t[3 * t + lane];
  if (lane == 0) { lm_home[j] = home_t[t]; lm_views[j] = views_t[t]; }
  for (int k = lane; k < D; k += WAVE) lm_desc[j * D + k] = desc_t[t * D + k];
}

__device__ __forceinline__ unsigned long long lm_wave_max_u64(unsigned long long v)
{
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

struct LmAsmIn {
  int n_query, n_ref, n_lm;
  int64_t n_match;
  const int64_t* match_ptr;
  const int32_t* idx_a;
  const double* lm_ray;
  const int32_t* lm_home;
  const double *cams, *R;
};

// one wave (= one workgroup) per query; dynamic LDS: n_ref int32 counters
__global__ __launch_bounds__(WAVE) void k_landmark_anchor(LmAsmIn a, const int32_t* __restrict__ query_wh, int32_t* __restrict__ anchor_ref,
                                                          int32_t* __restrict__ ok_range, uint8_t* __restrict__ keep,
                                                          double* __restrict__ cam_ref, double* __restrict__ cam_cur)
{
  extern __shared__ int32_t s_votes[];
  const int q = blockIdx.x, lane = threadIdx.x;
  for (int r = lane; r < a.n_ref; r += WAVE) s_votes[r] = 0;
  __syncthreads();
  int64_t lo = a.match_ptr[q], hi = a.match_ptr[q + 1];
  const bool ok = lo >= 0 && hi >= lo && hi <= a.n_match;
  if (!ok) { lo = 0; hi = 0; }  // (the device form does not validate: a malformed range is an empty one)
  for (int64_t i = lo + lane; i < hi; i += WAVE) {
    const int32_t r = landmark_vote(a.idx_a, a.lm_home, a.n_lm, a.n_ref, i);
    if (r >= 0) atomicAdd(&s_votes[r], 1);
  }
  __syncthreads();
  unsigned long long best = 0;
  for (int r = lane; r < a.n_ref; r += WAVE) {
    const unsigned long long key = landmark_anchor_key(s_votes[r], r);
    best = key > best ? key : best;
  }
  best = lm_wave_max_u64(best);
  const int32_t an = best ? reloc_key_pos(best) : -1;  // (one value in the wave)
  const int32_t ra = an >= 0 ? an : 0;
  if (lane == 0) {
    anchor_ref[q] = an;
    ok_range[q] = ok ? 1 : 0;
    double cr[15], cc[15];
    reloc_cameras(a.cams + 15 * (int64_t)ra, query_wh[2 * q], query_wh[2 * q + 1], 2, cr, cc);
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      cam_ref[15 * (int64_t)q + k] = cr[k];
      cam_cur[15 * (int64_t)q + k] = cc[k];
    }
  }
  const double* Ra = a.R + 9 * (int64_t)ra;
  const double fa = a.cams[15 * (int64_t)ra];
  for (int64_t i = lo + lane; i < hi; i += WAVE) {
    bool k = false;
    if (an >= 0 && landmark_vote(a.idx_a, a.lm_home, a.n_lm, a.n_ref, i) >= 0) k = landmark_transfer(Ra, fa, a.lm_ray + 3 * (int64_t)a.idx_a[i]).keep;
    keep[i] = k ? 1 : 0;
  }
}

__global__ __launch_bounds__(WAVE) void k_landmark_transfer(LmAsmIn a, const float2* __restrict__ uv_b, const int32_t* __restrict__ anchor_ref,
                                                            const int64_t* __restrict__ out_ptr, const int32_t* __restrict__ out_index,
                                                            float2* __restrict__ out_uv_ref, float2* __restrict__ out_uv_cur,
                                                            int32_t* __restrict__ out_src)
{
  const int q = blockIdx.x, lane = threadIdx.x;
  const int32_t an = anchor_ref[q];
  if (an < 0) return;
  const double* Ra = a.R + 9 * (int64_t)an;
  const double fa = a.cams[15 * (int64_t)an];
  int64_t hi = out_ptr[q + 1];
  if (hi > a.n_match) hi = a.n_match;
  for (int64_t o = out_ptr[q] + lane; o < hi; o += WAVE) {
    if (o < 0) continue;
    const int32_t src = out_index[o];
    if (src < 0 || src >= a.n_match) continue;  // (cannot happen: the index came from a keep byte)
    const int32_t l = a.idx_a[src];
    if (l < 0 || l >= a.n_lm) continue;
    const RelocPixel px = landmark_transfer(Ra, fa, a.lm_ray + 3 * (int64_t)l);
    out_uv_ref[o] = make_float2(px.u, px.v);
    out_uv_cur[o] = uv_b[src];
    out_src[o] = src;
  }
}

// the workspace of one assembly
struct LmWork {
  size_t ones, cnt, keep, index, total;
  LmWork(int n_query, int64_t n_match)
  {
    const size_t nq = (size_t)(n_query > 0 ? n_query : 1), nm = (size_t)(n_match > 0 ? n_match : 1);
    BlockLayout b;
    ones = b.take(sizeof(int32_t) * nq);
    cnt = b.take(sizeof(int32_t) * nq);
    keep = b.take(nm);
    index = b.take(sizeof(int32_t) * nm);
    total = b.total();
  }
};

bool lm_known_factor(int32_t t) { return t >= PTZ_KRT_F && t <= PTZ_KRT_FxfyDist; }

void enqueue_lm_assemble(const ptz_landmark_map* map, int n_query, int64_t n_match, const int64_t* d_match_ptr, const int32_t* d_idx_a,
                         const float* d_uv_b, const double* d_cams, const double* d_R, const int32_t* d_wh, int32_t* d_anchor,
                         int64_t* d_out_ptr, float* d_out_uv_ref, float* d_out_uv_cur, int32_t* d_out_src, double* d_cam_ref,
                         double* d_cam_cur, char* ws, hipStream_t st)
{
  const LmWork w(n_query, n_match);
  int32_t *ones = (int32_t*)(ws + w.ones), *cnt = (int32_t*)(ws + w.cnt), *index = (int32_t*)(ws + w.index);
  uint8_t* keep = (uint8_t*)(ws + w.keep);
  const LmAsmIn a = {n_query, map->n_ref, map->n_lm, n_match, d_match_ptr, d_idx_a, map->d_ray, map->d_home, d_cams, d_R};
  hipLaunchKernelGGL(k_landmark_anchor, dim3(n_query), dim3(WAVE), sizeof(int32_t) * (size_t)map->n_ref, st, a, d_wh, d_anchor, ones, keep, d_cam_ref,
                     d_cam_cur);
  enqueue_compact(n_query, d_match_ptr, ones, keep, 0, cnt, d_out_ptr, nullptr, nullptr, nullptr, nullptr, index, st);
  if (n_match > 0)
    hipLaunchKernelGGL(k_landmark_transfer, dim3(n_query), dim3(WAVE), 0, st, a, (const float2*)d_uv_b, (const int32_t*)d_anchor,
                       (const int64_t*)d_out_ptr, (const int32_t*)index, (float2*)d_out_uv_ref, (float2*)d_out_uv_cur, d_out_src);
}

}  // namespace
}  // namespace ptz

extern "C" void ptz_landmark_map_destroy(ptz_landmark_map* m)
{
  if (!m) return;
  ptz::DeviceGuard g(m->device);
  ptz_desc_set_destroy(m->set);
  ptz_desc_set_destroy(m->home_set);
  delete m;
}

namespace ptz {
namespace {

// The body of ptz_landmark_map_create.  The three track arrays are the caller's host arrays (kind = hipMemcpyHostToDevice, trk_ptr
// checked here) or a ptz_tracks' device arrays on the set's device (hipMemcpyDeviceToDevice, n_view the tracks' own): the copies
// differ, the launches do not.
int32_t lm_map_create(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, int32_t n_track, int64_t n_view, const int64_t* trk_ptr,
                      const int32_t* trk_img, const int32_t* trk_feat, hipMemcpyKind kind, int32_t factor_type, int32_t min_views,
                      int32_t device_id, ptz_landmark_map** out)
{
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  // validation first, device second
  if (!ref_set || !ref_cams || n_ref < 1 || n_track < 0 || !trk_ptr || min_views < 1 || device_id < 0) return PTZ_EINVAL;
  if (ref_set->n_img != n_ref || ref_set->device != device_id) return PTZ_EINVAL;
  if (kind == hipMemcpyHostToDevice) {
    if (trk_ptr[0] != 0) return PTZ_EINVAL;
    for (int t = 0; t < n_track; ++t)
      if (trk_ptr[t + 1] < trk_ptr[t]) return PTZ_EINVAL;
    n_view = trk_ptr[n_track];
  }
  if (n_view < 0) return PTZ_EINVAL;
  if (n_view > 0 && (!trk_img || !trk_feat)) return PTZ_EINVAL;
  if (ref_set->n_feat > 0 && !ref_set->d_kp) return PTZ_EINVAL;  // a set without key points has no rays
  if (!lm_known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  static_assert(LM_MAX_WORDS == 2 * WAVE, "two packed words a lane");
  if (n_ref > kLandmarkMaxRefs || 16 * ref_set->KS > LM_MAX_WORDS) return PTZ_ELIMIT;  // (ptz_desc_set_create bounds D by 512)
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  std::vector<double> R(9 * (size_t)n_ref);
  if (const int32_t rc = ptz_reloc_ref_rotations(n_ref, ref_cams, R.data())) return rc;

  struct Free { void operator()(ptz_landmark_map* m) const { ptz_landmark_map_destroy(m); } };
  std::unique_ptr<ptz_landmark_map, Free> map(new ptz_landmark_map());
  map->device = device_id; map->n_ref = n_ref; map->n_track = n_track; map->D = ref_set->D; map->factor_type = factor_type;
  map->min_views = min_views;
  const int D = ref_set->D;
  const size_t nt = (size_t)(n_track > 0 ? n_track : 1), nv = (size_t)(n_view > 0 ? n_view : 1);
  const int n_chunk = (n_track + LM_CHUNK - 1) / LM_CHUNK;
  const size_t nc = (size_t)(n_chunk > 0 ? n_chunk : 1);
  BlockLayout b;
  const size_t o_cams = b.take(sizeof(double) * 15 * n_ref), o_R = b.take(sizeof(double) * 9 * n_ref), o_tptr = b.take(sizeof(int64_t) * (nt + 1)),
               o_timg = b.take(sizeof(int32_t) * nv), o_tfeat = b.take(sizeof(int32_t) * nv), o_cptr = b.take(sizeof(int64_t) * (nc + 1)),
               o_ones = b.take(sizeof(int32_t) * nc), o_cnt = b.take(sizeof(int32_t) * nc), o_optr = b.take(sizeof(int64_t) * (nc + 1)),
               o_flag = b.take(nt), o_track = b.take(sizeof(int32_t) * nt), o_ray_t = b.take(sizeof(double) * 3 * nt),
               o_home_t = b.take(sizeof(int32_t) * nt), o_views_t = b.take(sizeof(int32_t) * nt), o_desc_t = b.take(nt * D),
               o_ray = b.take(sizeof(double) * 3 * nt), o_home = b.take(sizeof(int32_t) * nt), o_views = b.take(sizeof(int32_t) * nt),
               o_desc = b.take(nt * D);
  CallHeld h;  // (declared after the map: the stream is waited for before a map that is not returned gives its block back)
  if (const int32_t rc = h.acquire(device_id, b.total())) { (void)hipGetLastError(); return rc; }
  char* d = h.base;
  std::vector<int64_t> cptr(nc + 1, 0);
  for (int c = 0; c <= n_chunk; ++c) cptr[c] = std::min<int64_t>((int64_t)c * LM_CHUNK, n_track);
  const std::vector<int32_t> ones(nc, 1);
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_cams, ref_cams, sizeof(double) * 15 * n_ref, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_R, R.data(), sizeof(double) * 9 * n_ref, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_tptr, trk_ptr, sizeof(int64_t) * ((size_t)n_track + 1), kind, h.st));
  if (n_view > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_timg, trk_img, sizeof(int32_t) * n_view, kind, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_tfeat, trk_feat, sizeof(int32_t) * n_view, kind, h.st));
  }
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_cptr, cptr.data(), sizeof(int64_t) * (nc + 1), hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_ones, ones.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  const LmBuildIn a = {n_ref, n_track, D, 16 * ref_set->KS, factor_type & 1, min_views, ref_set->d_feat_ptr, ref_set->d_row_off,
                       (const uint32_t*)ref_set->d_desc, ref_set->d_kp, (const double*)(d + o_cams), (const double*)(d + o_R),
                       (const int64_t*)(d + o_tptr), (const int32_t*)(d + o_timg), (const int32_t*)(d + o_tfeat)};
  const int per = LM_WG / WAVE;
  if (n_track > 0)
    hipLaunchKernelGGL(k_landmark_build, dim3((n_track + per - 1) / per), dim3(LM_WG), 0, h.st, a, (uint8_t*)(d + o_flag), (double*)(d + o_ray_t),
                       (int32_t*)(d + o_home_t), (int32_t*)(d + o_views_t), (uint8_t*)(d + o_desc_t));
  enqueue_compact(n_chunk, (const int64_t*)(d + o_cptr), (const int32_t*)(d + o_ones), (const uint8_t*)(d + o_flag), 0, (int32_t*)(d + o_cnt),
                  (int64_t*)(d + o_optr), nullptr, nullptr, nullptr, nullptr, (int32_t*)(d + o_track), h.st);
  if (n_track > 0)
    hipLaunchKernelGGL(k_landmark_gather, dim3((n_track + per - 1) / per), dim3(LM_WG), 0, h.st, D, (const int64_t*)(d + o_optr) + n_chunk,
                       (const int32_t*)(d + o_track), (const double*)(d + o_ray_t), (const int32_t*)(d + o_home_t),
                       (const int32_t*)(d + o_views_t), (const uint8_t*)(d + o_desc_t), (double*)(d + o_ray), (int32_t*)(d + o_home),
                       (int32_t*)(d + o_views), (uint8_t*)(d + o_desc));
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  int64_t n_lm = 0;
  PTZ_HIP_TRY(hipMemcpyAsync(&n_lm, (const int64_t*)(d + o_optr) + n_chunk, sizeof(int64_t), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  if (n_lm < 0 || n_lm > n_track) return PTZ_ENODEVICE;  // (a scan that did not run)
  map->n_lm = (int32_t)n_lm;
  map->build_ms = h.elapsed_ms();
  const size_t nl = (size_t)n_lm;
  map->track.resize(nl); map->home.resize(nl); map->views.resize(nl); map->ray.resize(3 * nl); map->desc.resize(nl * D);
  BlockLayout mb;
  const size_t m_ray = mb.take(sizeof(double) * 3 * (nl ? nl : 1)), m_home = mb.take(sizeof(int32_t) * (nl ? nl : 1));
  if (map->blk.get(device_id, mb.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  map->d_ray = (double*)(map->blk.p + m_ray); map->d_home = (int32_t*)(map->blk.p + m_home);
  if (nl > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(map->d_ray, d + o_ray, sizeof(double) * 3 * nl, hipMemcpyDeviceToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->d_home, d + o_home, sizeof(int32_t) * nl, hipMemcpyDeviceToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->track.data(), d + o_track, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->ray.data(), d + o_ray, sizeof(double) * 3 * nl, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->home.data(), d + o_home, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->views.data(), d + o_views, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(map->desc.data(), d + o_desc, nl * D, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(stream_wait(h.st));
  }
  PTZ_HIP_TRY(hipGetLastError());
  // the map's descriptors as ONE image of the matcher's: the packing stays in ptz_desc_set_create
  const int64_t fp[2] = {0, n_lm};
  const std::vector<float> kp(2 * (nl ? nl : 1), 0.f);
  if (const int32_t rc = ptz_desc_set_create(1, fp, nl ? map->desc.data() : nullptr, D, kp.data(), device_id, &map->set)) return rc;
  *out = map.release();
  return PTZ_OK;
}

}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_landmark_map_create(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, int32_t n_track,
                                           const int64_t* trk_ptr, const int32_t* trk_img, const int32_t* trk_feat, int32_t factor_type,
                                           int32_t min_views, int32_t device_id, ptz_landmark_map** out)
{
  return ptz::lm_map_create(ref_set, ref_cams, n_ref, n_track, 0, trk_ptr, trk_img, trk_feat, hipMemcpyHostToDevice, factor_type, min_views, device_id,
                            out);
}

extern "C" int32_t ptz_landmark_map_create_from_tracks(const ptz_desc_set* ref_set, const double* ref_cams, int32_t n_ref, const ptz_tracks* tracks,
                                                       int32_t factor_type, int32_t min_views, ptz_landmark_map** out)
{
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (!tracks || !ref_set || tracks->device != ref_set->device || tracks->n_img != ref_set->n_img || tracks->n_feat != ref_set->n_feat) return PTZ_EINVAL;
  return ptz::lm_map_create(ref_set, ref_cams, n_ref, tracks->n_track, tracks->n_view, tracks->d_trk_ptr, tracks->d_trk_img, tracks->d_trk_feat,
                            hipMemcpyDeviceToDevice, factor_type, min_views, ref_set->device, out);
}

extern "C" int32_t ptz_landmark_map_n_landmarks(const ptz_landmark_map* m) { return m ? m->n_lm : 0; }

extern "C" double ptz_landmark_map_build_ms(const ptz_landmark_map* m) { return m ? m->build_ms : 0.0; }

extern "C" const ptz_desc_set* ptz_landmark_map_desc_set(const ptz_landmark_map* m) { return m ? m->set : nullptr; }

extern "C" int32_t ptz_landmark_map_download(const ptz_landmark_map* m, int32_t* lm_track, double* lm_ray, int32_t* lm_home, int32_t* lm_views,
                                             uint8_t* lm_desc)
{
  if (!m) return PTZ_EINVAL;
  const size_t n = (size_t)m->n_lm;
  if (n == 0) return PTZ_OK;
  if (lm_track) memcpy(lm_track, m->track.data(), sizeof(int32_t) * n);
  if (lm_ray) memcpy(lm_ray, m->ray.data(), sizeof(double) * 3 * n);
  if (lm_home) memcpy(lm_home, m->home.data(), sizeof(int32_t) * n);
  if (lm_views) memcpy(lm_views, m->views.data(), sizeof(int32_t) * n);
  if (lm_desc) memcpy(lm_desc, m->desc.data(), n * (size_t)m->D);
  return PTZ_OK;
}

extern "C" int64_t ptz_landmark_assemble_workspace_bytes(int32_t n_query, int64_t n_match)
{
  if (n_query < 0 || n_match < 0) return 0;
  return (int64_t)ptz::LmWork(n_query, n_match).total;
}

extern "C" int32_t ptz_landmark_assemble_device(const ptz_landmark_map* map, int32_t n_query, int64_t n_match, const int64_t* d_match_ptr,
                                                const int32_t* d_idx_a, const float* d_uv_b, const double* d_ref_cams, const double* d_ref_R,
                                                const int32_t* d_query_wh, int32_t factor_type, int32_t* d_anchor_ref, int64_t* d_out_ptr,
                                                float* d_out_uv_ref, float* d_out_uv_cur, int32_t* d_out_src, double* d_cam_ref,
                                                double* d_cam_cur, void* d_workspace, int64_t workspace_bytes, void* hip_stream)
{
  using namespace ptz;
  if (!map || n_query < 0 || n_match < 0) return PTZ_EINVAL;
  if (!lm_known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!d_match_ptr || !d_ref_cams || !d_ref_R || !d_query_wh || !d_anchor_ref || !d_out_ptr || !d_cam_ref || !d_cam_cur || !d_workspace)
    return PTZ_EINVAL;
  if (n_match > 0 && (!d_idx_a || !d_uv_b || !d_out_uv_ref || !d_out_uv_cur || !d_out_src)) return PTZ_EINVAL;
  if (n_match > INT32_MAX) return PTZ_ELIMIT;  // out_src and the compaction's positions are int32
  if (map->n_ref > kLandmarkMaxRefs) return PTZ_ELIMIT;
  if (((uintptr_t)d_workspace & 255) != 0 || workspace_bytes < ptz_landmark_assemble_workspace_bytes(n_query, n_match)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_cam_cur, hip_stream, &device)) return rc;
  if (device != map->device) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(device);
  enqueue_lm_assemble(map, n_query, n_match, d_match_ptr, d_idx_a, d_uv_b, d_ref_cams, d_ref_R, d_query_wh, d_anchor_ref, d_out_ptr, d_out_uv_ref,
                      d_out_uv_cur, d_out_src, d_cam_ref, d_cam_cur, (char*)d_workspace, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_landmark_assemble(const ptz_landmark_map* map, int32_t n_query, const int64_t* match_ptr, const int32_t* idx_a,
                                         const float* uv_b, const double* ref_cams, const double* ref_R, const int32_t* query_wh,
                                         int32_t factor_type, int32_t* anchor_ref, int64_t* out_ptr, float* out_uv_ref, float* out_uv_cur,
                                         int32_t* out_src, double* cam_ref, double* cam_cur, double* device_ms)
{
  using namespace ptz;
  // validation first, device second
  if (!map || n_query < 0 || !match_ptr || match_ptr[0] != 0) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (match_ptr[q + 1] < match_ptr[q]) return PTZ_EINVAL;
  const int64_t n_match = match_ptr[n_query];
  if (n_match > 0 && (!idx_a || !uv_b || !out_uv_ref || !out_uv_cur || !out_src)) return PTZ_EINVAL;
  if (n_match > INT32_MAX) return PTZ_ELIMIT;
  for (int64_t i = 0; i < n_match; ++i)
    if (idx_a[i] < 0 || idx_a[i] >= map->n_lm) return PTZ_EINVAL;
  if (n_query > 0 && (!ref_cams || !ref_R || !query_wh || !anchor_ref || !out_ptr || !cam_ref || !cam_cur)) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_wh[2 * q] <= 0 || query_wh[2 * q + 1] <= 0) return PTZ_EINVAL;
  if (!lm_known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (device_ms) *device_ms = 0;
  if (n_query == 0) return PTZ_OK;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= map->device) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(map->device);

  const size_t nq = (size_t)n_query, nm = (size_t)(n_match > 0 ? n_match : 1), nr = (size_t)map->n_ref;
  BlockLayout b;
  const size_t o_mptr = b.take(sizeof(int64_t) * (nq + 1)), o_ia = b.take(sizeof(int32_t) * nm), o_uvb = b.take(sizeof(float) * 2 * nm),
               o_cams = b.take(sizeof(double) * 15 * nr), o_R = b.take(sizeof(double) * 9 * nr), o_wh = b.take(sizeof(int32_t) * 2 * nq),
               o_an = b.take(sizeof(int32_t) * nq), o_optr = b.take(sizeof(int64_t) * (nq + 1)), o_our = b.take(sizeof(float) * 2 * nm),
               o_ouc = b.take(sizeof(float) * 2 * nm), o_osrc = b.take(sizeof(int32_t) * nm), o_cref = b.take(sizeof(double) * 15 * nq),
               o_ccur = b.take(sizeof(double) * 15 * nq), o_ws = b.take(LmWork(n_query, n_match).total);
  CallHeld h;
  if (const int32_t rc = h.acquire(map->device, b.total())) return rc;
  char* d = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_mptr, match_ptr, sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice, h.st));
  if (n_match > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_ia, idx_a, sizeof(int32_t) * n_match, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_uvb, uv_b, sizeof(float) * 2 * n_match, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_cams, ref_cams, sizeof(double) * 15 * nr, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_R, ref_R, sizeof(double) * 9 * nr, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_lm_assemble(map, n_query, n_match, (const int64_t*)(d + o_mptr), (const int32_t*)(d + o_ia), (const float*)(d + o_uvb),
                      (const double*)(d + o_cams), (const double*)(d + o_R), (const int32_t*)(d + o_wh), (int32_t*)(d + o_an), (int64_t*)(d + o_optr),
                      (float*)(d + o_our), (float*)(d + o_ouc), (int32_t*)(d + o_osrc), (double*)(d + o_cref), (double*)(d + o_ccur), d + o_ws, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(anchor_ref, d + o_an, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(out_ptr, d + o_optr, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(cam_ref, d + o_cref, sizeof(double) * 15 * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(cam_cur, d + o_ccur, sizeof(double) * 15 * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  const int64_t kept = out_ptr[n_query];
  if (kept < 0 || kept > n_match) return PTZ_ENODEVICE;  // (a scan that did not run)
  if (kept > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_ref, d + o_our, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_cur, d + o_ouc, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(out_src, d + o_osrc, sizeof(int32_t) * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(stream_wait(h.st));
  }
  PTZ_HIP_TRY(hipGetLastError());
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}
