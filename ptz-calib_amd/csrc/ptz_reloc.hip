// ptz_reloc.hip -- the relocalization assembly on the device (gfx950): from the match table of every (reference, query) pair to the
// CSR and the cameras the single-view solve takes, for the K best references of every query.  The contract is ptz_reloc_assemble.h
// (first include: its fp contract(off) must precede ptz_factor.h); this file adds the launch shapes and the C-ABI, nothing the result
// depends on.
//
//   k_reloc_select   one wave per query over its pair list, K rounds of a wave arg-max on the unique key (count, -position)
//   k_reloc_count    one thread per candidate match of the selected pairs: the keep byte of the header's rule
//   (kept counts per query, their scan and the kept candidates' positions: enqueue_compact of ptz_gate_compact.h)
//   k_reloc_gather   one thread per kept match: transfers it once more and writes it where the scan put it
//   k_reloc_cams     one thread per query: cam_ref, cam_cur
//
// The candidates of query q live at [qm[q], qm[q] + cand[q]) of a match-sized index space, qm[q] = match_ptr[query_ptr[q]]: a query's
// selected pairs are pairs of its own list, so its candidates never outnumber its own matches and the offsets need no scan of their
// own.  No atomics anywhere; a query's output depends on its own pairs only.
#include "ptz_reloc_assemble.h"

#include "ptz_common.h"
#include "ptz_gate_compact.h"
#include "ptz_host_batch.h"

namespace ptz {
namespace {

constexpr int RELOC_WG = 256;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(RELOC_WG) void k_reloc_select(int n_query, int n_pair, int n_ref, int K, const int64_t* __restrict__ match_ptr,
                                                           const int32_t* __restrict__ pair_ref, const int64_t* __restrict__ query_ptr,
                                                           int32_t* __restrict__ sel_pair, int32_t* __restrict__ n_sel,
                                                           int64_t* __restrict__ qm, int32_t* __restrict__ cand, int32_t* __restrict__ ones)
{
  const int q = blockIdx.x * (RELOC_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (q >= n_query) return;
  int64_t lo = query_ptr[q], hi = query_ptr[q + 1];
  if (lo < 0 || hi > n_pair || hi < lo) { lo = 0; hi = 0; }  // (the device form does not validate: a malformed list is an empty one)
  const int64_t len = hi - lo;
  unsigned long long prev = ~0ull;
  int ns = 0;
  int64_t total = 0;
  for (int s = 0; s < K; ++s) {
    unsigned long long best = 0;
    for (int64_t j = lane; j < len; j += WAVE) {
      const unsigned long long key = reloc_key(reloc_pair_count(match_ptr, pair_ref, n_ref, lo + j), (int32_t)j);
      if (key < prev && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (best == 0) break;  // (one value in the wave)
    if (lane == 0) sel_pair[(int64_t)K * q + s] = (int32_t)(lo + reloc_key_pos(best));
    total += reloc_key_count(best);
    prev = best;
    ++ns;
  }
  for (int s = ns + lane; s < K; s += WAVE) sel_pair[(int64_t)K * q + s] = -1;
  if (lane == 0) {
    n_sel[q] = ns;
    cand[q] = (int32_t)total;
    ones[q] = 1;
    qm[q] = match_ptr[lo];
    if (q == n_query - 1) qm[n_query] = match_ptr[hi];
  }
}

// the query whose candidate range holds index i: the last q with qm[q] <= i (empty queries repeat an offset)
__device__ __forceinline__ int reloc_query_of(const int64_t* __restrict__ qm, int n_query, int64_t i)
{
  int a = 0, b = n_query;  // qm[a] <= i < qm[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (qm[m] <= i) a = m; else b = m;
  }
  return a;
}

struct RelocIn {
  int n_query, n_ref, K, dist;
  int64_t n_match;
  const int64_t* match_ptr;
  const float2* uv_ref;
  const int32_t* pair_ref;
  const double *ref_cams, *ref_R;
  const int32_t *sel_pair, *n_sel;
  const int64_t* qm;
  const int32_t* cand;
};

// candidate index i -> its input index (src) and, for K > 1, its transferred pixel; false: i is no candidate
__device__ __forceinline__ bool reloc_candidate(const RelocIn& a, int64_t i, int64_t* src, RelocPixel* px)
{
  if (i < a.qm[0] || i >= a.qm[a.n_query]) return false;
  const int q = reloc_query_of(a.qm, a.n_query, i);
  const int64_t j = i - a.qm[q];
  if (j >= a.cand[q]) return false;
  const int32_t* sel = a.sel_pair + (int64_t)a.K * q;
  int32_t p;
  reloc_locate(a.match_ptr, sel, a.n_sel[q], j, &p, src);
  if (*src < 0 || *src >= a.n_match) return false;
  const float2 uv = a.uv_ref[*src];
  if (a.K == 1) {
    *px = {uv.x, uv.y, true};
    return true;
  }
  const int32_t r = a.pair_ref[p], an = a.pair_ref[sel[0]];
  *px = reloc_transfer(a.ref_cams + 15 * (int64_t)r, a.ref_R + 9 * (int64_t)r, a.ref_R + 9 * (int64_t)an, a.ref_cams[15 * (int64_t)an], a.dist, uv.x,
                       uv.y);
  return true;
}

__global__ __launch_bounds__(RELOC_WG) void k_reloc_count(RelocIn a, uint8_t* __restrict__ keep)
{
  const int64_t i = (int64_t)blockIdx.x * RELOC_WG + threadIdx.x;
  if (i >= a.n_match) return;
  int64_t src;
  RelocPixel px;
  keep[i] = (reloc_candidate(a, i, &src, &px) && px.keep) ? 1 : 0;
}

__global__ __launch_bounds__(RELOC_WG) void k_reloc_gather(RelocIn a, const float2* __restrict__ uv_cur, const int64_t* __restrict__ out_ptr,
                                                           const int32_t* __restrict__ out_index, float2* __restrict__ out_uv_ref,
                                                           float2* __restrict__ out_uv_cur, int32_t* __restrict__ out_src)
{
  const int64_t o = (int64_t)blockIdx.x * RELOC_WG + threadIdx.x;
  if (o >= a.n_match || o >= out_ptr[a.n_query]) return;
  int64_t src;
  RelocPixel px;
  if (!reloc_candidate(a, out_index[o], &src, &px)) return;  // (cannot happen: the index came from a keep byte)
  out_uv_ref[o] = make_float2(px.u, px.v);
  out_uv_cur[o] = uv_cur[src];
  out_src[o] = (int32_t)src;
}

__global__ void k_reloc_cams(int n_query, int n_pair, int n_ref, int K, const int32_t* __restrict__ pair_ref, const int64_t* __restrict__ query_ptr,
                             const double* __restrict__ ref_cams, const int32_t* __restrict__ query_wh, const int32_t* __restrict__ sel_pair,
                             const int32_t* __restrict__ n_sel, double* __restrict__ cam_ref, double* __restrict__ cam_cur)
{
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_query) return;
  int32_t r = 0;
  if (n_sel[q] > 0) r = pair_ref[sel_pair[(int64_t)K * q]];
  else {
    const int64_t lo = query_ptr[q], hi = query_ptr[q + 1];
    if (lo >= 0 && lo < hi && hi <= n_pair) r = pair_ref[lo];
    if (r < 0 || r >= n_ref) r = 0;
  }
  double cr[15], cc[15];
  reloc_cameras(ref_cams + 15 * (int64_t)r, query_wh[2 * q], query_wh[2 * q + 1], K, cr, cc);
  for (int k = 0; k < 15; ++k) {
    cam_ref[15 * (int64_t)q + k] = cr[k];
    cam_cur[15 * (int64_t)q + k] = cc[k];
  }
}

// the workspace of one call
struct RelocWork {
  size_t qm, cand, ones, cnt, keep, index, total;
  RelocWork(int n_query, int64_t n_match)
  {
    const size_t nq = (size_t)(n_query > 0 ? n_query : 1), nm = (size_t)(n_match > 0 ? n_match : 1);
    BlockLayout b;
    qm = b.take(sizeof(int64_t) * (nq + 1));
    cand = b.take(sizeof(int32_t) * nq);
    ones = b.take(sizeof(int32_t) * nq);
    cnt = b.take(sizeof(int32_t) * nq);
    keep = b.take(nm);
    index = b.take(sizeof(int32_t) * nm);
    total = b.total();
  }
};

bool known_factor(int32_t t) { return t >= PTZ_KRT_F && t <= PTZ_KRT_FxfyDist; }

void enqueue_assemble(int n_query, int n_pair, int64_t n_match, int n_ref, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                      const int32_t* d_pair_ref, const int64_t* d_query_ptr, const double* d_ref_cams, const double* d_ref_R,
                      const int32_t* d_query_wh, int factor_type, int K, int32_t* d_sel_pair, int32_t* d_n_sel, int64_t* d_out_ptr,
                      float* d_out_uv_ref, float* d_out_uv_cur, int32_t* d_out_src, double* d_cam_ref, double* d_cam_cur, char* ws, hipStream_t st)
{
  const RelocWork w(n_query, n_match);
  int64_t* qm = (int64_t*)(ws + w.qm);
  int32_t *cand = (int32_t*)(ws + w.cand), *ones = (int32_t*)(ws + w.ones), *cnt = (int32_t*)(ws + w.cnt), *index = (int32_t*)(ws + w.index);
  uint8_t* keep = (uint8_t*)(ws + w.keep);
  const int per = RELOC_WG / WAVE;
  hipLaunchKernelGGL(k_reloc_select, dim3((n_query + per - 1) / per), dim3(RELOC_WG), 0, st, n_query, n_pair, n_ref, K, d_match_ptr, d_pair_ref,
                     d_query_ptr, d_sel_pair, d_n_sel, qm, cand, ones);
  hipLaunchKernelGGL(k_reloc_cams, dim3((n_query + RELOC_WG - 1) / RELOC_WG), dim3(RELOC_WG), 0, st, n_query, n_pair, n_ref, K, d_pair_ref, d_query_ptr,
                     d_ref_cams, d_query_wh, (const int32_t*)d_sel_pair, (const int32_t*)d_n_sel, d_cam_ref, d_cam_cur);
  const RelocIn a = {n_query, n_ref, K, factor_type & 1, n_match, d_match_ptr, (const float2*)d_uv_ref, d_pair_ref, d_ref_cams, d_ref_R,
                     d_sel_pair, d_n_sel, qm, cand};
  const unsigned blocks = (unsigned)((n_match + RELOC_WG - 1) / RELOC_WG);
  if (n_match > 0) hipLaunchKernelGGL(k_reloc_count, dim3(blocks), dim3(RELOC_WG), 0, st, a, keep);
  enqueue_compact(n_query, qm, ones, keep, 0, cnt, d_out_ptr, nullptr, nullptr, nullptr, nullptr, index, st);
  if (n_match > 0)
    hipLaunchKernelGGL(k_reloc_gather, dim3(blocks), dim3(RELOC_WG), 0, st, a, (const float2*)d_uv_cur, (const int64_t*)d_out_ptr, (const int32_t*)index,
                       (float2*)d_out_uv_ref, (float2*)d_out_uv_cur, d_out_src);
}

}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_reloc_ref_rotations(int32_t n_ref, const double* ref_cams, double* ref_R)
{
  if (n_ref < 0 || (n_ref > 0 && (!ref_cams || !ref_R))) return PTZ_EINVAL;
  for (int r = 0; r < n_ref; ++r) ptz::rodrigues(ref_cams + 15 * (size_t)r + 4, ref_R + 9 * (size_t)r);
  return PTZ_OK;
}

extern "C" int64_t ptz_reloc_assemble_workspace_bytes(int32_t n_query, int64_t n_match)
{
  if (n_query < 0 || n_match < 0) return 0;
  return (int64_t)ptz::RelocWork(n_query, n_match).total;
}

extern "C" int32_t ptz_reloc_assemble_device(int32_t n_query, int32_t n_pair, int64_t n_match, int32_t n_ref, const int64_t* d_match_ptr,
                                             const float* d_uv_ref, const float* d_uv_cur, const int32_t* d_pair_ref,
                                             const int64_t* d_query_ptr, const double* d_ref_cams, const double* d_ref_R,
                                             const int32_t* d_query_wh, int32_t factor_type, int32_t max_refs, int32_t* d_sel_pair,
                                             int32_t* d_n_sel, int64_t* d_out_ptr, float* d_out_uv_ref, float* d_out_uv_cur,
                                             int32_t* d_out_src, double* d_cam_ref, double* d_cam_cur, void* d_workspace,
                                             int64_t workspace_bytes, void* hip_stream)
{
  using namespace ptz;
  if (n_query < 0 || n_pair < 0 || n_match < 0 || n_ref < 0 || max_refs < 1) return PTZ_EINVAL;
  if (!known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (n_ref < 1 || !d_match_ptr || !d_query_ptr || !d_ref_cams || !d_ref_R || !d_query_wh || !d_sel_pair || !d_n_sel || !d_out_ptr ||
      !d_cam_ref || !d_cam_cur || !d_workspace)
    return PTZ_EINVAL;
  if (n_pair > 0 && !d_pair_ref) return PTZ_EINVAL;
  if (n_match > 0 && (!d_uv_ref || !d_uv_cur || !d_out_uv_ref || !d_out_uv_cur || !d_out_src)) return PTZ_EINVAL;
  if (n_match > INT32_MAX) return PTZ_ELIMIT;  // out_src and the compaction's positions are int32
  if (((uintptr_t)d_workspace & 255) != 0 || workspace_bytes < ptz_reloc_assemble_workspace_bytes(n_query, n_match)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_cam_cur, hip_stream, &device)) return rc;
  PTZ_DEVICE_GUARD(device);
  enqueue_assemble(n_query, n_pair, n_match, n_ref, d_match_ptr, d_uv_ref, d_uv_cur, d_pair_ref, d_query_ptr, d_ref_cams, d_ref_R, d_query_wh,
                   factor_type, max_refs, d_sel_pair, d_n_sel, d_out_ptr, d_out_uv_ref, d_out_uv_cur, d_out_src, d_cam_ref, d_cam_cur,
                   (char*)d_workspace, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_reloc_assemble(int32_t n_query, int32_t n_pair, int32_t n_ref, const int64_t* match_ptr, const float* uv_ref,
                                      const float* uv_cur, const int32_t* pair_ref, const int64_t* query_ptr, const double* ref_cams,
                                      const double* ref_R, const int32_t* query_wh, int32_t factor_type, int32_t max_refs,
                                      int32_t device_id, int32_t* sel_pair, int32_t* n_sel, int64_t* out_ptr, float* out_uv_ref,
                                      float* out_uv_cur, int32_t* out_src, double* cam_ref, double* cam_cur, double* device_ms)
{
  using namespace ptz;
  // validation first, device second
  if (n_query < 0 || n_pair < 0 || n_ref < 0 || max_refs < 1 || device_id < 0) return PTZ_EINVAL;
  if (!match_ptr || !query_ptr) return PTZ_EINVAL;
  if (match_ptr[0] != 0 || query_ptr[0] != 0 || query_ptr[n_query] != n_pair) return PTZ_EINVAL;
  for (int p = 0; p < n_pair; ++p)
    if (match_ptr[p + 1] < match_ptr[p]) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_ptr[q + 1] < query_ptr[q]) return PTZ_EINVAL;
  const int64_t n_match = match_ptr[n_pair];
  if (n_pair > 0 && !pair_ref) return PTZ_EINVAL;
  for (int p = 0; p < n_pair; ++p)
    if (pair_ref[p] < 0 || pair_ref[p] >= n_ref) return PTZ_EINVAL;
  if (n_match > 0 && (!uv_ref || !uv_cur || !out_uv_ref || !out_uv_cur || !out_src)) return PTZ_EINVAL;
  if (n_query > 0 && (n_ref < 1 || !ref_cams || !ref_R || !query_wh || !sel_pair || !n_sel || !out_ptr || !cam_ref || !cam_cur)) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_wh[2 * q] <= 0 || query_wh[2 * q + 1] <= 0) return PTZ_EINVAL;
  if (!known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (device_ms) *device_ms = 0;
  if (n_query == 0) return PTZ_OK;
  if (n_match > INT32_MAX) return PTZ_ELIMIT;
  if ((int64_t)max_refs * n_query > INT32_MAX) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);

  const size_t nq = (size_t)n_query, np = (size_t)(n_pair > 0 ? n_pair : 1), nm = (size_t)(n_match > 0 ? n_match : 1), K = (size_t)max_refs;
  BlockLayout b;
  const size_t o_mptr = b.take(sizeof(int64_t) * (np + 1)), o_uvr = b.take(sizeof(float) * 2 * nm), o_uvc = b.take(sizeof(float) * 2 * nm),
               o_pref = b.take(sizeof(int32_t) * np), o_qptr = b.take(sizeof(int64_t) * (nq + 1)), o_cams = b.take(sizeof(double) * 15 * n_ref),
               o_R = b.take(sizeof(double) * 9 * n_ref), o_wh = b.take(sizeof(int32_t) * 2 * nq), o_sel = b.take(sizeof(int32_t) * K * nq),
               o_nsel = b.take(sizeof(int32_t) * nq), o_optr = b.take(sizeof(int64_t) * (nq + 1)), o_our = b.take(sizeof(float) * 2 * nm),
               o_ouc = b.take(sizeof(float) * 2 * nm), o_osrc = b.take(sizeof(int32_t) * nm), o_cref = b.take(sizeof(double) * 15 * nq),
               o_ccur = b.take(sizeof(double) * 15 * nq), o_ws = b.take(RelocWork(n_query, n_match).total);
  CallHeld h;
  if (const int32_t rc = h.acquire(device_id, b.total())) return rc;
  char* d = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_mptr, match_ptr, sizeof(int64_t) * ((size_t)n_pair + 1), hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_qptr, query_ptr, sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice, h.st));
  if (n_pair > 0) PTZ_HIP_TRY(hipMemcpyAsync(d + o_pref, pair_ref, sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
  if (n_match > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_uvr, uv_ref, sizeof(float) * 2 * n_match, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_uvc, uv_cur, sizeof(float) * 2 * n_match, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_cams, ref_cams, sizeof(double) * 15 * n_ref, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_R, ref_R, sizeof(double) * 9 * n_ref, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_assemble(n_query, n_pair, n_match, n_ref, (const int64_t*)(d + o_mptr), (const float*)(d + o_uvr), (const float*)(d + o_uvc),
                   (const int32_t*)(d + o_pref), (const int64_t*)(d + o_qptr), (const double*)(d + o_cams), (const double*)(d + o_R),
                   (const int32_t*)(d + o_wh), factor_type, max_refs, (int32_t*)(d + o_sel), (int32_t*)(d + o_nsel), (int64_t*)(d + o_optr),
                   (float*)(d + o_our), (float*)(d + o_ouc), (int32_t*)(d + o_osrc), (double*)(d + o_cref), (double*)(d + o_ccur), d + o_ws, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(sel_pair, d + o_sel, sizeof(int32_t) * K * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(n_sel, d + o_nsel, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
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
