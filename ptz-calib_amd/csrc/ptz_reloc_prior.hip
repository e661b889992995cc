// ptz_reloc_prior.hip -- relocalization from a prior camera on the device (gfx950): the overlap shortlist of every query and the
// homography of every listed pair, from cameras alone.  The contract is ptz_reloc_prior.h (first include: its fp contract(off) must
// precede ptz_factor.h's other users); this file adds the launch shapes and the C-ABI, nothing the result depends on.
//
//   k_reloc_prior         one wave per query.  Lanes stride over the references; each builds H(r -> q), its reverse and the overlap
//                         score and stores the score.  After the barrier the wave ranks by counting (sl_wave_list of
//                         ptz_desc_shortlist.h, k_desc_shortlist's own ranking) and writes the list in ascending index; the lane
//                         that owns a listed reference builds its H once more (the same operations, the same bits) into the slot.
//   k_reloc_prior_gather  one thread per pair of the host-built list: bisects query_ptr, copies the slot's nine doubles
//   k_reloc_prior_cams    one thread per query, after the assembly: reloc_prior_camera on its cam_cur
// No atomics, no LDS; a query's output depends on its own prior, its image size, the references and the options only.
#include "ptz_reloc_prior.h"

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"

namespace ptz {
namespace {

constexpr int PRIOR_WG = 256;  // four waves, four queries

__global__ __launch_bounds__(PRIOR_WG) void k_reloc_prior(int n_query, int n_ref, int R, int min_overlap, int factor_type,
                                                          const double* __restrict__ ref_cams, const double* __restrict__ ref_R,
                                                          const double* __restrict__ prior_cams, const double* __restrict__ prior_R,
                                                          const int32_t* __restrict__ query_wh, int32_t* __restrict__ overlap,
                                                          int32_t* __restrict__ shortlist, int32_t* __restrict__ n_short,
                                                          double* __restrict__ H_slot)
{
  const int lane = threadIdx.x % WAVE, q = blockIdx.x * (PRIOR_WG / WAVE) + threadIdx.x / WAVE;
  const bool has = q < n_query;  // (every wave reaches the barrier)
  const int64_t qq = has ? q : 0;
  int32_t* v = overlap + qq * n_ref;
  double Kq[4], Rq[9];
  const int32_t w = query_wh[2 * qq], h = query_wh[2 * qq + 1];
  prior_query_K(prior_cams + 15 * qq, w, h, factor_type, Kq);
  for (int k = 0; k < 9; ++k) Rq[k] = prior_R[9 * qq + k];
  if (has) {
    for (int r = lane; r < n_ref; r += WAVE) {
      double H[9];
      v[r] = prior_overlap(ref_cams + 15 * (int64_t)r, ref_R + 9 * (int64_t)r, Kq, Rq, w, h, H);
    }
  }
  __syncthreads();  // the wave ranks on what its other lanes wrote
  if (!has) return;
  double* Hq = H_slot + 9 * (int64_t)R * q;
  const int taken = sl_wave_list(v, n_ref, R, min_overlap, lane, shortlist + (int64_t)R * q, [&](int s, int r) {
    double H[9];
    prior_homography(ref_cams + 15 * (int64_t)r, ref_R + 9 * (int64_t)r, Kq, Rq, H);
    for (int k = 0; k < 9; ++k) Hq[9 * s + k] = H[k];
  });
  for (int i = 9 * taken + lane; i < 9 * R; i += WAVE) Hq[i] = 0.0;
  if (lane == 0) n_short[q] = taken;
}

__global__ __launch_bounds__(PRIOR_WG) void k_reloc_prior_gather(int n_pair, int n_query, int R, const int64_t* __restrict__ query_ptr,
                                                                 const double* __restrict__ H_slot, double* __restrict__ H)
{
  const int p = blockIdx.x * PRIOR_WG + threadIdx.x;
  if (p >= n_pair) return;
  int a = 0, b = n_query;  // the last q with query_ptr[q] <= p (empty queries repeat an offset)
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (query_ptr[m] <= p) a = m; else b = m;
  }
  const int64_t s = p - query_ptr[a];
  const bool ok = s >= 0 && s < R;  // (a list the host built from n_short <= R; anything else gets no admissible candidate)
  for (int k = 0; k < 9; ++k) H[9 * (int64_t)p + k] = ok ? H_slot[9 * ((int64_t)R * a + s) + k] : 0.0;
}

__global__ __launch_bounds__(PRIOR_WG) void k_reloc_prior_cams(int n_query, int factor_type, const double* __restrict__ prior_cams,
                                                               double* __restrict__ cam_cur)
{
  const int q = blockIdx.x * PRIOR_WG + threadIdx.x;
  if (q < n_query) reloc_prior_camera(cam_cur + 15 * (int64_t)q, prior_cams + 15 * (int64_t)q, factor_type);
}

bool known_factor(int32_t t) { return t >= PTZ_KRT_F && t <= PTZ_KRT_FxfyDist; }

void enqueue_prior(int n_ref, const double* d_ref_cams, const double* d_ref_R, int n_query, const double* d_prior_cams, const double* d_prior_R,
                   const int32_t* d_query_wh, int factor_type, const ptz_prior_options& o, int32_t* d_shortlist, int32_t* d_n_short,
                   int32_t* d_overlap, double* d_H_slot, hipStream_t st)
{
  const int per = PRIOR_WG / WAVE;
  hipLaunchKernelGGL(k_reloc_prior, dim3((n_query + per - 1) / per), dim3(PRIOR_WG), 0, st, n_query, n_ref, o.max_refs, o.min_overlap, factor_type,
                     d_ref_cams, d_ref_R, d_prior_cams, d_prior_R, d_query_wh, d_overlap, d_shortlist, d_n_short, d_H_slot);
}

// the checks both forms share; *o is the options with the defaults filled in
int32_t prior_check(int32_t n_ref, int32_t n_query, int32_t factor_type, const ptz_prior_options* opt, ptz_prior_options* o)
{
  ptz_prior_options_default(o);
  if (opt) *o = *opt;
  if (n_ref < 0 || n_query < 0) return PTZ_EINVAL;
  if (const int32_t rc = prior_options_check(*o)) return rc;
  if (!known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (n_query > 0 && n_ref < 1) return PTZ_EINVAL;
  if ((int64_t)o->max_refs * n_query > INT32_MAX / 9 || (int64_t)n_query * n_ref > INT32_MAX) return PTZ_ELIMIT;
  return PTZ_OK;
}

}  // namespace

void reloc_prior_enqueue_gather(int n_pair, int n_query, int R, const int64_t* d_query_ptr, const double* d_H_slot, double* d_H, hipStream_t st)
{
  if (n_pair > 0)
    hipLaunchKernelGGL(k_reloc_prior_gather, dim3((n_pair + PRIOR_WG - 1) / PRIOR_WG), dim3(PRIOR_WG), 0, st, n_pair, n_query, R, d_query_ptr, d_H_slot, d_H);
}

void reloc_prior_enqueue_cams(int n_query, const double* d_prior_cams, int factor_type, double* d_cam_cur, hipStream_t st)
{
  if (n_query > 0)
    hipLaunchKernelGGL(k_reloc_prior_cams, dim3((n_query + PRIOR_WG - 1) / PRIOR_WG), dim3(PRIOR_WG), 0, st, n_query, factor_type, d_prior_cams, d_cam_cur);
}

}  // namespace ptz

extern "C" void ptz_prior_options_default(ptz_prior_options* o)
{
  if (!o) return;
  o->radius_px = 40.0;
  o->max_refs = 8;
  o->min_overlap = 8;
  o->reserved_ = 0;
}

extern "C" int32_t ptz_reloc_prior_pairs_device(int32_t n_ref, const double* d_ref_cams, const double* d_ref_R, int32_t n_query,
                                                const double* d_prior_cams, const double* d_prior_R, const int32_t* d_query_wh,
                                                int32_t factor_type, const ptz_prior_options* opt, int32_t* d_shortlist, int32_t* d_n_short,
                                                int32_t* d_overlap, double* d_H_slot, void* hip_stream)
{
  using namespace ptz;
  ptz_prior_options o;
  if (const int32_t rc = prior_check(n_ref, n_query, factor_type, opt, &o)) return rc;
  if (n_query == 0) return PTZ_OK;
  if (!d_ref_cams || !d_ref_R || !d_prior_cams || !d_prior_R || !d_query_wh || !d_shortlist || !d_n_short || !d_overlap || !d_H_slot) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_shortlist, hip_stream, &device)) return rc;
  PTZ_DEVICE_GUARD(device);
  enqueue_prior(n_ref, d_ref_cams, d_ref_R, n_query, d_prior_cams, d_prior_R, d_query_wh, factor_type, o, d_shortlist, d_n_short, d_overlap, d_H_slot,
                (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_reloc_prior_pairs(int32_t n_ref, const double* ref_cams, const double* ref_R, int32_t n_query, const double* prior_cams,
                                         const double* prior_R, const int32_t* query_wh, int32_t factor_type, const ptz_prior_options* opt,
                                         int32_t device_id, int32_t* shortlist, int32_t* n_short, int32_t* overlap, double* H_slot,
                                         double* device_ms)
{
  using namespace ptz;
  // validation first, device second
  ptz_prior_options o;
  if (device_id < 0) return PTZ_EINVAL;
  if (const int32_t rc = prior_check(n_ref, n_query, factor_type, opt, &o)) return rc;
  if (n_query > 0 && (!ref_cams || !ref_R || !prior_cams || !prior_R || !query_wh || !shortlist || !n_short)) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_wh[2 * q] <= 0 || query_wh[2 * q + 1] <= 0) return PTZ_EINVAL;
  if (const int32_t rc = prior_cams_check(n_query, prior_cams)) return rc;
  if (device_ms) *device_ms = 0;
  if (n_query == 0) return PTZ_OK;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);

  const size_t nq = (size_t)n_query, nr = (size_t)n_ref, R = (size_t)o.max_refs;
  BlockLayout b;
  const size_t o_cams = b.take(sizeof(double) * 15 * nr), o_R = b.take(sizeof(double) * 9 * nr), o_pc = b.take(sizeof(double) * 15 * nq),
               o_pR = b.take(sizeof(double) * 9 * nq), o_wh = b.take(sizeof(int32_t) * 2 * nq), o_sl = b.take(sizeof(int32_t) * R * nq),
               o_ns = b.take(sizeof(int32_t) * nq), o_ov = b.take(sizeof(int32_t) * nq * nr), o_H = b.take(sizeof(double) * 9 * R * nq);
  CallHeld h;
  if (const int32_t rc = h.acquire(device_id, b.total())) return rc;
  char* d = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_cams, ref_cams, sizeof(double) * 15 * nr, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_R, ref_R, sizeof(double) * 9 * nr, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_pc, prior_cams, sizeof(double) * 15 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_pR, prior_R, sizeof(double) * 9 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_prior(n_ref, (const double*)(d + o_cams), (const double*)(d + o_R), n_query, (const double*)(d + o_pc), (const double*)(d + o_pR),
                (const int32_t*)(d + o_wh), factor_type, o, (int32_t*)(d + o_sl), (int32_t*)(d + o_ns), (int32_t*)(d + o_ov), (double*)(d + o_H), h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(shortlist, d + o_sl, sizeof(int32_t) * R * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(n_short, d + o_ns, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  if (overlap) PTZ_HIP_TRY(hipMemcpyAsync(overlap, d + o_ov, sizeof(int32_t) * nq * nr, hipMemcpyDeviceToHost, h.st));
  if (H_slot) PTZ_HIP_TRY(hipMemcpyAsync(H_slot, d + o_H, sizeof(double) * 9 * R * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}
