// reloc_assemble_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_reloc_assemble.h in the order the
// kernels of ptz_reloc.hip use it: the selection as K rounds of "the largest key below the last one", the candidates slot after
// slot, the transfer and keep rule per candidate, the cameras -- so that it can be held to the numpy restatement
// (tests/reloc_assemble_util.py) without a GPU and the device to it.  Never part of the product library.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o libreloc_assemble_harness.so reloc_assemble_harness.cc
#include <stdint.h>

#include "../../ptz-calib_amd/csrc/ptz_reloc_assemble.h"

using namespace ptz;

extern "C" {

void h_reloc_rotations(int32_t n_ref, const double* ref_cams, double* ref_R)
{
  for (int r = 0; r < n_ref; ++r) rodrigues(ref_cams + 15 * (size_t)r + 4, ref_R + 9 * (size_t)r);
}

// one pixel: returns keep, writes the transferred pixel
int32_t h_reloc_transfer(const double* cam_r, const double* R_r, const double* R_a, double fa, int32_t dist, float u, float v, float* out)
{
  const RelocPixel p = reloc_transfer(cam_r, R_r, R_a, fa, dist, u, v);
  out[0] = p.u; out[1] = p.v;
  return p.keep ? 1 : 0;
}

// the whole assembly; the outputs as ptz_reloc_assemble has them.  Returns the kept matches.
int64_t h_reloc_assemble(int32_t n_query, int32_t n_pair, int32_t n_ref, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                         const int32_t* pair_ref, const int64_t* query_ptr, const double* ref_cams, const double* ref_R,
                         const int32_t* query_wh, int32_t factor_type, int32_t K, int32_t* sel_pair, int32_t* n_sel, int64_t* out_ptr,
                         float* out_uv_ref, float* out_uv_cur, int32_t* out_src, double* cam_ref, double* cam_cur)
{
  int64_t o = 0;
  out_ptr[0] = 0;
  for (int q = 0; q < n_query; ++q) {
    const int64_t lo = query_ptr[q], hi = query_ptr[q + 1];
    int32_t* sel = sel_pair + (int64_t)K * q;
    uint64_t prev = ~0ull;
    int ns = 0;
    int64_t total = 0;
    for (int s = 0; s < K; ++s) {
      uint64_t best = 0;
      for (int64_t j = 0; j < hi - lo; ++j) {
        const uint64_t key = reloc_key(reloc_pair_count(match_ptr, pair_ref, n_ref, lo + j), (int32_t)j);
        if (key < prev && key > best) best = key;
      }
      if (best == 0) break;
      sel[s] = (int32_t)(lo + reloc_key_pos(best));
      total += reloc_key_count(best);
      prev = best;
      ++ns;
    }
    for (int s = ns; s < K; ++s) sel[s] = -1;
    n_sel[q] = ns;
    int32_t r0 = 0;
    if (ns > 0) r0 = pair_ref[sel[0]];
    else if (hi > lo) r0 = pair_ref[lo];
    reloc_cameras(ref_cams + 15 * (int64_t)r0, query_wh[2 * q], query_wh[2 * q + 1], K, cam_ref + 15 * (int64_t)q, cam_cur + 15 * (int64_t)q);
    for (int64_t i = 0; i < total; ++i) {
      int32_t p;
      int64_t src;
      reloc_locate(match_ptr, sel, ns, i, &p, &src);
      RelocPixel px = {uv_ref[2 * src], uv_ref[2 * src + 1], true};
      if (K > 1) {
        const int32_t r = pair_ref[p], a = pair_ref[sel[0]];
        px = reloc_transfer(ref_cams + 15 * (int64_t)r, ref_R + 9 * (int64_t)r, ref_R + 9 * (int64_t)a, ref_cams[15 * (int64_t)a], factor_type & 1,
                            uv_ref[2 * src], uv_ref[2 * src + 1]);
      }
      if (!px.keep) continue;
      out_uv_ref[2 * o] = px.u; out_uv_ref[2 * o + 1] = px.v;
      out_uv_cur[2 * o] = uv_cur[2 * src]; out_uv_cur[2 * o + 1] = uv_cur[2 * src + 1];
      out_src[o] = (int32_t)src;
      ++o;
    }
    out_ptr[q + 1] = o;
  }
  return o;
}
}
