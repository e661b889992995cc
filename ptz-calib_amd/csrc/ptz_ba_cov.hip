// ptz_ba_cov.hip -- covariance of bundle-adjusted cameras on MI355X (gfx950): ONE pipeline in two variants.  2D-2D: the per-view
// covariance of ptz_ba_cov.h, block dimension NF.  GEO: the georeferenced cameras and the rig centre of ptz_ba_cov_georef.h, block
// dimension NC = NF + 1 with the six T_l_w columns bordering the system.  One driver (cov_run) groups the problems, lays out a
// group's workspace (CovLayout), enqueues the group (enqueue_group) and reads back; a CovVariant says what differs.
//
// Per group of problems (as many as fit the workspace budget, PTZ_BA_COV_MAX_MB), on the batch's stream:
//   cam        camera blocks (R, intrinsics, Jl) at the state, n; GEO: the T_l_w block                       [thread / camera]
//   ray        P_r per ray; E_o, Y_o, the diagonal term and |e_o|^2 per observation; the squared residuals
//              are summed per wave of 64 rays by the butterfly, the waves of a problem in wave order      [thread / ray]
//   annot      GEO: a camera's annotations: records (A_a, G_a, |e_a|^2), then A^T A and A^T G summed over the
//              camera's annotations in stored order, one lane per element                                  [wave / camera]
//   reduce     GEO: (L, L) = sum G^T G and SSE_2d3d in stored order, the annotated cameras, the two variances [wave / problem]
//   assemble   block row ci of S and T: the diagonal block over the camera's observation list (cov_diag_sum), block (ci, cj)
//              over the pair's entry list (cov_pair_blocks), both in stored order, one lane per element -- no atomics.  GEO: T is
//              M = s_f^2 T_f + s_a^2 T_a, the 2D-2D columns sit at ba_geo_pos, plus the border (ci, L) and its mirror [workgroup / camera]
//   scale      identity rows / columns (the gauge; GEO: the dead fy columns), unit diagonal                [workgroup / row]
//   cholesky   chol_factor_solve (dense path, right-hand side zero): L in the strictly-lower tiles, the
//              inverses of the factored diagonal tiles in Linv
//   tri_inv    X = L^-1 by 64 x 64 tiles: X_jj = Linv_jj, X_ij = -Linv_ii sum_{k = j}^{i-1} L_ik X_kj     [workgroup / block column]
//   gemm       S^-1 = X^T X, then G = S^-1 T, on v_mfma_f64_16x16x4_f64                                    [workgroup / tile]
//   finish     2D-2D: diagonal blocks of G S^-1 (O(n^2 NF)), unscaling, left-perturbation form, s^2.  GEO: blocks (c, c), (c, L),
//              (L, L), unscaling, the world block; camera 0: the centre                                    [wave / camera]
// Every sum has one order that depends on the problem alone (a tile's k loop runs over the problem's own tiles, not the
// group's padded order), so a problem's bits do not depend on its position in the batch, on the grouping or on the run.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_host_batch.h"
#include "ptz_ba_cov.h"
#include "ptz_ba_cov_georef.h"

namespace ptz {

namespace {

constexpr int NB = CHOL_NB;
constexpr int LD = NB + 2;  // LDS row stride in doubles (as ptz_chol.hip)
typedef double d4 __attribute__((ext_vector_type(4)));

struct BaCovWork {  // one group of problems
  int first, count, np;  // first problem of the group, problems, padded order of the group's matrices
  int cam_lo, obs_lo;    // first camera / observation of the group (global indices)
  int max_waves;         // slots of squared-residual partials per problem
  double *A, *T, *X, *Si;  // [count][np][np]: S -> L -> G;  T;  L^-1;  S^-1
  double* Linv;            // [count][np / NB][NB * NB]
  double* dsc;             // [count][np] 1 / sqrt(S_ii)
  double* camblk;          // [cameras of the group][CAMBLK]
  double* EY;              // [observations of the group][6 NF]: E_o, Y_o
  double* Dg;              // [observations of the group][NF NF + 1]: the diagonal term (lower triangle read), w_r
  double* sse_part;        // [count][max_waves]
  double* sse;             // [count]
  int* n;                  // [count] NF n_cam
  int* flags;              // [count] kBaCov* bits
  const int* gauge;        // [count]
  double* cov;             // [cameras of the group][NF NF]
  double* sig;             // [count] sigma0
  double pixel_sigma;
  // the georeferenced variant only (ptz_ba_cov_georef.h)
  int o3_lo;               // first annotation of the group (global index)
  double* tlwblk;          // [count][TLWBLK]
  double* arec;            // [annotations of the group][ba_geo_rec(NC)]: A_a, G_a, |e_a|^2
  double* asum;            // [cameras of the group][NC NC + 6 NC]: the camera's annotation sums A^T A, A^T G
  int* live;               // [cameras of the group] 1: the camera has annotations, its fy column is live
  double* var;             // [count][4]: s_f^2 and s_a^2 of M, then the two estimates
  int* n_ann;              // [count] annotated cameras
  double* cen;             // [count][9]
  double annotation_sigma;
};

// nc: the block dimension (NF; GEO: NF + 1, and the six T_l_w columns border the system)
template <bool GEO>
__global__ void k_ba_cov_cam(BaCovIn in, BaGeoIn geo, BaCovWork w, int nc)
{
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[w.first + g];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) {
    w.n[g] = nc * s.n_cam + (GEO ? 6 : 0);
    if (GEO) ba_geo_tlwblk(geo.tlw_x + (size_t)s.cur * geo.tlw_stride + (size_t)s.idx * 6, w.tlwblk + (size_t)g * TLWBLK);
  }
  if (c >= s.n_cam) return;
  const double* c15 = in.cam_x + (size_t)s.cur * in.cam_stride + (size_t)(s.cam_off + c) * 15;
  ba_cov_camblk(c15, w.camblk + (size_t)(s.cam_off + c - w.cam_lo) * CAMBLK);
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_ba_cov_ray(BaCovIn in, BaCovWork w)
{
  constexpr int NF = BaDims<TYPE>::NC, NE = NF * NF;
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[w.first + g];
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int wave = j >> 6;
  if (wave * 64 >= s.n_ray) return;  // (whole waves leave; the butterfly below needs the 64 lanes of a wave that stays)
  double sse = 0;
  if (j < s.n_ray) {
    const int* rp = in.ray_ptr + s.ray_off + s.idx;
    const int a0 = rp[j], a1 = rp[j + 1];
    const double* xp = in.ray_x + (size_t)s.cur * in.ray_stride + (size_t)(s.ray_off + j) * 3;
    const double X[3] = {xp[0], xp[1], xp[2]};
    const double wr = in.ray_w[s.ray_off + j];
    const double* cbs = w.camblk + (size_t)(s.cam_off - w.cam_lo) * CAMBLK;
    double V[6] = {0, 0, 0, 0, 0, 0};
    bool penalty = false;
    for (int a = a0; a < a1; ++a) {
      const double* cb = cbs + (size_t)in.obs_cam[a] * CAMBLK;
      const float2 uv = in.obs_uv[a];
      double res[2], Jc[2][NF], Jr[2][3];
      ba_linearize<TYPE>(cb, X, uv.x, uv.y, res, Jc, Jr);
      if (TYPE == 1) penalty = penalty || (cb[CB_R + 6] * X[0] + cb[CB_R + 7] * X[1] + cb[CB_R + 8] * X[2] < 0);
      ba_cov_add_V(Jr, V);
      sse += res[0] * res[0] + res[1] * res[1];
    }
    // a ray with one candidate observation contributes exactly zero to S and T: its records are zero, not computed
    const bool coupled = a1 - a0 >= 2;
    double P[6] = {0, 0, 0, 0, 0, 0};
    const bool ok = coupled && ba_cov_ray_P(V, wr, X, P);
    if (penalty || (coupled && !ok)) atomicOr(&w.flags[g], penalty ? kBaCovPenalty : kBaCovBadRay);
    for (int a = a0; a < a1; ++a) {
      double* ey = w.EY + (size_t)(a - w.obs_lo) * (6 * NF);
      double* dg = w.Dg + (size_t)(a - w.obs_lo) * (NE + 1);
      dg[NE] = wr;
      if (!ok) {
#pragma unroll
        for (int k = 0; k < 6 * NF; ++k) ey[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NE; ++k) dg[k] = 0.0;
        continue;
      }
      const double* cb = cbs + (size_t)in.obs_cam[a] * CAMBLK;
      const float2 uv = in.obs_uv[a];
      double res[2], Jc[2][NF], Jr[2][3], E[3 * NF], Y[3 * NF];
      ba_linearize<TYPE>(cb, X, uv.x, uv.y, res, Jc, Jr);
      ba_cov_E<NF>(Jc, Jr, wr, E);
      ba_cov_Y<NF>(E, P, Y);
#pragma unroll
      for (int k = 0; k < 3 * NF; ++k) { ey[k] = E[k]; ey[3 * NF + k] = Y[k]; }
#pragma unroll
      for (int k = 0; k < NF; ++k)
#pragma unroll
        for (int l = 0; l < NF; ++l) dg[k * NF + l] = ba_cov_diag_term<NF>(Jc, wr, Y, E, k, l);
    }
  }
  sse = wave_sum(sse);
  if ((threadIdx.x & 63) == 0) w.sse_part[(size_t)g * w.max_waves + wave] = sse;
}

__global__ void k_ba_cov_sse(BaCovIn in, BaCovWork w)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= w.count) return;
  const int nw = (in.scene[w.first + g].n_ray + 63) / 64;
  double t = 0;
  for (int i = 0; i < nw; ++i) t += w.sse_part[(size_t)g * w.max_waves + i];
  w.sse[g] = t;
}

// element el of the diagonal term summed over a camera's observation list (o0, no) in stored order: into S, times w_r into T
template <int NF>
__device__ __forceinline__ void cov_diag_sum(const BaCovIn& in, const BaCovWork& w, int o0, int no, int el, double& sS, double& sT)
{
  constexpr int NE = NF * NF;
  for (int q = 0; q < no; ++q) {
    const double* dg = w.Dg + (size_t)(in.cam_obs[o0 + q] - w.obs_lo) * (NE + 1);
    const double v = dg[el];
    sS += v;
    sT += dg[NE] * v;
  }
}

// blocks (ci, cj), cj < ci, of S and T and their mirrors, each over the pair's entries in stored order, one lane per element; the
// waves take the camera's pairs in turn.  Row stride NC = NF (GEO: NF + 1, the NF columns at ba_geo_pos, T's terms times vf).
template <int NF, bool GEO>
__device__ __forceinline__ void cov_pair_blocks(const BaCovIn& in, const BaCovWork& w, const BaCovScene& s, const int* cp, int ci, int o0, double* A,
                                                double* T, double vf)
{
  constexpr int NE = NF * NF, NC = NF + (GEO ? 1 : 0);
  const int np = w.np;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int* cpair = in.cam_pair + s.cam_off + s.idx;
  const int pr0 = cpair[ci], npr = cpair[ci + 1] - pr0;
  const int* pps = in.pair_ptr + s.pair_off + s.idx + pr0;
  const int* pcj = in.pair_cj + s.pair_off + pr0;
  if (lane >= NE) return;
  const int k = lane / NF, l = lane % NF;
  for (int pl = wv; pl < npr; pl += 4) {
    const int cj = pcj[pl], e0 = pps[pl], e1 = pps[pl + 1];
    if (cj < 0 || cj >= ci) continue;
    const int oj = cp[cj];
    double sS = 0, sT = 0;
    for (int e = e0; e < e1; ++e) {
      const unsigned ab = in.ent[e];
      const size_t a = (size_t)(in.cam_obs[o0 + (int)(ab & 0xffffu)] - w.obs_lo), b = (size_t)(in.cam_obs[oj + (int)(ab >> 16)] - w.obs_lo);
      const double v = ba_cov_pair_term(w.EY + a * (6 * NF) + 3 * NF, w.EY + b * (6 * NF), k, l);
      sS += v;
      sT += w.Dg[a * (NE + 1) + NE] * v;
    }
    const size_t r = (size_t)(ci * NC + (GEO ? ba_geo_pos(k) : k)), c = (size_t)(cj * NC + (GEO ? ba_geo_pos(l) : l));
    const double t = GEO ? vf * sT : sT;
    A[r * np + c] = sS; A[c * np + r] = sS;
    T[r * np + c] = t; T[c * np + r] = t;
  }
}

template <int NF>
__global__ __launch_bounds__(256) void k_ba_cov_assemble(BaCovIn in, BaCovWork w)
{
  constexpr int NE = NF * NF;
  const int g = blockIdx.y, ci = blockIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  if (ci >= s.n_cam) return;
  const int np = w.np;
  double* A = w.A + (size_t)g * np * np;
  double* T = w.T + (size_t)g * np * np;
  const int* cp = in.cam_ptr + s.cam_off + s.idx;
  const int o0 = cp[ci], no = cp[ci + 1] - o0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k = lane / NF, l = lane % NF;
  if (wv == 0 && lane < NE) {  // the diagonal block over the camera's observation list
    double sS = 0, sT = 0;
    cov_diag_sum<NF>(in, w, o0, no, k >= l ? k * NF + l : l * NF + k, sS, sT);  // (the lower triangle's element for both halves: symmetric bit for bit)
    A[(size_t)(ci * NF + k) * np + ci * NF + l] = sS;
    T[(size_t)(ci * NF + k) * np + ci * NF + l] = sT;
    if (k == l) {
      const bool anchor_rot = ci == w.gauge[g] && k >= NF - 3;
      const bool ok = anchor_rot || (sS > 0.0 && isfinite(sS));
      if (!ok) atomicOr(&w.flags[g], kBaCovBadDiag);
      w.dsc[(size_t)g * np + ci * NF + k] = (ok && !anchor_rot) ? 1.0 / sqrt(sS) : 1.0;
    }
  }
  cov_pair_blocks<NF, false>(in, w, s, cp, ci, o0, A, T, 1.0);
}

// identity rows / columns (the gauge; GEO: the dead fy columns too -- identity in S, zero in T), then both matrices to the unit
// diagonal of S
template <bool GEO>
__global__ __launch_bounds__(256) void k_ba_cov_scale(BaCovIn in, BaCovWork w, int nc)
{
  const int g = blockIdx.y, i = blockIdx.x;
  const int n = w.n[g], np = w.np;
  if (i >= n) return;
  const int r0 = w.gauge[g] * nc + nc - 3;
  int nL = 0;
  const int* live = nullptr;
  if (GEO) {
    const BaCovScene s = in.scene[w.first + g];
    nL = nc * s.n_cam;
    live = w.live + (s.cam_off - w.cam_lo);
  }
  auto ident = [&](int j) { return (j >= r0 && j < r0 + 3) || (GEO && j < nL && j % nc == 1 && !live[j / nc]); };
  double* A = w.A + (size_t)g * np * np + (size_t)i * np;
  double* T = w.T + (size_t)g * np * np + (size_t)i * np;
  const double* sc = w.dsc + (size_t)g * np;
  const double si = sc[i];
  const bool gi = ident(i);
  for (int j = threadIdx.x; j < n; j += 256) {
    if (gi || ident(j)) { A[j] = i == j ? 1.0 : 0.0; T[j] = 0.0; }
    else { const double f = si * sc[j]; A[j] *= f; T[j] *= f; }
  }
}

// ---- 64 x 64 tile products on the matrix cores -------------------------------------------------------------------------------------
// global tile (row stride ld) -> LDS (row stride LD), as it is or transposed; 256 threads, 16 bytes per lane and pass
template <bool TRANS, bool NEGATE>
__device__ __forceinline__ void cov_g2s(const double* __restrict__ gsrc, int ld, double* s)
{
#pragma unroll
  for (int p = 0; p < (NB * NB / 2) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int row = idx >> 5, c2 = (idx & 31) * 2;
    double2 v = *reinterpret_cast<const double2*>(gsrc + (size_t)row * ld + c2);
    if (NEGATE) { v.x = -v.x; v.y = -v.y; }
    if (TRANS) { s[c2 * LD + row] = v.x; s[(c2 + 1) * LD + row] = v.y; }
    else *reinterpret_cast<double2*>(s + row * LD + c2) = v;
  }
}
// acc += As Bs^T: As[m][k], Bs[n][k]; wave wv owns rows [16 wv, 16 wv + 16); acc[c][i] = element (16 wv + fq + 4 i, 16 c + fr)
__device__ __forceinline__ void cov_mma(const double* As, const double* Bs, d4 (&acc)[4])
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const double* ap = As + (16 * wv + fr) * LD + fq;
  const double* bp = Bs + fr * LD + fq;
#pragma unroll
  for (int kk = 0; kk < NB / 4; ++kk) {
    const double av = ap[4 * kk];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * c) * LD + 4 * kk], acc[c], 0, 0, 0);
  }
}
__device__ __forceinline__ void cov_store(const d4 (&acc)[4], double* __restrict__ C, int ld)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(size_t)(16 * wv + fq + 4 * i) * ld + 16 * c + fr] = acc[c][i];
}

// X = L^-1, block column j: the tiles below the diagonal follow one another (X_ij needs X_kj, k < i), the block columns are
// independent.  L_ik: strictly-lower tiles of A; Linv: inverses of the factored diagonal tiles.
__global__ __launch_bounds__(256) void k_ba_cov_tri_inv(BaCovWork w)
{
  const int g = blockIdx.y, j = blockIdx.x;
  const int np = w.np, nt = np / NB;
  const int nts = w.n[g] / NB + 1;  // the problem's own tiles (the one that holds row n included)
  if (j >= nts) return;
  const double* L = w.A + (size_t)g * np * np;
  const double* Li = w.Linv + (size_t)g * nt * (NB * NB);
  double* X = w.X + (size_t)g * np * np;
  __shared__ __attribute__((aligned(16))) double As[NB * LD];
  __shared__ __attribute__((aligned(16))) double Bs[NB * LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  {  // X_jj
    const double* src = Li + (size_t)j * (NB * NB);
    double* dst = X + (size_t)(j * NB) * np + j * NB;
    for (int idx = threadIdx.x; idx < NB * NB; idx += 256) dst[(size_t)(idx >> 6) * np + (idx & 63)] = src[idx];
  }
  __threadfence_block();
  __syncthreads();  // (the tiles this workgroup wrote are read back by it below)
  for (int i = j + 1; i < nts; ++i) {
    d4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k = j; k < i; ++k) {
      cov_g2s<false, false>(L + (size_t)(i * NB) * np + k * NB, np, As);  // L_ik
      cov_g2s<true, false>(X + (size_t)(k * NB) * np + j * NB, np, Bs);   // X_kj, as Bs[n][k]
      __syncthreads();
      cov_mma(As, Bs, acc);
      __syncthreads();
    }
    // X_ij = -Linv_ii acc: the accumulator becomes the second operand
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) Bs[(16 * c + fr) * LD + 16 * wv + fq + 4 * r] = acc[c][r];
    cov_g2s<false, true>(Li + (size_t)i * (NB * NB), NB, As);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
    cov_mma(As, Bs, acc);
    cov_store(acc, X + (size_t)(i * NB) * np + j * NB, np);
    __threadfence_block();
    __syncthreads();
  }
}

// MODE 0: Si = X^T X, tile (i, j) = sum_{k >= max(i, j)} X_ki^T X_kj.  MODE 1: G = Si T, tile (i, j) = sum_k Si_ik T_kj (T symmetric:
// T_kj^T = T_jk), written into A, whose L is no longer needed.  k runs over the problem's own tiles.
template <int MODE>
__global__ __launch_bounds__(256) void k_ba_cov_gemm(BaCovWork w)
{
  const int g = blockIdx.y;
  const int np = w.np, nt = np / NB;
  const int nts = w.n[g] / NB + 1;
  const int i = blockIdx.x / nt, j = blockIdx.x % nt;
  if (i >= nts || j >= nts) return;
  const size_t off = (size_t)g * np * np;
  __shared__ __attribute__((aligned(16))) double As[NB * LD];
  __shared__ __attribute__((aligned(16))) double Bs[NB * LD];
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k = MODE == 0 ? max(i, j) : 0; k < nts; ++k) {
    if (MODE == 0) {
      cov_g2s<true, false>(w.X + off + (size_t)(k * NB) * np + i * NB, np, As);
      cov_g2s<true, false>(w.X + off + (size_t)(k * NB) * np + j * NB, np, Bs);
    }
    else {
      cov_g2s<false, false>(w.Si + off + (size_t)(i * NB) * np + k * NB, np, As);
      cov_g2s<false, false>(w.T + off + (size_t)(j * NB) * np + k * NB, np, Bs);
    }
    __syncthreads();
    cov_mma(As, Bs, acc);
    __syncthreads();
  }
  cov_store(acc, (MODE == 0 ? w.Si : w.A) + off + (size_t)(i * NB) * np + j * NB, np);
}

// the camera's diagonal block of G S^-1 (row k of G against row l of the symmetric S^-1), unscaled, converted, times s^2
template <int TYPE>
__global__ __launch_bounds__(64) void k_ba_cov_finish(BaCovIn in, BaCovWork w)
{
  constexpr int NF = BaDims<TYPE>::NC, NE = NF * NF, NH = NF * (NF + 1) / 2;
  const int g = blockIdx.y, c = blockIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  if (c >= s.n_cam) return;
  const int np = w.np, n = w.n[g];
  const double* G = w.A + (size_t)g * np * np + (size_t)(c * NF) * np;
  const double* Si = w.Si + (size_t)g * np * np + (size_t)(c * NF) * np;
  double acc[NH];
#pragma unroll
  for (int e = 0; e < NH; ++e) acc[e] = 0;
  for (int j = threadIdx.x; j < n; j += 64) {
    double gk[NF], sk[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) { gk[k] = G[(size_t)k * np + j]; sk[k] = Si[(size_t)k * np + j]; }
    int e = 0;
#pragma unroll
    for (int k = 0; k < NF; ++k)
#pragma unroll
      for (int l = 0; l <= k; ++l) acc[e++] += gk[k] * sk[l];
  }
#pragma unroll
  for (int e = 0; e < NH; ++e) acc[e] = wave_sum(acc[e]);
  if (threadIdx.x != 0) return;
  const double* sc = w.dsc + (size_t)g * np + c * NF;
  double Cr[NE];
  {
    int e = 0;
#pragma unroll
    for (int k = 0; k < NF; ++k)
#pragma unroll
      for (int l = 0; l <= k; ++l) {  // (ba_cov_to_left reads the lower triangle)
        if (l < k) Cr[l * NF + k] = 0.0;
        Cr[k * NF + l] = acc[e++] * sc[k] * sc[l];
      }
  }
  const double dof = (double)ba_cov_dof(NF, s.n_cam, s.n_ray, s.n_obs);
  const double s2 = w.sse[g] / dof;
  const double var = w.pixel_sigma > 0.0 ? w.pixel_sigma * w.pixel_sigma : s2;
  double out[NE];
  const bool fin = ba_cov_to_left<TYPE>(Cr, w.camblk + (size_t)(s.cam_off + c - w.cam_lo) * CAMBLK + CB_JL, var, c == w.gauge[g], out);
  if (!fin || !isfinite(s2)) atomicOr(&w.flags[g], kBaCovNonFinite);
  double* o = w.cov + (size_t)(s.cam_off + c - w.cam_lo) * NE;
#pragma unroll
  for (int e = 0; e < NE; ++e) o[e] = out[e];
  if (c == 0) w.sig[g] = sqrt(s2);
}

// ==== the kernels of the georeferenced variant alone (definition: ptz_ba_cov_georef.h) ============================================
// M is ONE matrix in absolute units: both variances are known before the assembly (the residuals are summed by the kernels that
// linearise), so there is one product S^-1 M, no second n x n matrix, and no ratio s_a^2 / s_f^2 that an exact fit would make 0 / 0.
template <int TYPE>
__global__ __launch_bounds__(64) void k_geo_annot(BaCovIn in, BaGeoIn geo, BaCovWork w)
{
  constexpr int NC = BaDims<TYPE>::NC + 1, REC = ba_geo_rec(NC), NA = NC * NC + 6 * NC;
  const int g = blockIdx.y, c = blockIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  if (c >= s.n_cam) return;
  const size_t gc = (size_t)(s.cam_off + c - w.cam_lo);
  const double* cb = w.camblk + gc * CAMBLK;
  const double* tb = w.tlwblk + (size_t)g * TLWBLK;
  const int* oc = geo.o3_cam + s.o3_off;
  double* rec0 = w.arec + (size_t)(s.o3_off - w.o3_lo) * REC;
  int mine = 0, behind = 0;
  for (int a = threadIdx.x; a < s.n_o3; a += 64) {
    if (oc[a] != c) continue;
    mine = 1;
    const size_t ga = (size_t)s.o3_off + a;
    const float2 uv = geo.o3_uv[ga];
    const double xyz[3] = {geo.o3_xyz[3 * ga], geo.o3_xyz[3 * ga + 1], geo.o3_xyz[3 * ga + 2]};
    if (!ba_geo_annot<TYPE>(cb, tb, xyz, uv.x, uv.y, rec0 + (size_t)a * REC)) behind = 1;
  }
  if (behind) atomicOr(&w.flags[g], kBaCovBehind);
  __threadfence_block();
  __syncthreads();  // (the records this wave wrote are read back by it below)
  for (int e = threadIdx.x; e < NA; e += 64) {
    double sum = 0;
    for (int a = 0; a < s.n_o3; ++a) {
      if (oc[a] != c) continue;
      const double* rec = rec0 + (size_t)a * REC;
      sum += e < NC * NC ? ba_geo_cc(rec, NC, e / NC, e % NC) : ba_geo_cl(rec, NC, (e - NC * NC) / 6, (e - NC * NC) % 6);
    }
    w.asum[gc * NA + e] = sum;
  }
  mine = __any(mine);
  if (threadIdx.x == 0) w.live[gc] = mine ? 1 : 0;
}

template <int TYPE>
__global__ __launch_bounds__(64) void k_geo_reduce(BaCovIn in, BaCovWork w)
{
  constexpr int NF = BaDims<TYPE>::NC, NC = NF + 1, REC = ba_geo_rec(NC);
  const int g = blockIdx.x, lane = threadIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  const double* rec0 = w.arec + (size_t)(s.o3_off - w.o3_lo) * REC;
  __shared__ double va;
  if (lane == 63) {
    double t = 0;
    for (int a = 0; a < s.n_o3; ++a) t += rec0[(size_t)a * REC + 2 * NC + 12];
    int na = 0;
    for (int c = 0; c < s.n_cam; ++c) na += w.live[s.cam_off + c - w.cam_lo];
    double est2[2], var[2];
    ba_geo_noise(NF, s.n_cam, s.n_ray, s.n_obs, s.n_o3, na, w.sse[g], t, w.pixel_sigma, w.annotation_sigma, est2, var);
    double* o = w.var + 4 * (size_t)g;
    o[0] = var[0]; o[1] = var[1]; o[2] = est2[0]; o[3] = est2[1];
    w.n_ann[g] = na;
    va = var[1];
  }
  const int m = lane / 6, q = lane % 6;
  double sum = 0;
  if (lane < 36)
    for (int a = 0; a < s.n_o3; ++a) sum += ba_geo_ll(rec0 + (size_t)a * REC, NC, m >= q ? m : q, m >= q ? q : m);
  __syncthreads();
  if (lane >= 36) return;
  const int np = w.np, nL = NC * s.n_cam;
  const size_t e = (size_t)g * np * np + (size_t)(nL + m) * np + nL + q;
  w.A[e] = sum;
  w.T[e] = va * sum;
  if (m == q) {
    const bool ok = sum > 0.0 && isfinite(sum);
    if (!ok) atomicOr(&w.flags[g], kBaCovBadDiag);
    w.dsc[(size_t)g * np + nL + m] = ok ? 1.0 / sqrt(sum) : 1.0;
  }
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_geo_assemble(BaCovIn in, BaCovWork w)
{
  constexpr int NF = BaDims<TYPE>::NC, NC = NF + 1, NA = NC * NC + 6 * NC;
  const int g = blockIdx.y, ci = blockIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  if (ci >= s.n_cam) return;
  const int np = w.np, nL = NC * s.n_cam;
  double* A = w.A + (size_t)g * np * np;
  double* T = w.T + (size_t)g * np * np;
  const double vf = w.var[4 * (size_t)g], va = w.var[4 * (size_t)g + 1];
  const size_t gc = (size_t)(s.cam_off + ci - w.cam_lo);
  const double* as = w.asum + gc * NA;
  const int* cp = in.cam_ptr + s.cam_off + s.idx;
  const int o0 = cp[ci], no = cp[ci + 1] - o0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (wv == 0 && lane < NC * NC) {  // the diagonal block: the 2D-2D terms over the camera's observation list, then its annotations' sum
    const int k = lane / NC, l = lane % NC;
    const int kk = k >= l ? k : l, ll = k >= l ? l : k;  // (the lower triangle's element for both halves: symmetric bit for bit)
    double sS = 0, sT = 0;
    if (k != 1 && l != 1) cov_diag_sum<NF>(in, w, o0, no, (kk ? kk - 1 : 0) * NF + (ll ? ll - 1 : 0), sS, sT);  // (ba_geo_pos inverted)
    const double a = as[kk * NC + ll], d = sS + a;
    A[(size_t)(ci * NC + k) * np + ci * NC + l] = d;
    T[(size_t)(ci * NC + k) * np + ci * NC + l] = vf * sT + va * a;
    if (k == l) {
      const bool ident = (ci == w.gauge[g] && k >= NC - 3) || (k == 1 && !w.live[gc]);
      const bool ok = ident || (d > 0.0 && isfinite(d));
      if (!ok) atomicOr(&w.flags[g], kBaCovBadDiag);
      w.dsc[(size_t)g * np + ci * NC + k] = (ok && !ident) ? 1.0 / sqrt(d) : 1.0;
    }
  }
  if (wv == 1 && lane < 6 * NC) {  // the border (ci, L) and its mirror
    const double a = as[NC * NC + lane];
    const size_t r = (size_t)(ci * NC + lane / 6), c = (size_t)(nL + lane % 6);
    A[r * np + c] = a; A[c * np + r] = a;
    T[r * np + c] = va * a; T[c * np + r] = va * a;
  }
  cov_pair_blocks<NF, true>(in, w, s, cp, ci, o0, A, T, vf);
}

// Z = the blocks (c, c), (c, L), (L, L) of G S^-1 (row p of G against row q of the symmetric S^-1), unscaled; the world block
// W Z W^T, one lane per element; camera 0 also writes the centre's covariance
template <int TYPE>
__global__ __launch_bounds__(64) void k_geo_finish(BaCovIn in, BaCovWork w)
{
  constexpr int NF = BaDims<TYPE>::NC, NE = NF * NF, NC = NF + 1, NZ = NC + 6, NH = NZ * (NZ + 1) / 2;
  const int g = blockIdx.y, c = blockIdx.x;
  const BaCovScene s = in.scene[w.first + g];
  if (c >= s.n_cam) return;
  const int np = w.np, n = w.n[g], nL = NC * s.n_cam;
  const double* G = w.A + (size_t)g * np * np;
  const double* Si = w.Si + (size_t)g * np * np;
  double acc[NH];
#pragma unroll
  for (int e = 0; e < NH; ++e) acc[e] = 0;
  for (int j = threadIdx.x; j < n; j += 64) {
    double gk[NZ], sk[NZ];
#pragma unroll
    for (int p = 0; p < NZ; ++p) {
      const size_t row = (size_t)(p < NC ? c * NC + p : nL + p - NC) * np;
      gk[p] = G[row + j]; sk[p] = Si[row + j];
    }
    int e = 0;
#pragma unroll
    for (int p = 0; p < NZ; ++p)
#pragma unroll
      for (int q = 0; q <= p; ++q) acc[e++] += gk[p] * sk[q];
  }
#pragma unroll
  for (int e = 0; e < NH; ++e) acc[e] = wave_sum(acc[e]);
  __shared__ double Z[NZ * NZ], W[NF * NZ], J[18], cen[3];
  const double* sc = w.dsc + (size_t)g * np;
  const size_t gc = (size_t)(s.cam_off + c - w.cam_lo);
  const double* tb = w.tlwblk + (size_t)g * TLWBLK;
  if (threadIdx.x == 0) {
    int e = 0;
#pragma unroll
    for (int p = 0; p < NZ; ++p)
#pragma unroll
      for (int q = 0; q <= p; ++q) {
        const double v = acc[e++] * sc[p < NC ? c * NC + p : nL + p - NC] * sc[q < NC ? c * NC + q : nL + q - NC];
        Z[p * NZ + q] = v; Z[q * NZ + p] = v;
      }
    const double* cb = w.camblk + gc * CAMBLK;
    ba_geo_world_W<TYPE>(cb + CB_JL, cb + CB_R, tb, W);
    ba_geo_centre_J(tb, cen, J);
  }
  __syncthreads();
  bool fin = true;
  if (threadIdx.x < NE) {
    const int k = threadIdx.x / NF, l = threadIdx.x % NF;
    const double v = ba_geo_quad(W + (k >= l ? k : l) * NZ, W + (k >= l ? l : k) * NZ, Z, NZ, NZ);
    fin = isfinite(v);
    w.cov[gc * NE + threadIdx.x] = v;
  }
  else if (c == 0 && threadIdx.x < NE + 9) {
    const int i = (threadIdx.x - NE) / 3, j = (threadIdx.x - NE) % 3;
    const double v = ba_geo_quad(J + 6 * (i >= j ? i : j), J + 6 * (i >= j ? j : i), Z + NC * NZ + NC, 6, NZ);
    fin = isfinite(v);
    w.cen[9 * (size_t)g + threadIdx.x - NE] = v;
  }
  else if (c == 0 && threadIdx.x == 63) {
    const double* v4 = w.var + 4 * (size_t)g;
    fin = isfinite(v4[2]) && isfinite(v4[3]);
    w.sig[2 * (size_t)g] = sqrt(v4[2]); w.sig[2 * (size_t)g + 1] = sqrt(v4[3]);
  }
  if (!fin) atomicOr(&w.flags[g], kBaCovNonFinite);
}

// one group's launches; GEO selects the variant's kernels at compile time
template <int TYPE, bool GEO>
void enqueue_group(const BaCovIn& in, const BaGeoIn& geo, const BaCovWork& w, const CholBatch& cb, double* x, int max_cam, int max_ray, int max_n,
                   hipStream_t st)
{
  constexpr int NF = BaDims<TYPE>::NC, NC = NF + (GEO ? 1 : 0);
  const int nt = w.np / NB;
  hipLaunchKernelGGL(k_ba_cov_cam<GEO>, dim3((max_cam + 63) / 64, w.count), dim3(64), 0, st, in, geo, w, NC);
  chol_clear(cb, st);  // zero, padding rows, fail flags (reads n)
  hipLaunchKernelGGL(k_ba_cov_ray<TYPE>, dim3((max_ray + 255) / 256, w.count), dim3(256), 0, st, in, w);
  hipLaunchKernelGGL(k_ba_cov_sse, dim3((w.count + 63) / 64), dim3(64), 0, st, in, w);
  if constexpr (GEO) {
    hipLaunchKernelGGL(k_geo_annot<TYPE>, dim3(max_cam, w.count), dim3(64), 0, st, in, geo, w);
    hipLaunchKernelGGL(k_geo_reduce<TYPE>, dim3(w.count), dim3(64), 0, st, in, w);
    hipLaunchKernelGGL(k_geo_assemble<TYPE>, dim3(max_cam, w.count), dim3(256), 0, st, in, w);
  }
  else hipLaunchKernelGGL(k_ba_cov_assemble<NF>, dim3(max_cam, w.count), dim3(256), 0, st, in, w);
  hipLaunchKernelGGL(k_ba_cov_scale<GEO>, dim3(max_n, w.count), dim3(256), 0, st, in, w, NC);
  chol_factor_solve(cb, x, st);
  hipLaunchKernelGGL(k_ba_cov_tri_inv, dim3(nt, w.count), dim3(256), 0, st, w);
  hipLaunchKernelGGL(k_ba_cov_gemm<0>, dim3(nt * nt, w.count), dim3(256), 0, st, w);
  hipLaunchKernelGGL(k_ba_cov_gemm<1>, dim3(nt * nt, w.count), dim3(256), 0, st, w);
  if constexpr (GEO) hipLaunchKernelGGL(k_geo_finish<TYPE>, dim3(max_cam, w.count), dim3(64), 0, st, in, w);
  else hipLaunchKernelGGL(k_ba_cov_finish<TYPE>, dim3(max_cam, w.count), dim3(64), 0, st, in, w);
}

// ==== the driver ==================================================================================================================
// what differs between the two variants
struct CovVariant {
  int nf;        // entries per camera of the result
  int nc;        // block dimension of the reduced system: nf, georef nf + 1
  int border;    // columns bordering the system: 0, georef 6 (T_l_w)
  int n_sig;     // sigmas per problem: 1, georef 2
  bool centre;   // georef: annotations, the T_l_w block and the centre's covariance
  int (*status)(int nf, const BaCovScene& s, int n_ann, int chol_fail, int flags);
  void (*enqueue)(const BaCovIn&, const BaGeoIn&, const BaCovWork&, const CholBatch&, double* x, int max_cam, int max_ray, int max_n, hipStream_t);
};
int status_2d2d(int nf, const BaCovScene& s, int, int fail, int flags) { return ba_cov_status(nf, s.n_cam, s.n_ray, s.n_obs, fail, flags); }
int status_geo(int nf, const BaCovScene& s, int n_ann, int fail, int flags) { return ba_geo_status(nf, s.n_cam, s.n_ray, s.n_obs, s.n_o3, n_ann, fail, flags); }
template <int TYPE, bool GEO>
constexpr CovVariant kVariant = {BaDims<TYPE>::NC, BaDims<TYPE>::NC + (GEO ? 1 : 0), GEO ? 6 : 0, GEO ? 2 : 1, GEO, GEO ? status_geo : status_2d2d,
                                 enqueue_group<TYPE, GEO>};

// byte offsets of a group's buffers in its workspace, each aligned to 256 bytes (an empty buffer takes none)
struct CovLayout {
  size_t A, T, X, Si;                    // [count][np][np]
  size_t Ldiag, Linv, Dinv, x;           // the Cholesky's: diagonal tiles, their inverses, the 16 x 16 inverses, the (zero) solution
  size_t dsc, camblk, EY, Dg, sse_part, sse, cov, sig;
  size_t ints;                           // the int block, [count] each: at i_n, i_flags, i_gauge, i_fail (georef: i_n_ann) ints from `ints`
  size_t tlwblk, arec, asum, live, var, cen;  // georef only
  size_t i_n, i_flags, i_gauge, i_fail, i_n_ann, n_ints;
};
// lays out a group of `count` problems of padded order np over `cams` cameras, `obs` observation slots, `o3` annotations and `waves`
// partial sums per problem; returns the bytes.  Sizes a candidate group and places the chosen one.
size_t cov_layout(const CovVariant& v, size_t count, size_t np, size_t cams, size_t obs, size_t o3, size_t waves, CovLayout& l)
{
  const size_t nt = np / NB, ne = (size_t)v.nf * v.nf, geo = v.centre ? 1 : 0, D = sizeof(double);
  size_t o = 0;
  auto take = [&o](size_t& slot, size_t bytes) { slot = o; o += up256(bytes); };
  take(l.A, D * count * np * np); take(l.T, D * count * np * np); take(l.X, D * count * np * np); take(l.Si, D * count * np * np);
  take(l.Ldiag, D * count * nt * NB * NB);
  take(l.Linv, D * count * nt * NB * NB);
  take(l.Dinv, D * count * nt * 4 * 16 * 16);
  take(l.x, D * count * np);
  take(l.dsc, D * count * np);
  take(l.camblk, D * cams * CAMBLK);
  take(l.EY, D * obs * 6 * v.nf);
  take(l.Dg, D * obs * (ne + 1));
  take(l.sse_part, D * count * waves);
  take(l.sse, D * count);
  take(l.cov, D * cams * ne);
  take(l.sig, D * count * v.n_sig);
  l.i_n = 0; l.i_flags = count; l.i_gauge = 2 * count; l.i_fail = 3 * count; l.i_n_ann = 4 * count; l.n_ints = (4 + geo) * count;
  take(l.ints, sizeof(int) * l.n_ints);
  take(l.tlwblk, geo * D * count * TLWBLK);
  take(l.arec, geo * D * (o3 + 1) * ba_geo_rec(v.nc));
  take(l.asum, geo * D * cams * (v.nc * v.nc + 6 * v.nc));
  take(l.live, geo * sizeof(int) * cams);
  take(l.var, geo * D * count * 4);
  take(l.cen, geo * D * count * 9);
  return o;
}

// bytes of workspace per group of problems (PTZ_BA_COV_MAX_MB, default 2048)
size_t cov_budget()
{
  if (const char* e = getenv("PTZ_BA_COV_MAX_MB")) return (size_t)std::max(1ll, atoll(e)) << 20;
  return (size_t)2048 << 20;
}

// Both variants: group by group under the budget -- lay out, enqueue, read back, hand the OK problems' results to the caller.
int cov_run(const CovVariant& v, const BaCovIn& in, const BaGeoIn& geo, const BaCovScene* hs, const int* gauge, double pixel_sigma,
            double annotation_sigma, hipStream_t st, double* cov, double* cov_centre, double* sigma0, int* status, double* device_ms)
{
  const int NE = v.nf * v.nf;
  const size_t budget = cov_budget();
  CallHeld h(st);  // a group's workspace and the two timing events, released once the stream is idle
  double total_ms = 0;
  for (int first = 0; first < in.n_scene;) {
    // the group: problems first .. first + count - 1, as many as the budget holds (one at least)
    int count = 0, max_cam = 0, max_ray = 0;
    size_t cams = 0, obs = 0, o3 = 0, bytes = 0;
    CovLayout l;
    for (int i = first; i < in.n_scene; ++i) {
      const int mc = std::max(max_cam, hs[i].n_cam), mr = std::max(max_ray, hs[i].n_ray);
      const size_t c2 = (size_t)(hs[i].cam_off + hs[i].n_cam - hs[first].cam_off), o2 = (size_t)(hs[i].obs_off + hs[i].n_obs - hs[first].obs_off);
      const size_t a2 = v.centre ? (size_t)(hs[i].o3_off + hs[i].n_o3 - hs[first].o3_off) : 0;
      const size_t b2 = cov_layout(v, (size_t)(i - first + 1), (size_t)chol_padded_order(v.nc * mc + v.border), c2, o2, a2, (size_t)(mr + 63) / 64 + 1, l);
      if (count > 0 && b2 > budget) break;
      count = i - first + 1; max_cam = mc; max_ray = mr; cams = c2; obs = o2; o3 = a2; bytes = b2;
    }
    const int max_n = v.nc * max_cam + v.border;  // the order of the group's largest problem
    BaCovWork w;
    w.first = first; w.count = count; w.np = chol_padded_order(max_n);
    w.cam_lo = hs[first].cam_off; w.obs_lo = hs[first].obs_off; w.o3_lo = hs[first].o3_off;
    w.max_waves = (max_ray + 63) / 64 + 1;
    w.pixel_sigma = pixel_sigma; w.annotation_sigma = annotation_sigma;
    (void)cov_layout(v, (size_t)count, (size_t)w.np, cams, obs, o3, (size_t)w.max_waves, l);
    if (const int rc = h.acquire(in.device, bytes)) {  // (the group before gives its workspace back here)
      if (rc == PTZ_ENOMEM) (void)hipGetLastError();
      return rc;
    }
    char* base = h.base;
    auto at = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
    w.A = at(l.A); w.T = at(l.T); w.X = at(l.X); w.Si = at(l.Si);
    w.Linv = at(l.Linv); w.dsc = at(l.dsc); w.camblk = at(l.camblk); w.EY = at(l.EY); w.Dg = at(l.Dg);
    w.sse_part = at(l.sse_part); w.sse = at(l.sse); w.cov = at(l.cov); w.sig = at(l.sig);
    w.tlwblk = at(l.tlwblk); w.arec = at(l.arec); w.asum = at(l.asum); w.live = reinterpret_cast<int*>(base + l.live); w.var = at(l.var); w.cen = at(l.cen);
    int* ints = reinterpret_cast<int*>(base + l.ints);
    w.n = ints + l.i_n; w.flags = ints + l.i_flags; w.gauge = ints + l.i_gauge; w.n_ann = ints + l.i_n_ann;
    CholBatch cb;
    cb.count = count; cb.np = w.np; cb.A = w.A; cb.Ldiag = at(l.Ldiag); cb.Linv = w.Linv; cb.Dinv = at(l.Dinv); cb.n = w.n; cb.fail = ints + l.i_fail;
    std::vector<int> hg(gauge + first, gauge + first + count);
    PTZ_HIP_TRY(hipMemsetAsync(ints, 0, sizeof(int) * l.n_ints, st));
    PTZ_HIP_TRY(hipMemcpyAsync(ints + l.i_gauge, hg.data(), sizeof(int) * count, hipMemcpyHostToDevice, st));
    PTZ_HIP_TRY(hipMemsetAsync(w.T, 0, sizeof(double) * (size_t)count * w.np * w.np, st));
    PTZ_HIP_TRY(hipEventRecord(h.ev[0], st));
    v.enqueue(in, geo, w, cb, at(l.x), max_cam, max_ray, max_n, st);
    PTZ_HIP_TRY(hipEventRecord(h.ev[1], st));
    // the group's results come back into buffers of their own: only problems whose status is OK reach the caller's arrays
    std::vector<double> hc(cams * NE), hsig((size_t)v.n_sig * count), hcen(v.centre ? 9 * (size_t)count : 0);
    std::vector<int> hi(l.n_ints);
    PTZ_HIP_TRY(hipMemcpyAsync(hc.data(), w.cov, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(hsig.data(), w.sig, sizeof(double) * hsig.size(), hipMemcpyDeviceToHost, st));
    if (v.centre) PTZ_HIP_TRY(hipMemcpyAsync(hcen.data(), w.cen, sizeof(double) * hcen.size(), hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(hi.data(), ints, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(stream_wait(st));
    PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a result
    total_ms += h.elapsed_ms();
    for (int k = 0; k < count; ++k) {
      const BaCovScene& s = hs[first + k];
      const int fail = hi[l.i_fail + k], flags = hi[l.i_flags + k], n_ann = v.centre ? hi[l.i_n_ann + k] : 0;
      if (fail & 2) return PTZ_ENODEVICE;  // (a hand-over of the one-launch factorisation: not a path this call takes)
      const int stt = v.status(v.nf, s, n_ann, fail & 1, flags);
      status[first + k] = stt;
      if (stt != kBaCovOk) continue;
      memcpy(cov + (size_t)s.cam_off * NE, hc.data() + (size_t)(s.cam_off - w.cam_lo) * NE, sizeof(double) * NE * s.n_cam);
      if (v.centre) memcpy(cov_centre + 9 * (size_t)(first + k), hcen.data() + 9 * (size_t)k, sizeof(double) * 9);
      memcpy(sigma0 + (size_t)v.n_sig * (first + k), hsig.data() + (size_t)v.n_sig * k, sizeof(double) * v.n_sig);
    }
    first += count;
  }
  if (device_ms) *device_ms = total_ms;
  return PTZ_OK;
}

}  // namespace

int ba_cov_run(const BaCovIn& in, const BaCovScene* hs, const int* gauge, double pixel_sigma, hipStream_t st, double* cov, double* sigma0,
               int* status, double* device_ms)
{
  if (ba_cov_dim(in.type) < 0) return PTZ_EUNSUPPORTED;
  const CovVariant& v = in.type == 0 ? kVariant<0, false> : in.type == 1 ? kVariant<1, false> : kVariant<2, false>;
  return cov_run(v, in, BaGeoIn{}, hs, gauge, pixel_sigma, 0.0, st, cov, nullptr, sigma0, status, device_ms);
}

int ba_geo_cov_run(const BaCovIn& in, const BaGeoIn& geo, const BaCovScene* hs, const int* gauge, double pixel_sigma, double annotation_sigma,
                   hipStream_t st, double* cov, double* cov_centre, double* sigma0, int* status, double* device_ms)
{
  if (ba_geo_cov_dim(in.type) < 0) return PTZ_EUNSUPPORTED;
  return cov_run(in.type == 0 ? kVariant<0, true> : kVariant<1, true>, in, geo, hs, gauge, pixel_sigma, annotation_sigma, st, cov, cov_centre, sigma0,
                 status, device_ms);
}

}  // namespace ptz
