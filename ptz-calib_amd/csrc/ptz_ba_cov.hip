// ptz_ba_cov.hip -- per-view covariance of bundle-adjusted cameras on MI355X (gfx950).  Definition: ptz_ba_cov.h.
//
// Per group of problems (as many as fit the workspace budget, PTZ_BA_COV_MAX_MB), on the batch's stream:
//   cam        camera blocks (R, intrinsics, Jl) at the state                                           [thread / camera]
//   ray        P_r per ray; E_o, Y_o, the diagonal term and |e_o|^2 per observation; the squared residuals
//              are summed per wave of 64 rays by the butterfly, the waves of a problem in wave order      [thread / ray]
//   assemble   block row ci of S and T: the diagonal block over the camera's observation list, block (ci, cj)
//              over the pair's entry list, both in stored order, one lane per element -- no atomics        [workgroup / camera]
//   scale      gauge rows / columns, unit diagonal                                                        [workgroup / row]
//   cholesky   chol_factor_solve (dense path, right-hand side zero): L in the strictly-lower tiles, the
//              inverses of the factored diagonal tiles in Linv
//   tri_inv    X = L^-1 by 64 x 64 tiles: X_jj = Linv_jj, X_ij = -Linv_ii sum_{k = j}^{i-1} L_ik X_kj     [workgroup / block column]
//   gemm       S^-1 = X^T X, then G = S^-1 T, on v_mfma_f64_16x16x4_f64                                    [workgroup / tile]
//   finish     diagonal blocks of G S^-1 (O(n^2 NF)), unscaling, left-perturbation form, s^2               [wave / camera]
// Every sum has one order that depends on the problem alone (a tile's k loop runs over the problem's own tiles, not the
// group's padded order), so a problem's bits do not depend on its position in the batch, on the grouping or on the run.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_ba_cov.h"

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
};

__global__ void k_ba_cov_cam(BaCovIn in, BaCovWork w, int nf)
{
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[w.first + g];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) w.n[g] = nf * s.n_cam;
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
    const int el = k >= l ? k * NF + l : l * NF + k;  // (the lower triangle's element for both halves: symmetric bit for bit)
    double sS = 0, sT = 0;
    for (int q = 0; q < no; ++q) {
      const double* dg = w.Dg + (size_t)(in.cam_obs[o0 + q] - w.obs_lo) * (NE + 1);
      const double v = dg[el];
      sS += v;
      sT += dg[NE] * v;
    }
    A[(size_t)(ci * NF + k) * np + ci * NF + l] = sS;
    T[(size_t)(ci * NF + k) * np + ci * NF + l] = sT;
    if (k == l) {
      const bool anchor_rot = ci == w.gauge[g] && k >= NF - 3;
      const bool ok = anchor_rot || (sS > 0.0 && isfinite(sS));
      if (!ok) atomicOr(&w.flags[g], kBaCovBadDiag);
      w.dsc[(size_t)g * np + ci * NF + k] = (ok && !anchor_rot) ? 1.0 / sqrt(sS) : 1.0;
    }
  }
  // block (ci, cj), cj < ci, over the pair's entries in stored order; the waves take the camera's pairs in turn
  const int* cpair = in.cam_pair + s.cam_off + s.idx;
  const int pr0 = cpair[ci], npr = cpair[ci + 1] - pr0;
  const int* pps = in.pair_ptr + s.pair_off + s.idx + pr0;
  const int* pcj = in.pair_cj + s.pair_off + pr0;
  if (lane >= NE) return;
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
    const size_t r = (size_t)(ci * NF + k), c = (size_t)(cj * NF + l);
    A[r * np + c] = sS; A[c * np + r] = sS;
    T[r * np + c] = sT; T[c * np + r] = sT;
  }
}

// gauge rows / columns (identity in S, zero in T), then both matrices to the unit diagonal of S
__global__ __launch_bounds__(256) void k_ba_cov_scale(BaCovWork w, int nf)
{
  const int g = blockIdx.y, i = blockIdx.x;
  const int n = w.n[g], np = w.np;
  if (i >= n) return;
  const int r0 = w.gauge[g] * nf + nf - 3;
  double* A = w.A + (size_t)g * np * np + (size_t)i * np;
  double* T = w.T + (size_t)g * np * np + (size_t)i * np;
  const double* sc = w.dsc + (size_t)g * np;
  const double si = sc[i];
  const bool gi = i >= r0 && i < r0 + 3;
  for (int j = threadIdx.x; j < n; j += 256) {
    if (gi || (j >= r0 && j < r0 + 3)) { A[j] = i == j ? 1.0 : 0.0; T[j] = 0.0; }
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

template <int TYPE> void enqueue_group(const BaCovIn& in, const BaCovWork& w, const CholBatch& cb, double* x, int max_cam, int max_ray, int max_n, hipStream_t st)
{
  constexpr int NF = BaDims<TYPE>::NC;
  const int nt = w.np / NB;
  hipLaunchKernelGGL(k_ba_cov_cam, dim3((max_cam + 63) / 64, w.count), dim3(64), 0, st, in, w, NF);
  chol_clear(cb, st);  // zero, padding rows, fail flags (reads n)
  hipLaunchKernelGGL(k_ba_cov_ray<TYPE>, dim3((max_ray + 255) / 256, w.count), dim3(256), 0, st, in, w);
  hipLaunchKernelGGL(k_ba_cov_sse, dim3((w.count + 63) / 64), dim3(64), 0, st, in, w);
  hipLaunchKernelGGL(k_ba_cov_assemble<NF>, dim3(max_cam, w.count), dim3(256), 0, st, in, w);
  hipLaunchKernelGGL(k_ba_cov_scale, dim3(max_n, w.count), dim3(256), 0, st, w, NF);
  chol_factor_solve(cb, x, st);
  hipLaunchKernelGGL(k_ba_cov_tri_inv, dim3(nt, w.count), dim3(256), 0, st, w);
  hipLaunchKernelGGL(k_ba_cov_gemm<0>, dim3(nt * nt, w.count), dim3(256), 0, st, w);
  hipLaunchKernelGGL(k_ba_cov_gemm<1>, dim3(nt * nt, w.count), dim3(256), 0, st, w);
  hipLaunchKernelGGL(k_ba_cov_finish<TYPE>, dim3(max_cam, w.count), dim3(64), 0, st, in, w);
}

}  // namespace

int ba_cov_run(const BaCovIn& in, const BaCovScene* hs, const int* gauge, double pixel_sigma, hipStream_t st, double* cov, double* sigma0,
               int* status, double* device_ms)
{
  const int nf = ba_cov_dim(in.type), NE = nf * nf;
  if (nf < 0) return PTZ_EUNSUPPORTED;
  size_t budget = (size_t)2048 << 20;  // of workspace per group of problems
  if (const char* e = getenv("PTZ_BA_COV_MAX_MB")) budget = (size_t)std::max(1ll, atoll(e)) << 20;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  struct Held {
    int dev; void* base = nullptr; hipStream_t st; hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Held()
    {
      (void)stream_wait(st);
      if (base) ptzpool::dev_release(dev, base);
      if (e0) ptzpool::event_release(dev, true, e0);
      if (e1) ptzpool::event_release(dev, true, e1);
    }
  } h;
  h.dev = in.device; h.st = st;
  PTZ_HIP_TRY(ptzpool::event_acquire(h.dev, true, &h.e0));
  PTZ_HIP_TRY(ptzpool::event_acquire(h.dev, true, &h.e1));
  double total_ms = 0;
  // bytes of a group of `count` problems of padded order np over `cams` cameras and `obs` observation slots
  auto group_bytes = [&](size_t count, size_t np, size_t cams, size_t obs, size_t waves, size_t* offs) {
    const size_t nt = np / NB;
    size_t o = 0;
    auto take = [&](int k, size_t bytes) { if (offs) offs[k] = o; o += up(bytes); };
    for (int k = 0; k < 4; ++k) take(k, sizeof(double) * count * np * np);  // A, T, X, Si
    take(4, sizeof(double) * count * nt * NB * NB);                         // Ldiag
    take(5, sizeof(double) * count * nt * NB * NB);                         // Linv
    take(6, sizeof(double) * count * nt * 4 * 16 * 16);                     // Dinv
    take(7, sizeof(double) * count * np);                                   // x
    take(8, sizeof(double) * count * np);                                   // dsc
    take(9, sizeof(double) * cams * CAMBLK);
    take(10, sizeof(double) * obs * 6 * nf);
    take(11, sizeof(double) * obs * (NE + 1));
    take(12, sizeof(double) * count * waves);
    take(13, sizeof(double) * count);                                       // sse
    take(14, sizeof(double) * cams * NE);                                   // cov
    take(15, sizeof(double) * count);                                       // sig
    take(16, sizeof(int) * count * 4);                                      // n, flags, gauge, fail
    return o;
  };
  for (int first = 0; first < in.n_scene;) {
    // the group: problems first .. first + count - 1, as many as the budget holds (one at least)
    int count = 0, max_cam = 0, max_ray = 0, max_n = 0;
    size_t cams = 0, obs = 0, bytes = 0;
    for (int i = first; i < in.n_scene; ++i) {
      const int mc = std::max(max_cam, hs[i].n_cam), mr = std::max(max_ray, hs[i].n_ray);
      const size_t c2 = (size_t)(hs[i].cam_off + hs[i].n_cam - hs[first].cam_off), o2 = (size_t)(hs[i].obs_off + hs[i].n_obs - hs[first].obs_off);
      const size_t b2 = group_bytes((size_t)(i - first + 1), (size_t)chol_padded_order(nf * mc), c2, o2, (size_t)(mr + 63) / 64 + 1, nullptr);
      if (count > 0 && b2 > budget) break;
      count = i - first + 1; max_cam = mc; max_ray = mr; max_n = nf * mc; cams = c2; obs = o2; bytes = b2;
    }
    BaCovWork w;
    w.first = first; w.count = count; w.np = chol_padded_order(max_n);
    w.cam_lo = hs[first].cam_off; w.obs_lo = hs[first].obs_off;
    w.max_waves = (max_ray + 63) / 64 + 1;
    w.pixel_sigma = pixel_sigma;
    size_t offs[17];
    (void)group_bytes((size_t)count, (size_t)w.np, cams, obs, (size_t)w.max_waves, offs);
    if (ptzpool::dev_acquire(h.dev, bytes, &h.base) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
    char* base = static_cast<char*>(h.base);
    auto at = [&](int k) { return reinterpret_cast<double*>(base + offs[k]); };
    w.A = at(0); w.T = at(1); w.X = at(2); w.Si = at(3);
    w.Linv = at(5); w.dsc = at(8); w.camblk = at(9); w.EY = at(10); w.Dg = at(11); w.sse_part = at(12); w.sse = at(13); w.cov = at(14); w.sig = at(15);
    int* ints = reinterpret_cast<int*>(base + offs[16]);
    w.n = ints; w.flags = ints + count; w.gauge = ints + 2 * count;
    CholBatch cb;
    cb.count = count; cb.np = w.np; cb.A = w.A; cb.Ldiag = at(4); cb.Linv = w.Linv; cb.Dinv = at(6); cb.n = w.n; cb.fail = ints + 3 * count;
    std::vector<int> hg(gauge + first, gauge + first + count);
    PTZ_HIP_TRY(hipMemsetAsync(ints, 0, sizeof(int) * 4 * count, st));
    PTZ_HIP_TRY(hipMemcpyAsync(ints + 2 * count, hg.data(), sizeof(int) * count, hipMemcpyHostToDevice, st));
    PTZ_HIP_TRY(hipMemsetAsync(w.T, 0, sizeof(double) * (size_t)count * w.np * w.np, st));
    PTZ_HIP_TRY(hipEventRecord(h.e0, st));
    switch (in.type) {
      case 0: enqueue_group<0>(in, w, cb, at(7), max_cam, max_ray, max_n, st); break;
      case 1: enqueue_group<1>(in, w, cb, at(7), max_cam, max_ray, max_n, st); break;
      default: enqueue_group<2>(in, w, cb, at(7), max_cam, max_ray, max_n, st); break;
    }
    PTZ_HIP_TRY(hipEventRecord(h.e1, st));
    // the group's results come back into buffers of their own: only problems whose status is OK reach the caller's arrays
    std::vector<double> hc(cams * NE), hsig(count);
    std::vector<int> hi(4 * (size_t)count);
    PTZ_HIP_TRY(hipMemcpyAsync(hc.data(), w.cov, sizeof(double) * hc.size(), hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(hsig.data(), w.sig, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(hipMemcpyAsync(hi.data(), ints, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, st));
    PTZ_HIP_TRY(stream_wait(st));
    PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a result
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h.e0, h.e1);
    total_ms += ms;
    for (int k = 0; k < count; ++k) {
      const BaCovScene& s = hs[first + k];
      const int fail = hi[3 * (size_t)count + k], flags = hi[(size_t)count + k];
      if (fail & 2) return PTZ_ENODEVICE;  // (a hand-over of the one-launch factorisation: not a path this call takes)
      const int stt = ba_cov_status(nf, s.n_cam, s.n_ray, s.n_obs, fail & 1, flags);
      status[first + k] = stt;
      if (stt != kBaCovOk) continue;
      memcpy(cov + (size_t)s.cam_off * NE, hc.data() + (size_t)(s.cam_off - w.cam_lo) * NE, sizeof(double) * NE * s.n_cam);
      sigma0[first + k] = hsig[k];
    }
    ptzpool::dev_release(h.dev, h.base);
    h.base = nullptr;
    first += count;
  }
  if (device_ms) *device_ms = total_ms;
  return PTZ_OK;
}

}  // namespace ptz
