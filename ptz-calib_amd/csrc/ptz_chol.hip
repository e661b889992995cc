// ptz_chol.hip -- batched dense Cholesky solve of the reduced camera system (FP64, gfx950).
//
// Replaces, for the PTZ-IBA hot path, the sparse Cholesky that Ceres' SparseSchurComplementSolver
// runs on the Schur complement (linear_solver_type = SPARSE_SCHUR, src/core/ptzray_optimizer.cc:471).
// Any exact factorisation of the damped reduced system yields the same LM step up to round-off; for a
// 360-degree rig the reduced system is ~30 % dense at camera-block level, so it is factored densely.
//
// Layout: right-looking, 64 x 64 tiles, lower triangle, in place in A[count][np][np] (row-major).
//   step k:  chol_diag   : one 4-wave workgroup factors tile (k,k) (left-looking, lane = row, the inner sum
//                          split over the waves) and inverts its four 16x16 diagonal blocks.  L_kk goes to
//                          Ldiag, never back into A.
//            chol_trsm   : one workgroup per off-diagonal tile of block column k: X L_kk^T = A_ik, blocked by
//                          16 columns, v_mfma_f64_16x16x4_f64 with the block inverses.
//            chol_syrk   : one 256-thread workgroup per trailing tile (i >= j > k):
//                          A_ij -= L_ik L_jk^T with v_mfma_f64_16x16x4_f64, operands staged through LDS.
//   The right-hand side rides along as row n of the padded matrix (diagonal = CHOL_BIG), so the forward
//   substitution is done by the same kernels; chol_backsolve finishes with L^T x = y.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "ptz_common.h"

namespace ptz {

namespace {

constexpr int NB = CHOL_NB;
constexpr int LD = NB + 2;  // LDS row stride in doubles: 16-byte aligned rows, conflict-free fragment reads

typedef double d4 __attribute__((ext_vector_type(4)));

// ---- hand-overs INSIDE a launch (chol_chain_kernel): write-through stores, L1-bypassing loads -----------------------------------
// A tile handed from one workgroup to another inside the launch is stored with sc1 stores (write-through: the bytes leave the
// storing XCD's L2 with the store, no release fence / L2 write-back in front of the flag), every storing wave drains its stores
// (s_waitcnt vmcnt(0)) before the flag is raised, and EVERY load of such bytes is an sc1 load (served by the L2, never by this
// compute unit's L1), so the consumer needs no agent-scope acquire (a buffer_inv sc1 and its ~1.7 us) between its poll and its
// loads -- only the compiler must not hoist the loads over the poll (wavefront-scope fence: no instruction).
__device__ __forceinline__ double ld_sc1(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
typedef double d2n __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_sc1_2(double* p, double2 v)  // 16 bytes (the stores are drained by the caller's drain_stores())
{
  const d2n x = {v.x, v.y};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// 1/sqrt(d): hardware seed (v_rsq_f64) + two Newton steps; d <= 0 propagates NaN/inf (flagged by the caller)
__device__ __forceinline__ double rsqrt_nr(double d)
{
  double y = __builtin_amdgcn_rsq(d);
  y = y * (1.5 - 0.5 * d * y * y);
  y = y * (1.5 - 0.5 * d * y * y);
  return y;
}


// coalesced 64x64 tile copy global (row stride ld) -> LDS (row stride LD); nthreads * 16 B per pass
template <int NTHREADS, bool NEGATE>
__device__ __forceinline__ void tile_g2s(const double* __restrict__ g, int ld, double* s)
{
#pragma unroll
  for (int p = 0; p < (NB * NB / 2) / NTHREADS; ++p) {
    const int idx = p * NTHREADS + threadIdx.x;
    const int row = idx >> 5, c2 = (idx & 31) * 2;
    double2 v = *reinterpret_cast<const double2*>(g + (size_t)row * ld + c2);
    if (NEGATE) { v.x = -v.x; v.y = -v.y; }
    *reinterpret_cast<double2*>(s + row * LD + c2) = v;
  }
}
template <int NTHREADS>
__device__ __forceinline__ void tile_s2g(const double* s, double* __restrict__ g, int ld)
{
#pragma unroll
  for (int p = 0; p < (NB * NB / 2) / NTHREADS; ++p) {
    const int idx = p * NTHREADS + threadIdx.x;
    const int row = idx >> 5, c2 = (idx & 31) * 2;
    *reinterpret_cast<double2*>(g + (size_t)row * ld + c2) = *reinterpret_cast<const double2*>(s + row * LD + c2);
  }
}

// ---- clear the tiles of the lower-triangular structure ------------------------------------------------
__global__ __launch_bounds__(256) void chol_clear_tiles_kernel(CholBatch cb)
{
  const int slot = blockIdx.y, sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int ti = blockIdx.x / nt, tj = blockIdx.x % nt;
  if (tj > ti || !cb.tmask[((size_t)sys * nt + ti) * nt + tj]) return;
  double* T = cb.A + (size_t)sys * np * np + (size_t)(ti * NB) * np + tj * NB;
#pragma unroll
  for (int p = 0; p < (NB * NB / 2) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int row = idx >> 5, c2 = (idx & 31) * 2;
    *reinterpret_cast<double2*>(T + (size_t)row * np + c2) = make_double2(0.0, 0.0);
  }
}

// ---- padding: identity rows beyond n, CHOL_BIG at (n, n) --------------------------------------------
__global__ void chol_pad_kernel(CholBatch cb)
{
  const int slot = blockIdx.y, sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = cb.n[sys];
  if (i >= cb.np || i < n) return;
  cb.A[(size_t)sys * cb.np * cb.np + (size_t)i * cb.np + i] = (i == n) ? CHOL_BIG : 1.0;
  if (i == n) cb.fail[sys] = 0;
}

// ---- diag: Cholesky of the diagonal tile by one 4-wave workgroup ----------------------------------------
// Blocked inside the tile, 16 columns at a time, so that the sequential part never crosses a barrier:
//   1. the 16x16 diagonal block is factored IN REGISTERS by every wave redundantly (same arithmetic -> same bits):
//      lane r holds row r, column steps exchange values with v_readlane, no LDS and no barrier;
//   2. the inverse of that block follows the same way (lane c holds column c of L_bb^-1);
//   3. the rows below are solved on the matrix cores, X = P L_bb^-T = P (L_bb^-1)^T, one 16-row block per wave;
//   4. the trailing 16x16 blocks of the tile get  C -= X_i X_j^T  on the matrix cores.
// Two barriers per 16 columns instead of one per column.  Outputs: Ldiag[sys][k] = L_kk (upper part zero) and
// Dinv[sys][k][4][16x16], the inverses of its diagonal blocks for the MFMA triangular solve of chol_trsm.
constexpr int DB = 16;              // diagonal sub-block order
constexpr int LDD = DB + 2;         // LDS row stride of a 16x16 block

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Factor the tile held in As (row-major, stride LD, fully loaded and synchronised by the caller; 256 threads).
// Writes Ldiag[sys][k], Dinv[sys][k][*] and raises cb.fail[sys] on a non-positive pivot.
//
// The factorisation of a 64 x 64 tile is a chain of 64 pivots; what bounds it is the instruction stream of one pivot step,
// not arithmetic.  So ONE wave runs the chain and keeps it in registers: lane r holds row 16 b + r of the current 16-column
// block -- the rows of the diagonal block AND every row below it -- and one column sweep
//     d = A[j][j];  L[r][j] = A[r][j] / sqrt(d);  A[r][q] -= L[r][j] L[q][j]   (q = j + 1 .. 15, all lanes at once)
// factors the block and solves the rows below in the same instructions (the scalars L[q][j] come from lane q by
// v_readlane; no LDS, no separate triangular solve).  Measured: 185 cycles per pivot, issue-bound (two v_readlane and one
// FP64 FMA per updated column).  Everything else happens beside the chain: before a sweep the four waves bring its 16
// columns up to date on the matrix cores (one 16-row block each, C -= X X^T over the finished column blocks); during a
// sweep wave 1 inverts the previous 16 x 16 diagonal block (for the MFMA triangular solves of chol_trsm and the
// back-substitution) and wave 2 stores the previous column block of L.  (That is the batch path's form, diag_factor_tile; the
// one-launch kernels' form, diag_factor_tile_w0, is described in front of it.)
// ---- the same sweep with DPP broadcasts (round 5; chol_chain_kernel) ----------------------------------------------------------
// What a pivot of the sweep below pays for is the way a scalar of the pivot column reaches the other lanes: v_readlane into a
// scalar register and from there into the multiply-add -- 30 cycles per dependent step (tools/probes/hip/dep_probe.hip: a dependent
// FP64 multiply-add alone is 6).  v_fmac_f64_dpp row_newbcast broadcasts inside a row of 16 lanes in the multiply-add itself.  So
// every row of 16 lanes carries a REPLICA of the diagonal block's rows (ar: lane r of the row holds block row r) beside its own rows
// of the tile (a: lane 16 g + r holds tile row 16 (b + g) + r): the replicas are factored side by side -- same chain, same
// operations, same bits -- and the own rows take their column updates with the replica's broadcasts.  Same products and sums per
// element as the v_readlane form: the values are bit-identical (tools/probes/hip/sweep16_probe.hip: 171 against 207 cycles per
// pivot for the 64 x 16 column block, 0 of 1040 values differ); twice the multiply-adds, hence only for the kernel whose critical
// path the sweep is on (one rig, a few rigs) and which has the registers for it.
#define PTZ_DPP_BC(dst, src, q) asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:" #q " row_mask:0xf bank_mask:0xf" : "=v"(dst) : "v"(src))
#define PTZ_DPP_FD(acc, bsrc, m, q) asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #q " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(bsrc), "v"(m))
template <int Q> __device__ __forceinline__ void dpp_fd(double& acc, const double& l, const double& ml)
{
  if constexpr (Q == 1) PTZ_DPP_FD(acc, l, ml, 1); else if constexpr (Q == 2) PTZ_DPP_FD(acc, l, ml, 2); else if constexpr (Q == 3) PTZ_DPP_FD(acc, l, ml, 3);
  else if constexpr (Q == 4) PTZ_DPP_FD(acc, l, ml, 4); else if constexpr (Q == 5) PTZ_DPP_FD(acc, l, ml, 5); else if constexpr (Q == 6) PTZ_DPP_FD(acc, l, ml, 6);
  else if constexpr (Q == 7) PTZ_DPP_FD(acc, l, ml, 7); else if constexpr (Q == 8) PTZ_DPP_FD(acc, l, ml, 8); else if constexpr (Q == 9) PTZ_DPP_FD(acc, l, ml, 9);
  else if constexpr (Q == 10) PTZ_DPP_FD(acc, l, ml, 10); else if constexpr (Q == 11) PTZ_DPP_FD(acc, l, ml, 11); else if constexpr (Q == 12) PTZ_DPP_FD(acc, l, ml, 12);
  else if constexpr (Q == 13) PTZ_DPP_FD(acc, l, ml, 13); else if constexpr (Q == 14) PTZ_DPP_FD(acc, l, ml, 14); else PTZ_DPP_FD(acc, l, ml, 15);
}
template <int Q> __device__ __forceinline__ void dpp_bc(double& d, const double& s)
{
  if constexpr (Q == 0) PTZ_DPP_BC(d, s, 0); else if constexpr (Q == 1) PTZ_DPP_BC(d, s, 1); else if constexpr (Q == 2) PTZ_DPP_BC(d, s, 2); else if constexpr (Q == 3) PTZ_DPP_BC(d, s, 3);
  else if constexpr (Q == 4) PTZ_DPP_BC(d, s, 4); else if constexpr (Q == 5) PTZ_DPP_BC(d, s, 5); else if constexpr (Q == 6) PTZ_DPP_BC(d, s, 6); else if constexpr (Q == 7) PTZ_DPP_BC(d, s, 7);
  else if constexpr (Q == 8) PTZ_DPP_BC(d, s, 8); else if constexpr (Q == 9) PTZ_DPP_BC(d, s, 9); else if constexpr (Q == 10) PTZ_DPP_BC(d, s, 10); else if constexpr (Q == 11) PTZ_DPP_BC(d, s, 11);
  else if constexpr (Q == 12) PTZ_DPP_BC(d, s, 12); else if constexpr (Q == 13) PTZ_DPP_BC(d, s, 13); else if constexpr (Q == 14) PTZ_DPP_BC(d, s, 14); else PTZ_DPP_BC(d, s, 15);
}
// Round 6: the sweep SOFTWARE-PIPELINED, every instruction of it in inline asm so that the order below IS the issue order.  The sweep is
// bound by instruction issue (tools/probes/hip/issue_probe.hip: 4.75 cycles per FP64 instruction, 19.4 for v_rsq_f64), and the form
// before this one paid the latency of pivot J's chain -- broadcast of the pivot, rsq + two Newton steps, scaling of column J: eleven
// dependent instructions -- on top of it, because the column updates of pivot J - 1 all stood in front of that chain.  Only column J's
// update has to: the updates of the columns behind J are issued BETWEEN the chain's instructions, in its latency shadows, and what
// does not fit behind it.  The negated copies of the column are gone (neg modifier of the DPP multiply-add).  Same operations on the
// same operands in the same order per element: the bits of the form before (tools/probes/hip/sweep16_probe.hip: 0 of 1040 values
// differ, 171 -> 165 cycles per pivot there; in the product 200 -> ...).
//   Hazards kept by hand (the compiler's hazard recogniser does not look inside inline asm): a DPP read of a register needs two
// instructions between it and the VALU write of that register (the broadcast source ar[J] behind its scaling, ar[J + 1] behind its
// last update); the result of v_rsq_f64 is not read by the next instruction.  tests/test_cpu_abi_host.py checks the disassembly.
#define PTZ_A_RSQ(y, d)        asm volatile("v_rsq_f64 %0, %1" : "=v"(y) : "v"(d))
#define PTZ_A_MULH(h, d)       asm volatile("v_mul_f64 %0, %1, 0.5" : "=v"(h) : "v"(d))
#define PTZ_A_MUL(o, a, b)     asm volatile("v_mul_f64 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b))
#define PTZ_A_FNMA(o, y, t, c) asm volatile("v_fma_f64 %0, -%1, %2, %3" : "=v"(o) : "v"(y), "v"(t), "s"(c))
#define PTZ_A_MULIP(x, r)      asm volatile("v_mul_f64 %0, %0, %1" : "+v"(x) : "v"(r))
#define PTZ_DPP_FDN(acc, bsrc, m, q) asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:" #q " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(bsrc), "v"(m))
template <int Q> __device__ __forceinline__ void dpp_fdn(double& acc, const double& l, const double& m)  // acc -= (lane Q of the row's l) * m
{
  if constexpr (Q == 1) PTZ_DPP_FDN(acc, l, m, 1); else if constexpr (Q == 2) PTZ_DPP_FDN(acc, l, m, 2); else if constexpr (Q == 3) PTZ_DPP_FDN(acc, l, m, 3);
  else if constexpr (Q == 4) PTZ_DPP_FDN(acc, l, m, 4); else if constexpr (Q == 5) PTZ_DPP_FDN(acc, l, m, 5); else if constexpr (Q == 6) PTZ_DPP_FDN(acc, l, m, 6);
  else if constexpr (Q == 7) PTZ_DPP_FDN(acc, l, m, 7); else if constexpr (Q == 8) PTZ_DPP_FDN(acc, l, m, 8); else if constexpr (Q == 9) PTZ_DPP_FDN(acc, l, m, 9);
  else if constexpr (Q == 10) PTZ_DPP_FDN(acc, l, m, 10); else if constexpr (Q == 11) PTZ_DPP_FDN(acc, l, m, 11); else if constexpr (Q == 12) PTZ_DPP_FDN(acc, l, m, 12);
  else if constexpr (Q == 13) PTZ_DPP_FDN(acc, l, m, 13); else if constexpr (Q == 14) PTZ_DPP_FDN(acc, l, m, 14); else PTZ_DPP_FDN(acc, l, m, 15);
}
// item I of pivot P's update list: column q = P + 1 + I / 2 of the replica's rows (I even) or of the own rows (I odd)
template <int P, int I> __device__ __forceinline__ void dpp_item(double (&ar)[DB], double (&a)[DB])
{
  constexpr int q = P + 1 + I / 2;
  if constexpr (P >= 0 && q < DB) {
    if constexpr ((I & 1) == 0) dpp_fdn<q>(ar[q], ar[P], ar[P]); else dpp_fdn<q>(a[q], ar[P], a[P]);
  }
}
template <int P, int I0, int I1> __device__ __forceinline__ void dpp_fill(double (&ar)[DB], double (&a)[DB])
{
  if constexpr (I0 < I1) { dpp_item<P, I0>(ar, a); dpp_fill<P, I0 + 1, I1>(ar, a); }
}
template <int J> __device__ __forceinline__ void dpp_sweep(double (&ar)[DB], double (&a)[DB], double (&ird)[DB], int live_cols, double& dmin, bool& bad, const double c15 = 1.5)
{
  if constexpr (J < DB) {
    constexpr int P = J - 1;                       // the pivot whose remaining updates fill this one's chain
    constexpr int NP = P >= 0 ? 2 * (DB - 1 - P) : 0;  // its items; 0 and 1 (column J) went out at the end of its own stage
    double d, y, h, t;
    if constexpr (NP > 2) dpp_item<P, 2>(ar, a); else asm volatile("s_nop 0");
    dpp_bc<J>(d, ar[J]);                 // A[j][j] of the (partly eliminated) block, from lane j of every row of lanes
    dpp_fill<P, 3, 4>(ar, a);
    PTZ_A_RSQ(y, d);                     // rsqrt_nr(d), instruction by instruction as the compiler makes it (the other paths' bits)
    PTZ_A_MULH(h, d);
    dpp_fill<P, 4, 6>(ar, a);
    PTZ_A_MUL(t, h, y);
    dpp_fill<P, 6, 7>(ar, a);
    PTZ_A_FNMA(t, y, t, c15);
    dpp_fill<P, 7, 8>(ar, a);
    PTZ_A_MUL(y, y, t);
    dpp_fill<P, 8, 9>(ar, a);
    PTZ_A_MUL(t, h, y);
    dpp_fill<P, 9, 10>(ar, a);
    PTZ_A_FNMA(t, y, t, c15);
    dpp_fill<P, 10, 11>(ar, a);
    PTZ_A_MUL(y, y, t);
    dpp_fill<P, 11, 12>(ar, a);
    PTZ_A_MULIP(ar[J], y);               // replica lane j: sqrt(d), below: L[r][j], above: 0
    PTZ_A_MULIP(a[J], y);                // own rows likewise
    if constexpr (NP > 12) dpp_fill<P, 12, NP>(ar, a); else asm volatile("s_nop 0");
    dpp_fill<J, 0, 2>(ar, a);            // column J + 1 is final
    ird[J] = y;
    dpp_sweep<J + 1>(ar, a, ird, live_cols, dmin, bad, c15);
  }
  else {
    // A pivot that is not positive (or not a number) leaves a NaN as its 1 / sqrt(d) -- rsq of a negative number or of a NaN is a NaN,
    // of a zero an infinity that the Newton steps turn into one -- and a NaN column of L makes every later pivot of the system a NaN
    // (every row below takes 0 x NaN or worse into its diagonal).  So the sixteen checks of a block are ONE compare of its LAST
    // reciprocal root (was: a compare, a minimum and their masks per pivot, ~150 instructions that the compiler gathered behind the
    // asm block, on the chain; then a sum of sixteen masked roots, ~80).  What the masks left out -- the row of the right-hand side and
    // the padding behind it -- is in now: a NaN there (a non-finite gradient) fails the solve here, where it used to fail the step's
    // finiteness test a kernel later; the LM control takes the same branch (an invalid step) either way.
    bad |= ird[DB - 1] != ird[DB - 1];
    (void)live_cols;
    (void)dmin;
  }
}

// DPP, b > 0: the fourth row of lanes has no rows of the tile left and carries the rows of the IDENTITY instead -- what the sweep
// makes of them is L_bb^-T, lane r holding column r of L_bb^-1: the block's inverse is there when the sweep ends, by the same
// multiply-adds in the same order as diag_block_inverse (bit-identical), and no wave has to compute it afterwards.  It goes to
// dv (LDS, [16][LDD]) and, if dg is given (the last block: nothing else of it is needed by a consumer), to global memory --
// with `flag`, as stores that go through to memory, followed by the flag itself.
#ifdef PTZ_CHOL_TIMELINE
__device__ long long dft_sw[64][8];   // per diagonal tile and block: pivots begin, pivots end
#endif
template <bool DPP = false>
__device__ __forceinline__ void diag_sweep_block(double* As, int b, int kbase, int n, double& dmin, bool& bad, double* dv = nullptr, double* dg = nullptr,
                                                 int* flag = nullptr, int gen = 0)
{
#ifdef PTZ_CHOL_TIMELINE
  long long* flag_dbg_row = (DPP && kbase / NB < 64) ? &dft_sw[kbase / NB][2 * b] : nullptr;
#endif
  const int lane = threadIdx.x & 63;
  const int rows = NB - DB * b;  // rows 16 b .. 63 of the tile live in lanes 0 .. rows - 1
  // The rows of the diagonal block start with a zero upper triangle, so that L[r][j] = A[r][j] / sqrt(d) needs no case
  // distinction (0 for r < j).
  double a[DB], ird[DB];
  {
    const double* src = As + (DB * b + (lane < rows ? lane : 0)) * LD + DB * b;
#pragma unroll
    for (int q = 0; q < DB; q += 2) {
      const double2 v = *reinterpret_cast<const double2*>(src + q);
      a[q] = (!DPP && lane < DB && q > lane) ? 0.0 : v.x;
      a[q + 1] = (!DPP && lane < DB && q + 1 > lane) ? 0.0 : v.y;
    }
  }
  if constexpr (DPP) {
    double ar[DB];
    {
      // (the image's diagonal blocks are zero above the diagonal: the callers of diag_factor_tile_w0 see to it)
      const double* src = As + (DB * b + (lane & (DB - 1))) * LD + DB * b;
#pragma unroll
      for (int q = 0; q < DB; q += 2) {
        const double2 v = *reinterpret_cast<const double2*>(src + q);
        ar[q] = v.x; ar[q + 1] = v.y;
      }
    }
    const bool inv_rows = b > 0 && lane >= 3 * DB;
    if (inv_rows) {
#pragma unroll
      for (int q = 0; q < DB; ++q) a[q] = (q == (lane & (DB - 1))) ? 1.0 : 0.0;
    }
#ifdef PTZ_CHOL_TIMELINE
    if (threadIdx.x == 0 && flag_dbg_row) flag_dbg_row[0] = wall_clock64();
#endif
    dpp_sweep<0>(ar, a, ird, n - (kbase + DB * b), dmin, bad);
#ifdef PTZ_CHOL_TIMELINE
    if (threadIdx.x == 0 && flag_dbg_row) flag_dbg_row[1] = wall_clock64();
#endif
    if (inv_rows) {
      const int r = lane & (DB - 1);
#pragma unroll
      for (int i = 0; i < DB; ++i) dv[i * LDD + r] = a[i];
      if (dg) {
#pragma unroll
        for (int i = 0; i < DB; ++i) {
          if (flag) __hip_atomic_store(&dg[i * DB + r], a[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else dg[i * DB + r] = a[i];
        }
      }
    }
    if (dg && flag) {
      drain_stores();  // vmcnt(0) (inline asm: the compiler's waitcnt pass never drops it)
      if (lane == 0) __hip_atomic_store(flag, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  else {
  // Software-pipelined by hand: the chain d_j -> 1/sqrt(d_j) -> L[:, j] -> A[:, j+1] -> d_{j+1} is issued first in every
  // step, the updates of the columns further right fill its latency.  The scheduling fences keep the compiler from
  // deferring those updates (it otherwise turns the sweep left-looking: a dependent chain of j products in front of
  // every pivot).
  double d = readlane_f64(a[0], 0);
  ird[0] = rsqrt_nr(d);
#pragma unroll
  for (int j = 0; j < DB; ++j) {
    const bool live = (kbase + DB * b + j) < n;
    dmin = fmin(dmin, live ? d : 1.0);  // NaN pivots: fmin keeps the other operand, caught by `bad`
    bad |= (d != d) && live;
    const double l = a[j] * ird[j];   // lane j: d / sqrt(d); lanes below: L[r][j]; lanes above (diagonal block): 0
    a[j] = l;
    if (j + 1 < DB) {
      a[j + 1] -= l * readlane_f64(l, j + 1);
      d = readlane_f64(a[j + 1], j + 1);
      ird[j + 1] = rsqrt_nr(d);
    }
#pragma unroll
    for (int q = j + 2; q < DB; ++q) a[q] -= l * readlane_f64(l, q);  // A[r][q] -= L[r][j] L[q][j]
    __builtin_amdgcn_sched_barrier(0);
  }
  }
  if (lane == 0 && (!DPP || b == 0)) {  // (DPP: only block 0's inverse is still computed from the image)
#pragma unroll
    for (int j = 0; j < DB; ++j) As[(DB * b + j) * LD + NB] = ird[j];  // 1 / L[j][j] in the padding column of the tile image, for the block inverses
  }
  if (lane < rows) {
    double* dst = As + (DB * b + lane) * LD + DB * b;
#pragma unroll
    for (int q = 0; q < DB; q += 2) *reinterpret_cast<double2*>(dst + q) = make_double2(a[q], a[q + 1]);
  }
}

// inverse of the 16 x 16 diagonal block b of the factored tile by forward substitution, one wave, lane c = column c of
// X = L_bb^-1:  X[i][c] = (delta_ic - sum_{m < i} L[i][m] X[m][c]) / L[i][i]   (the L entries are LDS broadcasts)
__device__ __forceinline__ void diag_block_inverse(const double* As, int b, double* out, double* out_lds, bool wt = false)
{
  const int lane = threadIdx.x & 63, fr = lane & 15;
  const double* Lb = As + (DB * b) * LD + DB * b;
  // ONE chain of multiply-adds per element, m ascending: the order in which the DPP sweep (diag_sweep_block<true>) arrives at the
  // same inverse in its spare rows of lanes -- the two must agree in every bit, the paths share their results
  double x[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) {
    double s = (i == fr) ? 1.0 : 0.0;
#pragma unroll
    for (int m = 0; m + 1 < i; m += 2) {
      const double2 lv = *reinterpret_cast<const double2*>(Lb + i * LD + m);
      s = fma(lv.x, -x[m], s);
      s = fma(lv.y, -x[m + 1], s);
    }
    if (i & 1) s = fma(Lb[i * LD + i - 1], -x[i - 1], s);
    x[i] = s * As[(DB * b + i) * LD + NB];
  }
  if (lane < DB) {
#pragma unroll
    for (int i = 0; i < DB; ++i) {
      if (wt) st_sc1(&out[i * DB + fr], x[i]); else out[i * DB + fr] = x[i];
      out_lds[i * LDD + fr] = x[i];
    }
  }
}

// column block b of the factored tile (16 columns, all 64 rows; the rows above the diagonal block are zero) to global, one wave
// wt: the block is handed on inside this launch (chol_chain_kernel) -- write-through stores, see st_sc1_2
__device__ __forceinline__ void diag_store_block(const double* As, int b, double* __restrict__ Lg, bool wt = false)
{
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int idx = p * 64 + lane;           // 64 rows x 8 double2
    const int row = idx >> 3, c2 = (idx & 7) * 2;
    double2 v = make_double2(0.0, 0.0);
    if (row >= DB * b) v = *reinterpret_cast<const double2*>(As + row * LD + DB * b + c2);
    if (wt) st_sc1_2(Lg + (size_t)row * NB + DB * b + c2, v);
    else *reinterpret_cast<double2*>(Lg + (size_t)row * NB + DB * b + c2) = v;
  }
}

// X = L^-1 of a factored 64 x 64 tile from its 16 x 16 block inverses D_i = L_ii^-1:  X_ii = D_i,
//   X_ij = -D_i sum_{m = j}^{i-1} L_im X_mj   (i > j),
// one wave per block column j, everything on the matrix cores and in registers: with v_mfma_f64_16x16x4_f64 the accumulator
// of a product (lane = column, register ks = row 4 ks + lane / 16) already IS the B operand of the next product.
// Ls: tile image in LDS (stride LD); Dis: [4][16][LDD] block inverses in LDS; out: row-major 64 x 64 in global memory.
__device__ __forceinline__ void tile_inverse(const double* Ls, const double* Dis, double* __restrict__ out)
{
  const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  d4 X[NB / DB];  // X_mj, m = j .. 3, as B operands / accumulators
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) X[0][ks] = Dis[j * DB * LDD + (4 * ks + fq) * LDD + fr];
  // block column j of X: zero above the diagonal block, D_j on it, X_ij below
#pragma unroll
  for (int bi = 0; bi < NB / DB; ++bi)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      if (bi <= j) out[(size_t)(DB * bi + 4 * ks + fq) * NB + DB * j + fr] = (bi == j) ? X[0][ks] : 0.0;
#pragma unroll
  for (int i = 1; i < NB / DB; ++i) {
    const int bi = j + i;  // block row
    if (bi < NB / DB) {    // (uniform per wave)
      d4 S = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < i; ++m)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          S = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[(DB * bi + fr) * LD + DB * (j + m) + 4 * ks + fq], X[m][ks], S, 0, 0, 0);
      d4 R = {0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        R = __builtin_amdgcn_mfma_f64_16x16x4f64(-Dis[bi * DB * LDD + fr * LDD + 4 * ks + fq], S[ks], R, 0, 0, 0);
      X[i] = R;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) out[(size_t)(DB * bi + 4 * ks + fq) * NB + DB * j + fr] = R[ks];
    }
  }
}

#ifdef PTZ_CHOL_TIMELINE  // probe builds: inside the diagonal tiles' factorisation (system 0), per block: update phase done, sweep phase done
__device__ long long dft_tl[64][12];
#define DFT_STAMP(i) do { if (threadIdx.x == 0 && Fk && sys == 0 && k < 64) dft_tl[k][i] = wall_clock64(); } while (0)
#else
#define DFT_STAMP(i) do { } while (0)
#endif
__device__ __forceinline__ void diag_factor_tile(double* As, double (*Dv)[DB * LDD], const CholBatch& cb, int sys, int k, int n)
{
  const int np = cb.np, nt = np / NB;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  double* Lg = cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB);
  double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
  double dmin = 1.0;
  bool bad = false;
#pragma unroll 1
  for (int b = 0; b < NB / DB; ++b) {
    if (b > 0) {
      // bring column block b up to date: wave w takes the 16-row block ri = b + w:  C(ri, b) -= sum_{m < b} X(ri, m) X(b, m)^T
      const int ri = b + w;
      if (ri < NB / DB) {
        double* C = As + (DB * ri) * LD + DB * b;
        d4 acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = C[(fq + 4 * i) * LD + fr];
        for (int m = 0; m < b; ++m) {
          const double* Xi = As + (DB * ri) * LD + DB * m;
          const double* Xj = As + (DB * b) * LD + DB * m;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Xi[fr * LD + 4 * ks + fq], Xj[fr * LD + 4 * ks + fq], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) C[(fq + 4 * i) * LD + fr] = acc[i];
      }
      __syncthreads();
    }
    if (w == 0) diag_sweep_block<false>(As, b, k * NB, n, dmin, bad);
    else if (w == 1 && b > 0) diag_block_inverse(As, b - 1, Dg + (b - 1) * (DB * DB), Dv[b - 1]);
    else if (w == 2 && b > 0) diag_store_block(As, b - 1, Lg);
    __syncthreads();
  }
  if (w == 0 && lane == 0 && (bad || !(dmin > 0.0))) atomicOr(&cb.fail[sys], 1);
  if (w == 1) diag_block_inverse(As, NB / DB - 1, Dg + (NB / DB - 1) * (DB * DB), Dv[NB / DB - 1]);
  else if (w == 2) diag_store_block(As, NB / DB - 1, Lg);
  if (cb.L && cb.Linv && k == nt - 1) {
    // the last diagonal tile has no later launch whose spare workgroup could invert it
    __syncthreads();
    tile_inverse(As, &Dv[0][0], cb.Linv + ((size_t)sys * nt + k) * (NB * NB));
  }
}

// ---- round 6: the diagonal tile of the chain kernels with ONE wave on the chain and no barrier on it ----------------------------------
// With the four waves in lock step (diag_factor_tile's form, also with the DPP sweep), a rank-16 update spread over the four waves stands
// between two sweeps, behind a barrier and in front of another: per 16-column block 0.24 us of loads + 1.1 of pivots + 0.48 of stores
// + 0.56 of update (stamps, NOTES_r06 1c) -- the pivots are less than half of a tile's 9.3 us.  Here wave 0 alone walks the chain: it
// sweeps block b, stores the panel, applies block b's share to column block b + 1 itself (3 - b rank-16 products on ITS matrix core,
// read from and written to LDS by the same wave: LDS operations of one wave complete in order, no barrier), loads and sweeps block b + 1.  Beside it, synchronised through two counters in
// LDS that the chain never waits on while they keep up: wave 2 applies block b's share to the column blocks behind b + 1 (as before),
// wave 3 stores the finished column blocks and the inverses to global memory and raises their flags, wave 1 inverts diagonal block 0.
// The same products in the same order per element as every other path (diag_factor_tile): same bits.
// ctl: three ints in LDS -- [0] the two publishers of block 0, [1] panels stored by wave 0, [2] blocks whose far updates wave 2 has done.
__device__ __forceinline__ void diag_factor_tile_w0(double* As, double (*Dv)[DB * LDD], int* ctl, const CholBatch& cb, int sys, int k, int n,
                                                    int* Fk = nullptr, int gen = 0)
{
  const int np = cb.np, nt = np / NB;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  double* Lg = cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB);
  double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
  if (threadIdx.x == 0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; }
  __syncthreads();
  volatile int* vctl = ctl;
  auto wait_ge = [&](int idx, int v) { while (vctl[idx] < v) __builtin_amdgcn_s_sleep(1); };
  // C(ri, c) -= X(ri, m) X(c, m)^T on the matrix cores, one wave; `diag`: the finished diagonal block goes back with zeros above its diagonal
  auto rank16 = [&](int ri, int c, int m, bool diag) {
    double* C = As + (DB * ri) * LD + DB * c;
    const double* Xi = As + (DB * ri) * LD + DB * m;
    const double* Xj = As + (DB * c) * LD + DB * m;
    d4 acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = C[(fq + 4 * i) * LD + fr];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Xi[fr * LD + 4 * ks + fq], Xj[fr * LD + 4 * ks + fq], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(fq + 4 * i) * LD + fr] = (diag && fr > fq + 4 * i) ? 0.0 : acc[i];
  };
  // block b - 1's share in column block b, all N = 4 - b row blocks at once: every LDS read first (X(b, b - 1) is every product's second
  // operand), the N x 4 MFMAs interleaved over the N accumulators, then the stores -- one LDS latency and N x 4 MFMA issue slots where
  // N calls of rank16 pay N latencies and N dependent chains of four (the same products in the same order per accumulator)
  auto near_update = [&](auto nn, int b) {
    constexpr int N = decltype(nn)::value;
    const double* Xj = As + (DB * b) * LD + DB * (b - 1);
    double xj[4], xi[N][4];
    d4 acc[N];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) xj[ks] = Xj[fr * LD + 4 * ks + fq];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double* Xi = As + (DB * (b + i)) * LD + DB * (b - 1);
      const double* C = As + (DB * (b + i)) * LD + DB * b;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) xi[i][ks] = Xi[fr * LD + 4 * ks + fq];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][q] = C[(fq + 4 * q) * LD + fr];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xi[i][ks], xj[ks], acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double* C = As + (DB * (b + i)) * LD + DB * b;
#pragma unroll
      for (int q = 0; q < 4; ++q) C[(fq + 4 * q) * LD + fr] = (i == 0 && fr > fq + 4 * q) ? 0.0 : acc[i][q];  // (the diagonal block: zeros above its diagonal)
    }
  };
  DFT_STAMP(0);
  if (w == 0) {
    double dmin = 1.0;
    bool bad = false;
#pragma unroll 1
    for (int b = 0; b < NB / DB; ++b) {
      if (b > 0) {
        if (b >= 2) wait_ge(2, b - 1);  // column block b holds the shares of blocks 0 .. b - 2 (wave 2)
        if (b == 1) near_update(std::integral_constant<int, 3>{}, b);
        else if (b == 2) near_update(std::integral_constant<int, 2>{}, b);
        else near_update(std::integral_constant<int, 1>{}, b);
      }
      DFT_STAMP(1 + 2 * b);  // column block b is up to date
      const bool last = b == NB / DB - 1;
      diag_sweep_block<true>(As, b, k * NB, n, dmin, bad, Dv[b], last ? Dg + b * (DB * DB) : nullptr, (last && Fk) ? &Fk[b] : nullptr, gen);
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS stores of the panel (and of the block's inverse) are done
      if (lane == 0) vctl[1] = b + 1;
      DFT_STAMP(2 + 2 * b);
    }
    if (lane == 0 && (bad || !(dmin > 0.0))) atomicOr(&cb.fail[sys], 1);
  }
  else if (w == 2) {
    for (int b = 0; b + 2 < NB / DB; ++b) {  // block b's share in the column blocks behind b + 1
      wait_ge(1, b + 1);
      for (int c = b + 2; c < NB / DB; ++c)
        for (int ri = c; ri < NB / DB; ++ri) rank16(ri, c, b, false);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      if (lane == 0) vctl[2] = b + 1;
    }
  }
  else if (w == 3) {
    for (int b = 0; b < NB / DB; ++b) {  // the finished column blocks (and, behind block 0, their inverses) on their way to global memory
      wait_ge(1, b + 1);
      diag_store_block(As, b, Lg, Fk != nullptr);
      if (b > 0 && b + 1 < NB / DB) {  // (block 0's inverse is wave 1's, the last block's left from the sweeping wave's registers)
        const double* dv = Dv[b];
        double* dg = Dg + b * (DB * DB);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          if (Fk) st_sc1(&dg[(4 * p + fq) * DB + fr], dv[(4 * p + fq) * LDD + fr]);
          else dg[(4 * p + fq) * DB + fr] = dv[(4 * p + fq) * LDD + fr];
        }
      }
      if (Fk && b + 1 < NB / DB) {
        drain_stores();
        if (lane == 0 && (b > 0 || atomicAdd(&ctl[0], 1) == 1)) __hip_atomic_store(&Fk[b], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  else {  // w == 1: the inverse of diagonal block 0 (the sweep leaves the others')
    wait_ge(1, 1);
    diag_block_inverse(As, 0, Dg, Dv[0], Fk != nullptr);
    if (Fk) {
      drain_stores();
      if (lane == 0 && atomicAdd(&ctl[0], 1) == 1) __hip_atomic_store(&Fk[0], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  DFT_STAMP(9);
  if (cb.L && cb.Linv && k == nt - 1) tile_inverse(As, &Dv[0][0], cb.Linv + ((size_t)sys * nt + k) * (NB * NB));  // the last diagonal tile has no later launch whose spare workgroup could invert it
}

// block columns of step `step` of system `sys` (one-launch-per-step path)
__device__ __forceinline__ void chol_step_columns(const CholBatch& cb, int sys, int step, int nt, int (&col)[CHOL_STEP_COLS])
{
#pragma unroll
  for (int c = 0; c < CHOL_STEP_COLS; ++c) col[c] = -1;
  if (step >= nt) return;
  if (!cb.sched) { col[0] = step; return; }
  const int* sp = cb.sched + ((size_t)sys * nt + step) * CHOL_STEP_COLS;
#pragma unroll
  for (int c = 0; c < CHOL_STEP_COLS; ++c) col[c] = sp[c];
}

__global__ __launch_bounds__(256) void chol_diag_kernel(CholBatch cb, int kk)
{
  const int slot = blockIdx.y, sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np;
  const int n = cb.n[sys];
  int k = kk;
  if (kk < 0) {  // the columns of step 0
    int col[CHOL_STEP_COLS];
    chol_step_columns(cb, sys, 0, np / NB, col);
    k = -1;
#pragma unroll
    for (int c = 0; c < CHOL_STEP_COLS; ++c) if ((int)blockIdx.x == c) k = col[c];
    if (k < 0) return;
  }
  if (k * NB > n) return;  // whole block column is padding (identity)
  const double* A = cb.A + (size_t)sys * np * np;
  __shared__ __attribute__((aligned(16))) double As[NB * LD];        // A_kk, overwritten by L_kk block column by block column
  __shared__ __attribute__((aligned(16))) double Dv[4][DB * LDD];    // L_bb^-1 of the current block, one private copy per wave
  tile_g2s<256, false>(A + (size_t)(k * NB) * np + k * NB, np, As);
  __syncthreads();
  diag_factor_tile(As, Dv, cb, sys, k, n);
}

// ---- trsm: X L_kk^T = A_ik for one off-diagonal tile, blocked by 16 columns, on the matrix cores --------
// wave w owns rows [16w, 16w+16) of the tile and walks the four column blocks:
//   X_c = (A_c - sum_{q<c} X_q L_cq^T) Dinv_c^T
// with v_mfma_f64_16x16x4_f64; finished X_q blocks pass from accumulator layout to operand layout through a
// wave-private LDS strip, so the four waves never synchronise after the initial load.
__global__ __launch_bounds__(256, 3) void chol_trsm_kernel(CholBatch cb, const double* __restrict__ Dinv, int k)
{
  int bx, slot;
  if (!xcd_remap(bx, slot, chol_live_rows(cb))) return;
  const int sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int n = cb.n[sys];
  const int ti = k + 1 + bx;
  if (k * NB > n || ti * NB > n) return;  // padding
  if (cb.tmask && !cb.tmask[((size_t)sys * nt + ti) * nt + k]) return;  // structurally zero tile
  double* A = cb.A + (size_t)sys * np * np;
  // LDS: only what the solve reads -- the six 16 x 16 blocks of L_kk below its diagonal blocks (13.8 KB instead of the whole
  // tile's 33.8), the block inverses, and a strip of THREE column blocks per wave (the fourth block is parked in the first one's
  // place, which is dead by then): 48.6 KB instead of 76.8, three workgroups per compute unit instead of two.  Same arithmetic.
  constexpr int NBLK = 6, LDX = 3 * DB + 2;
  __shared__ __attribute__((aligned(16))) double Lb[NBLK * DB * LDD];  // block (c, q), q < c, at c (c - 1) / 2 + q
  __shared__ __attribute__((aligned(16))) double Di[4 * DB * LDD];
  __shared__ __attribute__((aligned(16))) double Xs[4][DB * LDX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  {
    const double* Lg = cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB);
    for (int idx = threadIdx.x; idx < NBLK * DB * DB; idx += 256) {
      const int blk = idx >> 8, r = (idx >> 4) & 15, c = idx & 15;
      const int bc = blk < 1 ? 1 : (blk < 3 ? 2 : 3), bq = blk - bc * (bc - 1) / 2;
      Lb[blk * DB * LDD + r * LDD + c] = Lg[(size_t)(DB * bc + r) * NB + DB * bq + c];
    }
  }
  {
    const double* Dg = Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
    for (int idx = threadIdx.x; idx < 4 * DB * DB; idx += 256) {
      const int b = idx >> 8, r = (idx >> 4) & 15, c = idx & 15;
      Di[b * DB * LDD + r * LDD + c] = Dg[idx];
    }
  }
  double* T = A + (size_t)(ti * NB + 16 * w) * np + k * NB;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = T[(size_t)(fq + 4 * i) * np + 16 * c + fr];
  __syncthreads();
  double* xs = Xs[w];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int slot_c = c < 3 ? c : 0;  // where block c of the strip lives
    // acc[c] -= X_q L_cq^T for the finished blocks q < c
#pragma unroll
    for (int q = 0; q < c; ++q)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double av = -xs[fr * LDX + 16 * q + 4 * ks + fq];
        const double bv = Lb[(c * (c - 1) / 2 + q) * DB * LDD + fr * LDD + 4 * ks + fq];
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[c], 0, 0, 0);
      }
    if (c == 3) __builtin_amdgcn_s_waitcnt(0xc07f);  // the reads of block 0 are done before block 3 takes its place
    // T_c to operand layout, then X_c = T_c Dinv_c^T
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[(fq + 4 * i) * LDX + 16 * slot_c + fr] = acc[c][i];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the strip is private to this wave
    d4 xc = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double av = xs[fr * LDX + 16 * slot_c + 4 * ks + fq];
      const double bv = Di[c * DB * LDD + fr * LDD + 4 * ks + fq];
      xc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, xc, 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (c < 3) xs[(fq + 4 * i) * LDX + 16 * c + fr] = xc[i];  // (block 3 is nobody's operand)
      T[(size_t)(fq + 4 * i) * np + 16 * c + fr] = xc[i];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
}

// ---- trailing update: A_ij -= L_ik L_jk^T on the matrix cores ---------------------------------------
// mode 0: every trailing tile (i >= j > k); mode 1: only block column k+1 (tiles (i, k+1)), the part the next panel
// depends on; mode 2: the rest (j >= k+2).  Modes 1 + 2 together equal mode 0 (one-step look-ahead split).
__global__ __launch_bounds__(256) void chol_syrk_kernel(CholBatch cb, int k, int mode, int fuse_diag)
{
  int bx, slot;
  if (!xcd_remap(bx, slot, chol_live_rows(cb))) return;
  const int sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int n = cb.n[sys];
  // linear index -> (i, j), k < j <= i < nt (row-major over the lower triangle of the trailing block)
  const int m = nt - k - 1;
  int ii, jj;
  if (mode == 1) {
    ii = bx; jj = 0;
  }
  else {
    const int t = bx;
    ii = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
    while (ii * (ii + 1) / 2 > t) --ii;
    jj = t - ii * (ii + 1) / 2;
    if (mode == 2) { ++ii; ++jj; }  // lower triangle of the (m-1) x (m-1) block that starts at tile column k+2
  }
  if (ii >= m) return;
  const int ti = k + 1 + ii, tj = k + 1 + jj;
  if (ti * NB > n) return;  // rows of this tile are beyond the rhs row: nothing to update
  const bool next_diag = fuse_diag && ti == tj && ti == k + 1;  // this workgroup also factors the tile afterwards
  bool do_update = true;
  if (cb.tmask) {
    const unsigned char* tm = cb.tmask + (size_t)sys * nt * nt;
    if (!tm[ti * nt + k] || !tm[tj * nt + k]) {  // L_ik or L_jk is structurally zero
      if (!next_diag) return;
      do_update = false;
    }
  }
  double* A = cb.A + (size_t)sys * np * np;
  __shared__ __attribute__((aligned(16))) double As[NB * LD];
  __shared__ __attribute__((aligned(16))) double Bs[NB * LD];
  if (do_update) {
    tile_g2s<256, true>(A + (size_t)(ti * NB) * np + k * NB, np, As);   // -L_ik
    tile_g2s<256, false>(A + (size_t)(tj * NB) * np + k * NB, np, Bs);  //  L_jk
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  // C fragment (f64 16x16x4): element (row = fq + 4 * i, col = fr) of the 16x16 block, i = 0..3
  double* C = A + (size_t)(ti * NB + 16 * w) * np + tj * NB;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = C[(size_t)(fq + 4 * i) * np + 16 * c + fr];
  __syncthreads();
  const double* ap = As + (16 * w + fr) * LD + fq;
  const double* bp = Bs + fr * LD + fq;
  if (do_update) {
#pragma unroll
    for (int kk = 0; kk < NB / 4; ++kk) {
      const double av = ap[4 * kk];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * c) * LD + 4 * kk], acc[c], 0, 0, 0);
    }
  }
  if (next_diag) {
    // This tile is final after this update and nobody else touches it: factor it right here instead of writing it out
    // and launching the diagonal kernel for step k + 1 (saves a launch and a tile round trip per block column).
    __shared__ __attribute__((aligned(16))) double Dv[4][DB * LDD];
    __syncthreads();  // all waves are done reading the operand tiles
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) As[(16 * w + fq + 4 * i) * LD + 16 * c + fr] = acc[c][i];
    __syncthreads();
    diag_factor_tile(As, Dv, cb, sys, ti, n);
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(size_t)(fq + 4 * i) * np + 16 * c + fr] = acc[c][i];
}

// ---- one launch per step (one block column, or two that do not couple) for a FEW systems: triangular solves folded into
//      the trailing update ----------------------------------------------------------------------------------------------
// Right-looking step k as ONE kernel: the workgroup of trailing tile (i, j), i >= j > k, first turns A_ik and A_jk into
// L_ik = A_ik L_kk^-T and L_jk itself (the same blocked MFMA solve as chol_trsm_kernel, into LDS), then A_ij -= L_ik L_jk^T,
// and the workgroup of tile (k+1, k+1) factors it on the spot.  Every L_ik is solved for by each tile of row / column i --
// redundant arithmetic on compute units that would otherwise idle -- which removes the separate triangular-solve launch
// from the 13-deep dependency chain of a single 800 x 800 system (26 launches -> 13).  With a step schedule
// (CholBatch::sched) a step holds two block columns that do not couple -- the arcs of a dissected ring -- whose updates and
// next diagonal tiles proceed in the same launch (13 -> 9 on that system).  The workgroup of the diagonal tile (i, i) is
// the one that writes L_ik back (the back-substitution reads it).  For batches the left-looking kernels are used.
// this wave's 16 rows of a tile in accumulator layout, asked for ahead of the solve (one vector value: an array would be kept in
// scratch across the barrier in between)
typedef double d16v __attribute__((ext_vector_type(16)));
template <bool SC1 = false>  // SC1: the tile was written by another workgroup of THIS launch (chol_chain_kernel), see ld_sc1
__device__ __forceinline__ d16v trsm_rows_fetch(const double* __restrict__ Tg, int ldg)
{
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  d16v r;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) r[4 * c + i] = SC1 ? ld_sc1(&Tg[(size_t)(fq + 4 * i) * ldg + 16 * c + fr]) : Tg[(size_t)(fq + 4 * i) * ldg + 16 * c + fr];
  return r;
}
__device__ __forceinline__ void trsm_rows_to_lds(const d16v rows, int ldg, const double* Lk, const double* Di, double* xs,
                                                 double* __restrict__ store_to)
{
  // this wave's 16 rows of the tile: X_c = (A_c - sum_{q<c} X_q L_cq^T) Dinv_c^T, c = 0..3; xs = those rows of the LDS image
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = rows[4 * c + i];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int q = 0; q < c; ++q)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const double av = -xs[fr * LD + 16 * q + 4 * ks + fq];
        const double bv = Lk[(16 * c + fr) * LD + 16 * q + 4 * ks + fq];
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[c], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[(fq + 4 * i) * LD + 16 * c + fr] = acc[c][i];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): these rows are private to this wave
    d4 xc = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double av = xs[fr * LD + 16 * c + 4 * ks + fq];
      const double bv = Di[c * DB * LDD + fr * LDD + 4 * ks + fq];
      xc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, xc, 0, 0, 0);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xs[(fq + 4 * i) * LD + 16 * c + fr] = xc[i];
      if (store_to) store_to[(size_t)(fq + 4 * i) * ldg + 16 * c + fr] = xc[i];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
}

// The same solve one 16-column block at a time (chol_chain_kernel takes the blocks of L_kk as its producer publishes them):
//   trsm_block_pre<C>    acc[C] -= sum_{q < C} X_q L_Cq^T        needs the blocks (C, q), q < C, of L_kk and X_0 .. X_{C-1} in xs
//   trsm_block_solve<C>  X_C = acc[C] Dinv_C^T -> xs (and store_to)  needs Dinv_C
// Same operations in the same order as trsm_rows_to_lds.
// SW: block (C, q) of L_kk lies at block position (q, C) of the image -- the SECOND column's blocks of a pair of columns taken side by
// side (chain_tile), which share the image with the first column's: the solve reads the blocks below the diagonal blocks only.
template <int C, bool SW = false>
__device__ __forceinline__ void trsm_block_pre(d4 (&acc)[4], const double* Lk, const double* xs)
{
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int q = 0; q < C; ++q)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const double av = -xs[fr * LD + 16 * q + 4 * ks + fq];
      const double bv = SW ? Lk[(16 * q + fr) * LD + 16 * C + 4 * ks + fq] : Lk[(16 * C + fr) * LD + 16 * q + 4 * ks + fq];
      acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[C], 0, 0, 0);
    }
}
// block column C of a factored diagonal tile as its consumers take it (chol_chain_kernel): the rows below its diagonal block
// (16 (C + 1) .. 63) and the inverse of that diagonal block -- asked for with sc1 loads (chain_fetch), staged in LDS (chain_stash)
struct ChainBlk { double2 l0, l1; double di; };
template <int C>
__device__ __forceinline__ ChainBlk chain_fetch(const double* Lg, const double* Dg)
{
  constexpr int rows = NB - DB * (C + 1), items = rows * (DB / 2);
  ChainBlk r;
  r.l0 = make_double2(0.0, 0.0); r.l1 = r.l0;
  if (items > 0) {
    const int i0 = min((int)threadIdx.x, max(items - 1, 0));
    const double* src = Lg + (size_t)(DB * (C + 1) + i0 / (DB / 2)) * NB + DB * C + (i0 % (DB / 2)) * 2;
    r.l0 = make_double2(ld_sc1(src), ld_sc1(src + 1));
  }
  if (items > 256) {
    const int i1 = min((int)threadIdx.x + 256, max(items - 1, 0));
    const double* src = Lg + (size_t)(DB * (C + 1) + i1 / (DB / 2)) * NB + DB * C + (i1 % (DB / 2)) * 2;
    r.l1 = make_double2(ld_sc1(src), ld_sc1(src + 1));
  }
  r.di = ld_sc1(&Dg[C * (DB * DB) + threadIdx.x]);
  return r;
}
template <int C, bool SW = false>
__device__ __forceinline__ void chain_stash(const ChainBlk& r, double* Lk, double* Di)
{
  constexpr int rows = NB - DB * (C + 1), items = rows * (DB / 2);
  auto at = [&](int i) {  // piece i: row 16 (C + 1) + i / 8 of the tile, columns 16 C + 2 (i % 8) ..
    const int rr = i / (DB / 2), c2 = (i % (DB / 2)) * 2;
    return SW ? Lk + (DB * C + (rr & 15)) * LD + DB * (C + 1 + (rr >> 4)) + c2 : Lk + (DB * (C + 1) + rr) * LD + DB * C + c2;
  };
  if (items > 0 && (int)threadIdx.x < items) *reinterpret_cast<double2*>(at(threadIdx.x)) = r.l0;
  if (items > 256 && (int)threadIdx.x + 256 < items) *reinterpret_cast<double2*>(at(threadIdx.x + 256)) = r.l1;
  Di[C * DB * LDD + (threadIdx.x >> 4) * LDD + (threadIdx.x & 15)] = r.di;
}
template <int C>
__device__ __forceinline__ void trsm_block_solve(const d4 (&acc)[4], int ldg, const double* Di, double* xs, double* __restrict__ store_to)
{
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) xs[(fq + 4 * i) * LD + 16 * C + fr] = acc[C][i];
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): these rows are private to this wave
  d4 xc = {0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const double av = xs[fr * LD + 16 * C + 4 * ks + fq];
    const double bv = Di[C * DB * LDD + fr * LDD + 4 * ks + fq];
    xc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, xc, 0, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xs[(fq + 4 * i) * LD + 16 * C + fr] = xc[i];
    if (store_to) store_to[(size_t)(fq + 4 * i) * ldg + 16 * C + fr] = xc[i];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
}

// two such solves side by side (chain_tile's pairs of columns): the same operations per solve, the two streams interleaved so that
// one's LDS round trips and dependent MFMAs stand in the other's shadow
template <int C>
__device__ __forceinline__ void trsm_block_solve2(const d4 (&acc1)[4], const d4 (&acc2)[4], int ldg, const double* Di1, const double* Di2, double* xs1, double* xs2,
                                                  double* __restrict__ st1, double* __restrict__ st2)
{
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) { xs1[(fq + 4 * i) * LD + 16 * C + fr] = acc1[C][i]; xs2[(fq + 4 * i) * LD + 16 * C + fr] = acc2[C][i]; }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): these rows are private to this wave
  d4 x1 = {0, 0, 0, 0}, x2 = {0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const double a1 = xs1[fr * LD + 16 * C + 4 * ks + fq], b1 = Di1[C * DB * LDD + fr * LDD + 4 * ks + fq];
    const double a2 = xs2[fr * LD + 16 * C + 4 * ks + fq], b2 = Di2[C * DB * LDD + fr * LDD + 4 * ks + fq];
    x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, x1, 0, 0, 0);
    x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, x2, 0, 0, 0);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xs1[(fq + 4 * i) * LD + 16 * C + fr] = x1[i];
    xs2[(fq + 4 * i) * LD + 16 * C + fr] = x2[i];
    if (st1) st1[(size_t)(fq + 4 * i) * ldg + 16 * C + fr] = x1[i];
    if (st2) st2[(size_t)(fq + 4 * i) * ldg + 16 * C + fr] = x2[i];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
}

// kmin: no system factors a block column below it in this step, so only the tiles (ti, tj), ti >= tj > kmin, can have work
__global__ __launch_bounds__(256) void chol_col_step_kernel(CholBatch cb, int step, int kmin)
{
  int bx, slot;
  if (!xcd_remap(bx, slot, chol_live_rows(cb))) return;
  const int sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int n = cb.n[sys];
  int col[CHOL_STEP_COLS], nxt[CHOL_STEP_COLS];
  chol_step_columns(cb, sys, step, nt, col);
  chol_step_columns(cb, sys, step + 1, nt, nxt);
  if (col[0] < 0) return;  // (slot 0 is used whenever the step has a column)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int m = nt - kmin - 1, ntri = m * (m + 1) / 2;
  if (bx >= ntri) {
    // the spare workgroups of the launch: full inverse of the diagonal tile of each column of the step (factored by the
    // previous launch), off the critical chain; the back-substitution multiplies by it instead of solving with it
    int k = -1;
#pragma unroll
    for (int c = 0; c < CHOL_STEP_COLS; ++c) if (bx - ntri == c) k = col[c];
    if (!cb.Linv || k < 0 || k * NB > n) return;
    double* Lk = smem;
    double* Di = smem + 3 * NB * LD;
    tile_g2s<256, false>(cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB), NB, Lk);
    const double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
    for (int idx = threadIdx.x; idx < 4 * DB * DB; idx += 256) Di[(idx >> 8) * DB * LDD + ((idx >> 4) & 15) * LDD + (idx & 15)] = Dg[idx];
    __syncthreads();
    tile_inverse(Lk, Di, cb.Linv + ((size_t)sys * nt + k) * (NB * NB));
    return;
  }
  int ii = (int)((sqrt(8.0 * bx + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= bx) ++ii;
  while (ii * (ii + 1) / 2 > bx) --ii;
  const int ti = kmin + 1 + ii, tj = kmin + 1 + (bx - ii * (ii + 1) / 2);
  if (ti * NB > n) return;  // padding
  bool next_diag = false;
#pragma unroll
  for (int c = 0; c < CHOL_STEP_COLS; ++c) next_diag |= ti == tj && ti == nxt[c];
  const unsigned char* tm = cb.tmask ? cb.tmask + (size_t)sys * nt * nt : nullptr;
  // the columns of the step this tile takes an update from: it lies behind them and L_ik and L_jk are both in the structure
  // (kept in four scalars, not an array: a dynamically indexed local array goes to scratch memory)
  static_assert(CHOL_STEP_COLS == 4, "four update slots below");
  int u0 = -1, u1 = -1, u2 = -1, u3 = -1, nu = 0;
#pragma unroll
  for (int c = 0; c < CHOL_STEP_COLS; ++c) {
    const int k = col[c];
    if (k >= 0 && tj > k && k * NB <= n && (!tm || (tm[ti * nt + k] && tm[tj * nt + k]))) {
      if (nu == 0) u0 = k; else if (nu == 1) u1 = k; else if (nu == 2) u2 = k; else u3 = k;
      ++nu;
    }
  }
  if (nu == 0 && !next_diag) return;
  double* A = cb.A + (size_t)sys * np * np;
  double* Lk = smem;                    // [NB * LD]   L_kk
  double* As = Lk + NB * LD;            // [NB * LD]   L_ik
  double* Bs = As + NB * LD;            // [NB * LD]   L_jk (i != j)
  double* Di = Bs + NB * LD;            // [4 * DB * LDD] inverses of the diagonal blocks of L_kk
  double (*Dv)[DB * LDD] = reinterpret_cast<double (*)[DB * LDD]>(Di + 4 * DB * LDD);  // scratch of the diagonal factorisation
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  double* C = A + (size_t)(ti * NB + 16 * w) * np + tj * NB;
  d4 acc[4];
  const double* Bop = ti == tj ? As : Bs;
  // operand tiles of block column k: L_kk and its block inverses into LDS, then L_ik (and L_jk) by triangular solves
  auto operands = [&](int k) {
    tile_g2s<256, false>(cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB), NB, Lk);
    const double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
    for (int idx = threadIdx.x; idx < 4 * DB * DB; idx += 256) Di[(idx >> 8) * DB * LDD + ((idx >> 4) & 15) * LDD + (idx & 15)] = Dg[idx];
    __syncthreads();
    // (asking for the rows in front of L_kk was measured: +0.2 ms per one-rig solve -- everything of a step starts at once here and
    //  their strided loads queue up in front of the tile every wave waits for; chol_chain_kernel, which waits for L_kk, does it)
    double* Lik = cb.L + (size_t)slot * np * np + (size_t)(ti * NB + 16 * w) * np + k * NB;
    trsm_rows_to_lds(trsm_rows_fetch(A + (size_t)(ti * NB + 16 * w) * np + k * NB, np), np, Lk, Di, As + 16 * w * LD, ti == tj ? Lik : nullptr);
    if (ti != tj) trsm_rows_to_lds(trsm_rows_fetch(A + (size_t)(tj * NB + 16 * w) * np + k * NB, np), np, Lk, Di, Bs + 16 * w * LD, nullptr);
  };
  auto update = [&]() {
    __syncthreads();
    const double* ap = As + (16 * w + fr) * LD + fq;
    const double* bp = Bop + fr * LD + fq;
#pragma unroll
    for (int kk = 0; kk < NB / 4; ++kk) {
      const double av = -ap[4 * kk];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * cc) * LD + 4 * kk], acc[cc], 0, 0, 0);
    }
  };
  // The step's columns in ascending order (a tile behind both -- a separator tile -- takes both updates, always in this
  // order).  The C tile is asked for after the first triangular solve has been issued, so that its sixteen strided loads do
  // not queue up in front of the operand tiles on the critical workgroup.
  if (nu > 0) operands(u0);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = C[(size_t)(fq + 4 * i) * np + 16 * c + fr];
  if (nu > 0) update();
  for (int u = 1; u < nu; ++u) {  // a tile behind several columns of the step (fetching the next L_kk ahead was tried: no gain)
    __syncthreads();  // all waves are done with the operand tiles of the previous column
    operands(u == 1 ? u1 : (u == 2 ? u2 : u3));
    update();
  }
  if (next_diag) {
    __syncthreads();  // all waves are done reading the operand tiles
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) As[(16 * w + fq + 4 * i) * LD + 16 * c + fr] = (c == w && fr > fq + 4 * i) ? 0.0 : acc[c][i];  // (diag_factor_tile_w0: zero above the diagonal)
    __syncthreads();
    diag_factor_tile_w0(As, Dv, reinterpret_cast<int*>(Dv + 4), cb, sys, ti, n);  // (no static LDS: the dynamic base stays 16-byte aligned)
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(size_t)(fq + 4 * i) * np + 16 * c + fr] = acc[c][i];
}

// ---- the whole factorisation of a FEW systems as ONE launch: workgroup = tile, tiles handed on through flags -----------------
// The one-launch-per-step path above pays, per step of the dependent chain, the drain of a launch, the start of the next, its
// prologue and a cold read of L_kk (~9 of the ~23 us of a step).  Here every tile (i, j), i >= j, of every system has ONE
// workgroup for the whole factorisation, left-looking like chol_update_col_h_kernel: it keeps its C tile in the accumulators and
// walks the block columns k < j of its update list in the order of the step schedule; for each it waits until the diagonal tile
// k is factored (flag F[k]) and the tiles (i, k), (j, k) are final (flags T[i][k], T[j][k]), solves for L_ik and L_jk in LDS as
// chol_col_step_kernel does and applies the update.  A diagonal workgroup then factors its tile, publishes L_jj with its block
// inverses and raises F[j] (its full inverse for the back-substitution follows, off the chain); any other stores its tile and
// raises T[i][j].  Same arithmetic per tile in the same order as the other two paths: same bits.
//   Flags hold the GENERATION of the launch that raised them (a counter kept beside them), so nothing is cleared between
// launches -- the kernel is replayed from a hipGraph with frozen arguments.  Workgroups take a TICKET when they start and the
// ticket, not the block index, decides which tile they own: tickets count up through the tiles in column-major order, and a
// tile only ever waits for tiles of earlier columns, i.e. for workgroups that started before it did -- whatever the number of
// workgroups the chip holds at a time, the one with the smallest unfinished ticket can always run.  Waits are bounded: if a
// flag does not come (a device fault elsewhere), the system is marked failed and the workgroup goes on -- never a hang.
constexpr int CHAIN_SPIN_LIMIT = 1 << 21;
// `fail`: the system's failure word.  Once ANY wait of the system has run out (bit 1), every other waiter of that system gives up
// at its next look (every 1024 polls): a lost hand-over costs one bound, not one bound per tile behind it.
__device__ __forceinline__ bool chain_wait(const int* flag, int gen, int limit, const int* fail = nullptr)  // (one thread polls with an sc1 load; the bytes the flag stands for are read with sc1 loads: see ld_sc1)
{
  for (int it = 0; it < limit; ++it) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) return true;
    if (fail && (it & 1023) == 1023 && (__hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2)) return false;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}
// raise a flag behind this workgroup's global stores, which were all write-through (st_sc1): every wave waits until its own are
// acknowledged, the barrier collects the waves, one lane stores the flag (no L2 write-back: round 6, was __threadfence())
__device__ __forceinline__ void chain_post(int* flag, int gen)
{
  drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(flag, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#ifdef PTZ_CHOL_TIMELINE  // probe builds: where every tile of system 0 was when, in the REPLAYED graph (a few stores, no printf in the kernel)
__device__ long long chain_tl[128][36];
#define TL_STAMP(i) do { if (threadIdx.x == 0 && tl_row) tl_row[i] = wall_clock64(); } while (0)
__global__ void chol_chain_tl_print(int nt)
{
  long long t0 = 0x7fffffffffffffffll;
  for (int o = 0; o < nt * (nt + 1) / 2; ++o) if (chain_tl[o][0] > 0 && chain_tl[o][0] < t0) t0 = chain_tl[o][0];
  for (int k = 0; k < nt && k < 64; ++k) {
    const long long* r = dft_tl[k];
    if (r[0] <= 0) continue;
    printf("tl dft tile %2d: in %.2f |", k, (r[0] - t0) / 100.0);
    for (int b = 0; b < 4; ++b) printf(" b%d updated %.2f swept %.2f", b, (r[1 + 2 * b] - t0) / 100.0, (r[2 + 2 * b] - t0) / 100.0);
    printf(" | out %.2f | pivots", (r[9] - t0) / 100.0);
    for (int b = 0; b < 4; ++b) printf(" %.2f-%.2f", (dft_sw[k][2 * b] - t0) / 100.0, (dft_sw[k][2 * b + 1] - t0) / 100.0);
    printf("\n");
  }
  int o = 0;
  for (int tj = 0; tj < nt; ++tj)
    for (int ti = tj; ti < nt; ++ti, ++o) {
      const long long* r = chain_tl[o];
      if (r[0] <= 0) continue;
      printf("tl tile (%2d,%2d) start %7.2f  operands done %7.2f  end %7.2f |", ti, tj, (r[0] - t0) / 100.0, r[1] > 0 ? (r[1] - t0) / 100.0 : -1.0, (r[2] - t0) / 100.0);
      for (int q = 0; q < 12 && r[4 + 2 * q] > 0; ++q) printf(" c%lld %.2f-%.2f", r[3] >> (5 * q) & 31, (r[4 + 2 * q] - t0) / 100.0, (r[5 + 2 * q] - t0) / 100.0);
      if (r[28] > 0) printf(" | last column: flags looked at %.2f (have %lld), blocks reached %.2f %.2f %.2f %.2f", (r[28] - t0) / 100.0, r[35], (r[29] - t0) / 100.0, (r[30] - t0) / 100.0, (r[31] - t0) / 100.0, (r[32] - t0) / 100.0);
      printf("\n");
    }
}
#else
#define TL_STAMP(i) do { } while (0)
#endif

__device__ __forceinline__ void chain_tile(const CholBatch& cb, double* smem, int* wg, short* klist, int ticket, int gen)
{
  short* kstep = klist + 1024;  // step of the schedule each list entry is a column of
  const int np = cb.np, nt = np / NB;
  const int slot = ticket % cb.count;
  int ord = ticket / cb.count;  // the tile's number in column-major order over the lower triangle
  const int sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
#ifdef PTZ_CHOL_TIMELINE
  long long* tl_row = (slot == 0 && ord < 128) ? chain_tl[ord] : nullptr;
  if (threadIdx.x == 0 && tl_row) for (int i = 0; i < 36; ++i) tl_row[i] = 0;
  TL_STAMP(0);
#endif
  const int spin = cb.chain_spin_limit > 0 ? cb.chain_spin_limit : CHAIN_SPIN_LIMIT;
  int tj = 0;
  while (tj < nt && ord >= nt - tj) { ord -= nt - tj; ++tj; }
  if (tj >= nt) {  // a ticket beyond the launch's tiles: the counters were left dirty by a launch that did not finish (the host
    if (threadIdx.x == 0) atomicOr(&cb.fail[sys], 2);  // resets them before a solve, k_ctl_reset); never walk off the triangle
    return;
  }
  const int ti = tj + ord;
  const int n = cb.n[sys];
  if (ti * NB > n || tj * NB > n) return;  // padding
  const unsigned char* tm = cb.tmask ? cb.tmask + (size_t)sys * nt * nt : nullptr;
  if (tm && !tm[ti * nt + tj]) return;
  int* F = cb.chain_ctl + 4 + (size_t)slot * (4 * nt + nt * nt);  // F[4 k + b]: block b of diagonal tile k factored and published
  int* T = F + 4 * nt;                                            // T[i * nt + k]: tile (i, k) final in A
  if (threadIdx.x < 64) {  // the update list, as chol_update_col_h_kernel makes it (schedule order)
    const int nq = cb.sched ? CHOL_STEP_COLS * cb.n_steps : tj;
    const int* sq = cb.sched ? cb.sched + (size_t)sys * nt * CHOL_STEP_COLS : nullptr;
    int cnt = 0;
    for (int q0 = 0; q0 < nq; q0 += 64) {
      const int qq = q0 + (int)threadIdx.x;
      const int kc = qq < nq ? (sq ? sq[qq] : qq) : -1;
      const bool in = kc >= 0 && kc < tj;
      const bool ok = in && (!tm || (tm[ti * nt + (in ? kc : 0)] && tm[tj * nt + (in ? kc : 0)]));
      const unsigned long long m = __ballot(ok);
      const int pos = cnt + __popcll(m & ((1ull << threadIdx.x) - 1ull));
      if (ok && pos < 1024) { klist[pos] = (short)kc; kstep[pos] = (short)(sq ? qq / CHOL_STEP_COLS : qq); }
      cnt += __popcll(m);
    }
    if (threadIdx.x == 0) wg[2] = min(cnt, 1024);
  }
  __syncthreads();
  const int Q = wg[2];
  if (ti != tj && Q == 0) {  // final as assembled
    if (threadIdx.x == 0) __hip_atomic_store(&T[ti * nt + tj], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (nothing of this launch to publish)
    return;
  }
  double* A = cb.A + (size_t)sys * np * np;
  double* Lk = smem;                    // [NB * LD]   L_kk
  double* As = Lk + NB * LD;            // [NB * LD]   L_ik
  double* Bs = As + NB * LD;            // [NB * LD]   L_jk (i != j)
  double* Di = Bs + NB * LD;            // [4 * DB * LDD] inverses of the diagonal blocks of L_kk
  double (*Dv)[DB * LDD] = reinterpret_cast<double (*)[DB * LDD]>(Di + 4 * DB * LDD);  // scratch of the diagonal factorisation
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  double* C = A + (size_t)(ti * NB + 16 * w) * np + tj * NB;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = C[(size_t)(fq + 4 * i) * np + 16 * c + fr];
  const double* Bop = ti == tj ? As : Bs;
  // TWO columns of a diagonal tile's list side by side (round 6), when their producers are columns of ONE step of the schedule --
  // the two halves of a dissected arc, the two arcs in front of the separator: they end together, and taken one after the other
  // the second costs a finished column's ~6 us behind the first on the chain.  Side by side: both columns' blocks are taken as
  // they come, round by round; the first column's rows are solved for and applied as always (As), the second column's are only
  // SOLVED for (into Bs, which a diagonal tile does not otherwise use; its L blocks share the image Lk -- the block positions
  // above the diagonal, trsm_block_pre<.., true> -- and its block inverses lie in Dv, which is idle until the tile is factored),
  // and its 64 update MFMAs follow the first column's last round.  Every accumulator takes the same products in the same order
  // as one column after the other: same bits.
  const bool pairs_on = ti == tj && cb.sched;
  for (int q = 0; q < Q; ++q) {
    const int k = klist[q];
    const bool pair = pairs_on && q + 1 < Q && kstep[q] == kstep[q + 1];
    if (q > 0) __syncthreads();  // all waves are done with the operand tiles of the previous column
    if (threadIdx.x == 0) {
      bool ok = chain_wait(&T[ti * nt + k], gen, spin, &cb.fail[sys]) && (ti == tj || chain_wait(&T[tj * nt + k], gen, spin, &cb.fail[sys]));
      if (pair) ok = ok && chain_wait(&T[ti * nt + klist[q + 1]], gen, spin, &cb.fail[sys]);
      if (!ok) atomicOr(&cb.fail[sys], 2);  // bit 1: a hand-over that did not come (reported to the host: LmState::chain_timeouts)
      // is the whole column there already?  ONE thread decides for the workgroup (the waves' own looks below may differ by a flag)
      int all = !pair;
      for (int c = 0; c < 4; ++c) all &= __hip_atomic_load(&F[4 * k + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen;
      wg[3] = all;
    }
    __syncthreads();
    const bool whole = wg[3] != 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (every load of handed-over bytes below is an sc1 load: no invalidate needed, see ld_sc1)
#ifdef PTZ_CHOL_TIMELINE
    if (q < 12) { TL_STAMP(4 + 2 * q); if (threadIdx.x == 0 && tl_row) tl_row[3] |= (long long)(k & 31) << (5 * q); }
#endif
    // the rows to be solved for are on their way while the workgroup waits for L_kk
    const d16v rik = trsm_rows_fetch<true>(A + (size_t)(ti * NB + 16 * w) * np + k * NB, np);
    d16v rjk = rik;
    if (ti != tj) rjk = trsm_rows_fetch<true>(A + (size_t)(tj * NB + 16 * w) * np + k * NB, np);
    // L_kk comes in four 16-column blocks, each with its flag (diag_factor_tile raises them as the blocks reach global memory):
    // block c is staged, X_c = (A_c - sum_{q<c} X_q L_cq^T) Dinv_c^T solved for and its share of the update applied while the
    // producer still works on the blocks behind it -- when the LAST block arrives, all that is left on the chain is its 16 x 16
    // inverse, one product with it and a quarter of the update (was: the whole tile, the whole solve, the whole update).
    const double* Lg = cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB);
    const double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
    double* Lik = cb.L + (size_t)slot * np * np + (size_t)(ti * NB + 16 * w) * np + k * NB;
    d4 xa[4], xb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) { xa[c][i] = rik[4 * c + i]; xb[c][i] = rjk[4 * c + i]; }
    const double* ap = As + (16 * w + fr) * LD + fq;
    const double* bp = Bop + fr * LD + fq;
    if (pair) {
      const int k2 = klist[q + 1];
#ifdef PTZ_CHOL_TIMELINE
      if (q + 1 < 12) { TL_STAMP(4 + 2 * (q + 1)); if (threadIdx.x == 0 && tl_row) tl_row[3] |= (long long)(k2 & 31) << (5 * (q + 1)); }
#endif
      {
        const d16v r2 = trsm_rows_fetch<true>(A + (size_t)(ti * NB + 16 * w) * np + k2 * NB, np);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) xb[c][i] = r2[4 * c + i];
      }
      const double* Lg2 = cb.Ldiag + ((size_t)sys * nt + k2) * (NB * NB);
      const double* Dg2 = cb.Dinv + ((size_t)sys * nt + k2) * 4 * (DB * DB);
      double* Lik2 = cb.L + (size_t)slot * np * np + (size_t)(ti * NB + 16 * w) * np + k2 * NB;
      double* Di2 = &Dv[0][0];
      double* xs1 = As + 16 * w * LD;
      double* xs2 = Bs + 16 * w * LD;
      ChainBlk r1[4], r2[4];
      int p1[4], p2[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        p1[c] = lane == 0 ? __hip_atomic_load(&F[4 * k + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        p2[c] = lane == 0 ? __hip_atomic_load(&F[4 * k2 + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
      }
      int h1 = 0, h2 = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        p1[c] = __builtin_amdgcn_readfirstlane(p1[c]); if (h1 == c && p1[c] == gen) h1 = c + 1;
        p2[c] = __builtin_amdgcn_readfirstlane(p2[c]); if (h2 == c && p2[c] == gen) h2 = c + 1;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (h1 > 0) r1[0] = chain_fetch<0>(Lg, Dg);
      if (h2 > 0) r2[0] = chain_fetch<0>(Lg2, Dg2);
      if (h1 > 1) r1[1] = chain_fetch<1>(Lg, Dg);
      if (h2 > 1) r2[1] = chain_fetch<1>(Lg2, Dg2);
      if (h1 > 2) r1[2] = chain_fetch<2>(Lg, Dg);
      if (h2 > 2) r2[2] = chain_fetch<2>(Lg2, Dg2);
      if (h1 > 3) r1[3] = chain_fetch<3>(Lg, Dg);
      if (h2 > 3) r2[3] = chain_fetch<3>(Lg2, Dg2);
#ifdef PTZ_CHOL_TIMELINE
      if (q + 2 >= Q) { TL_STAMP(28); if (threadIdx.x == 0 && tl_row) tl_row[35] = 10 * h1 + h2; }
#endif
      auto take = [&](auto cc, int kk2, const double* Lgx, const double* Dgx, int (&pp)[4], int hh, ChainBlk (&rr)[4]) {  // block c of one of the two columns: wait, ask
        constexpr int c = decltype(cc)::value;
        if (c >= hh) {  // (uniform)
          if (pp[c] != gen) {
            if (lane == 0 && !chain_wait(&F[4 * kk2 + c], gen, spin, &cb.fail[sys])) atomicOr(&cb.fail[sys], 2);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          rr[c] = chain_fetch<c>(Lgx, Dgx);
          if (c < 3) {
            int nf = lane == 0 ? __hip_atomic_load(&F[4 * kk2 + (c < 3 ? c + 1 : 3)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            pp[c < 3 ? c + 1 : 3] = __builtin_amdgcn_readfirstlane(nf);
          }
        }
      };
      auto pround = [&](auto cc) {
        constexpr int c = decltype(cc)::value;
        trsm_block_pre<c, false>(xa, Lk, xs1);
        trsm_block_pre<c, true>(xb, Lk, xs2);
        take(cc, k, Lg, Dg, p1, h1, r1);
        take(cc, k2, Lg2, Dg2, p2, h2, r2);
#ifdef PTZ_CHOL_TIMELINE
        if (q + 2 >= Q) TL_STAMP(29 + c);
#endif
        chain_stash<c, false>(r1[c], Lk, Di);
        chain_stash<c, true>(r2[c], Lk, Di2);
        __syncthreads();
        trsm_block_solve2<c>(xa, xb, np, Di, Di2, xs1, xs2, Lik, Lik2);
        __syncthreads();  // X_c of every wave, both columns, is in LDS
#pragma unroll
        for (int kk = 4 * c; kk < 4 * c + 4; ++kk) {
          const double av = -ap[4 * kk];
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) acc[q4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * q4) * LD + 4 * kk], acc[q4], 0, 0, 0);
        }
      };
      pround(std::integral_constant<int, 0>{});
      pround(std::integral_constant<int, 1>{});
      pround(std::integral_constant<int, 2>{});
      pround(std::integral_constant<int, 3>{});
#ifdef PTZ_CHOL_TIMELINE
      if (q < 12) TL_STAMP(5 + 2 * q);
#endif
      {  // the second column's update: its X is complete in Bs (the barrier behind the last solve)
        const double* ap2 = Bs + (16 * w + fr) * LD + fq;
        const double* bp2 = Bs + fr * LD + fq;
#pragma unroll
        for (int kk = 0; kk < NB / 4; ++kk) {
          const double av = -ap2[4 * kk];
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) acc[q4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp2[(16 * q4) * LD + 4 * kk], acc[q4], 0, 0, 0);
        }
      }
#ifdef PTZ_CHOL_TIMELINE
      if (q + 1 < 12) TL_STAMP(5 + 2 * (q + 1));
#endif
      ++q;  // both columns are applied
      continue;
    }
    // One look at all four flags first (a look is a memory round trip): the blocks that are there already are asked for at once, so
    // that a column whose producer finished long ago costs two round trips, not eight; only the blocks still to come are waited for
    // one by one -- and while one of those is fetched, the next flag is looked at, so that a consumer on the critical chain keeps
    // up with its producer's sweeps.
    typedef ChainBlk Blk;
    Blk rb[4];
    int pk[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) pk[c] = lane == 0 ? __hip_atomic_load(&F[4 * k + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    int have = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) { pk[c] = __builtin_amdgcn_readfirstlane(pk[c]); if (have == c && pk[c] == gen) have = c + 1; }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef PTZ_CHOL_TIMELINE
    if (q == Q - 1) { TL_STAMP(28); if (threadIdx.x == 0 && tl_row) tl_row[35] = have; }
#endif
    auto fetch = [&](auto cc) { return chain_fetch<decltype(cc)::value>(Lg, Dg); };
    auto stash = [&](auto cc, const Blk& r) { chain_stash<decltype(cc)::value>(r, Lk, Di); };
    if (whole) have = 4;
    if (have > 0) rb[0] = fetch(std::integral_constant<int, 0>{});
    if (have > 1) rb[1] = fetch(std::integral_constant<int, 1>{});
    if (have > 2) rb[2] = fetch(std::integral_constant<int, 2>{});
    if (have > 3) rb[3] = fetch(std::integral_constant<int, 3>{});
    auto block = [&](auto cc) {
      constexpr int c = decltype(cc)::value;
      // what needs only the earlier blocks, in front of the wait
      trsm_block_pre<c>(xa, Lk, As + 16 * w * LD);
      if (ti != tj) trsm_block_pre<c>(xb, Lk, Bs + 16 * w * LD);
      if (c >= have) {  // (uniform)
        if (pk[c] != gen) {  // (the look taken while the previous block was fetched did not find it yet)
          if (lane == 0 && !chain_wait(&F[4 * k + c], gen, spin, &cb.fail[sys])) atomicOr(&cb.fail[sys], 2);  // (every wave polls: no barrier to pass the news on)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        rb[c] = fetch(cc);
        if (c < 3) {  // a look at the next flag rides with this block's fetch
          int nf = lane == 0 ? __hip_atomic_load(&F[4 * k + (c < 3 ? c + 1 : 3)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
          pk[c < 3 ? c + 1 : 3] = __builtin_amdgcn_readfirstlane(nf);
        }
      }
#ifdef PTZ_CHOL_TIMELINE
      if (q == Q - 1) TL_STAMP(29 + c);  // block c: pre done, its flag seen, its fetch issued
#endif
      stash(cc, rb[c]);
      __syncthreads();
      if (ti != tj) trsm_block_solve2<c>(xa, xb, np, Di, Di, As + 16 * w * LD, Bs + 16 * w * LD, nullptr, nullptr);
      else trsm_block_solve<c>(xa, np, Di, As + 16 * w * LD, Lik);
      __syncthreads();  // X_c of every wave is in LDS
#pragma unroll
      for (int kk = 4 * c; kk < 4 * c + 4; ++kk) {
        const double av = -ap[4 * kk];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) acc[q4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * q4) * LD + 4 * kk], acc[q4], 0, 0, 0);
      }
    };
    if (whole) {
      // A column whose producer finished before this workgroup looked (all four flags up, all four blocks asked for above): the whole
      // column at once -- the blocks to LDS together, every wave solves its 16 rows block after block (they are its own: no barrier),
      // ONE barrier, then the 64 update MFMAs.  Same operations on the same operands in the same order per accumulator as the four
      // block rounds (same bits); what it drops is their eight barriers and four dependent LDS hand-overs, which is what a tile with
      // a long list of finished columns -- every tile of the separator's rows -- is paced by (a round: ~1.5 us; its MFMAs: ~0.7).
      stash(std::integral_constant<int, 0>{}, rb[0]); stash(std::integral_constant<int, 1>{}, rb[1]);
      stash(std::integral_constant<int, 2>{}, rb[2]); stash(std::integral_constant<int, 3>{}, rb[3]);
      __syncthreads();
      double* xsa = As + 16 * w * LD;
      double* xsb = Bs + 16 * w * LD;
      if (ti != tj) trsm_block_solve2<0>(xa, xb, np, Di, Di, xsa, xsb, nullptr, nullptr);  // (the two solves of an off-diagonal tile side by side)
      else trsm_block_solve<0>(xa, np, Di, xsa, Lik);
      trsm_block_pre<1>(xa, Lk, xsa); if (ti != tj) trsm_block_pre<1>(xb, Lk, xsb);
      if (ti != tj) trsm_block_solve2<1>(xa, xb, np, Di, Di, xsa, xsb, nullptr, nullptr);  // (the two solves of an off-diagonal tile side by side)
      else trsm_block_solve<1>(xa, np, Di, xsa, Lik);
      trsm_block_pre<2>(xa, Lk, xsa); if (ti != tj) trsm_block_pre<2>(xb, Lk, xsb);
      if (ti != tj) trsm_block_solve2<2>(xa, xb, np, Di, Di, xsa, xsb, nullptr, nullptr);  // (the two solves of an off-diagonal tile side by side)
      else trsm_block_solve<2>(xa, np, Di, xsa, Lik);
      trsm_block_pre<3>(xa, Lk, xsa); if (ti != tj) trsm_block_pre<3>(xb, Lk, xsb);
      if (ti != tj) trsm_block_solve2<3>(xa, xb, np, Di, Di, xsa, xsb, nullptr, nullptr);  // (the two solves of an off-diagonal tile side by side)
      else trsm_block_solve<3>(xa, np, Di, xsa, Lik);
      __syncthreads();  // X of every wave is in LDS
#pragma unroll
      for (int kk = 0; kk < NB / 4; ++kk) {
        const double av = -ap[4 * kk];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) acc[q4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * q4) * LD + 4 * kk], acc[q4], 0, 0, 0);
      }
    }
    else {
    block(std::integral_constant<int, 0>{});
    block(std::integral_constant<int, 1>{});
    block(std::integral_constant<int, 2>{});
    block(std::integral_constant<int, 3>{});
    }
#ifdef PTZ_CHOL_TIMELINE
    if (q < 12) TL_STAMP(5 + 2 * q);
#endif
  }
  TL_STAMP(1);
  if (ti == tj) {
    __syncthreads();  // all waves are done reading the operand tiles
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) As[(16 * w + fq + 4 * i) * LD + 16 * c + fr] = (c == w && fr > fq + 4 * i) ? 0.0 : acc[c][i];  // (diag_factor_tile_w0: zero above the diagonal)
    __syncthreads();
    diag_factor_tile_w0(As, Dv, reinterpret_cast<int*>(Dv + 4), cb, sys, ti, n, &F[4 * ti], gen);  // (the last tile also inverts itself there)
    TL_STAMP(2);
    // (F[4 ti + 3] was raised inside, by the sweeping wave, whose spare lanes hold the last diagonal block's inverse)
    if (cb.Linv && ti != nt - 1) {
      __syncthreads();  // the block inverses of all four blocks are in LDS
      tile_inverse(As, &Dv[0][0], cb.Linv + ((size_t)sys * nt + ti) * (NB * NB));  // off the chain: for the back-substitution
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) st_sc1(&C[(size_t)(fq + 4 * i) * np + 16 * c + fr], acc[c][i]);  // (handed on inside the launch: write-through)
  chain_post(&T[ti * nt + tj], gen);
  TL_STAMP(2);
}

__global__ __launch_bounds__(256) void chol_chain_kernel(CholBatch cb)
{
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nt = cb.np / NB;
  const int total = nt * (nt + 1) / 2 * cb.count;
  int* wg = reinterpret_cast<int*>(smem + 3 * NB * LD + 4 * DB * LDD + 4 * DB * LDD + 2);  // [ticket, generation, list length, -]
  short* klist = reinterpret_cast<short*>(wg + 4);                                          // [1024] + the entries' steps [1024]
  int* ctl = cb.chain_ctl;
  if (threadIdx.x == 0) {
    wg[0] = atomicAdd(&ctl[0], 1);
    wg[1] = __hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  }
  __syncthreads();
  const int ticket = wg[0], gen = wg[1];
  chain_tile(cb, smem, wg, klist, ticket, gen);
  // the last workgroup to finish closes the launch: tickets start at zero again, the generation moves on (nobody reads
  // either any more: every workgroup has taken its ticket and read the generation before it counted itself done)
  if (threadIdx.x == 0) {
    const int d = atomicAdd(&ctl[1], 1);
    if (d == total - 1) {
      __hip_atomic_store(&ctl[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&ctl[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&ctl[2], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- left-looking column update: A_ij -= sum_{k < j} L_ik L_jk^T for the tiles (i, j), i >= j, of block column j -------
// One workgroup per tile: the C tile stays in the accumulators while the loop walks the block columns k < j whose tiles
// L_ik and L_jk are both in the structure, so C is read and written once per column step instead of once per k (the
// right-looking update moves 128 KB per 64^3 update, this one 64 KB), and the whole factorisation needs no trailing
// update launches.  Same arithmetic per (i, j, k) triple as chol_syrk_kernel; the k order is ascending.
// The operand tiles come in HALVES of 32 columns: 35 KB of LDS and two half-tile register sets instead of 68 KB and two whole-tile
// sets, so that three workgroups share a compute unit and the ~8 us of dependent loads in front of a tile's first MFMA overlap other
// tiles' arithmetic (81.5 -> 73.4 ms of column updates per C4 solve).  Same MFMAs per accumulator in the same order: same bits.
constexpr int KH = 32, LDH = KH + 2;
// this thread's pieces of a 64 x 32 half tile (row stride ld) into registers, all loads in flight together (256 threads).  The
// buffer is ONE vector value (not an array): it is carried around the loop back-edge, and hipcc keeps arrays that are in scratch.
typedef double d8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ d8 half_fetch(const double* __restrict__ g, int ld)
{
  d8 r;
#pragma unroll
  for (int p = 0; p < (NB * KH / 2) / 256; ++p) {
    const int idx = p * 256 + threadIdx.x;
    const int row = idx >> 4, c2 = (idx & 15) * 2;
    const double2 v = *reinterpret_cast<const double2*>(g + (size_t)row * ld + c2);
    r[2 * p] = v.x; r[2 * p + 1] = v.y;
  }
  return r;
}
__global__ __launch_bounds__(256, 3) void chol_update_col_h_kernel(CholBatch cb, int j, int fuse_diag)
{
  int bx, slot;
  if (!xcd_remap(bx, slot, chol_live_rows(cb))) return;
  const int sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int n = cb.n[sys];
  const int ti = j + bx;
  if (ti >= nt || ti * NB > n || j * NB > n) return;
  const unsigned char* tm = cb.tmask ? cb.tmask + (size_t)sys * nt * nt : nullptr;
  if (tm && !tm[ti * nt + j]) return;
  double* A = cb.A + (size_t)sys * np * np;
  __shared__ __attribute__((aligned(16))) double Ls[2 * NB * LDH];  // the two half tiles; afterwards (fuse_diag) the whole C tile at stride LD
  static_assert(2 * NB * LDH >= NB * LD, "the diagonal tile is factored in the operand buffers");
  double* As = Ls;
  double* Bs = Ls + NB * LDH;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  double* C = A + (size_t)(ti * NB + 16 * w) * np + j * NB;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = C[(size_t)(fq + 4 * i) * np + 16 * c + fr];
  const double* ap = As + (16 * w + fr) * LDH + fq;
  const double* bp = Bs + fr * LDH + fq;
  // The operand tiles of step k + 1 are fetched into registers while the matrix cores work on step k: a step then costs its 64
  // MFMAs per wave plus one LDS hand-over, not a global-memory round trip on top (the loop used to: barrier, load, barrier, MFMA).
  // The block columns k < j are taken in the order of the step schedule (ascending k without one): a tile then sums its
  // updates in the order the one-launch-per-step path applies them, and a scene has the same bits on either path.
  // The list is made once, in LDS (a system has at most a few hundred block columns).
  __shared__ short klist[1024];
  __shared__ int kcount;
  if (threadIdx.x < 64) {  // wave 0: 64 candidates at a time, all their loads in flight together, compacted in order by ballot
    const int nq = cb.sched ? CHOL_STEP_COLS * cb.n_steps : j;
    const int* sq = cb.sched ? cb.sched + (size_t)sys * nt * CHOL_STEP_COLS : nullptr;
    int cnt = 0;
    for (int q0 = 0; q0 < nq; q0 += 64) {
      const int qq = q0 + (int)threadIdx.x;
      const int kc = qq < nq ? (sq ? sq[qq] : qq) : -1;
      const bool in = kc >= 0 && kc < j;
      const bool ok = in && (!tm || (tm[ti * nt + (in ? kc : 0)] && tm[j * nt + (in ? kc : 0)]));
      const unsigned long long m = __ballot(ok);
      const int pos = cnt + __popcll(m & ((1ull << threadIdx.x) - 1ull));
      if (ok && pos < 1024) klist[pos] = (short)kc;
      cnt += __popcll(m);
    }
    if (threadIdx.x == 0) kcount = min(cnt, 1024);
  }
  __syncthreads();
  const int Q = kcount;
  auto col_of = [&](int q) { return (int)klist[q]; };
  auto next_q = [&](int q) { return q; };
  int q = 0;
  const bool any = q < Q;
  int k = any ? col_of(q) : 0;
  // Two steps of operand tiles are in flight (the tiles were written by other launches, mostly on other XCDs, and come from
  // HBM: one step of 64 MFMAs per wave does not cover that round trip).  The fetches stay unconditional: past the end of the
  // list they re-read the last tiles.
  auto kq = [&](int qq) { return any ? col_of(qq < Q ? qq : Q - 1) : 0; };
  // unit u = half h = u & 1 of the operand tiles of list entry u >> 1
  auto fetch_a = [&](int u) { return half_fetch(A + (size_t)(ti * NB) * np + kq(u >> 1) * NB + KH * (u & 1), np); };
  auto fetch_b = [&](int u) { return half_fetch(A + (size_t)(j * NB) * np + kq(u >> 1) * NB + KH * (u & 1), np); };
  d8 ra = fetch_a(0), rb = fetch_b(0), ra1 = fetch_a(1), rb1 = fetch_b(1);
  (void)k; (void)next_q;
  // one half step: hand the half tiles in (xa, xb) over to LDS, refill the two register sets with unit uf, multiply
  auto step = [&](d8& xa, d8& xb, int uf) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int p = 0; p < (NB * KH / 2) / 256; ++p) {
      const int idx = p * 256 + threadIdx.x;
      const int row = idx >> 4, c2 = (idx & 15) * 2;
      *reinterpret_cast<double2*>(As + row * LDH + c2) = make_double2(-xa[2 * p], -xa[2 * p + 1]);   // -L_ik
      *reinterpret_cast<double2*>(Bs + row * LDH + c2) = make_double2(xb[2 * p], xb[2 * p + 1]);      //  L_jk
    }
    __syncthreads();
    xa = fetch_a(uf);
    xb = fetch_b(uf);
#pragma unroll
    for (int kk = 0; kk < KH / 4; ++kk) {
      const double av = ap[4 * kk];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(16 * c) * LDH + 4 * kk], acc[c], 0, 0, 0);
    }
  };
  for (int u = 0; u < 2 * Q; u += 2) {  // the two register sets take turns: first and second half of a list entry
    step(ra, rb, u + 2);
    step(ra1, rb1, u + 3);
  }
  if (fuse_diag && ti == j) {
    // the diagonal tile of this block column is complete: factor it here, no separate diagonal launch for step j
    __shared__ __attribute__((aligned(16))) double Dv[4][DB * LDD];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) As[(16 * w + fq + 4 * i) * LD + 16 * c + fr] = acc[c][i];
    __syncthreads();
    diag_factor_tile(Ls, Dv, cb, sys, j, n);
    return;
  }
  if (!any) return;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) C[(size_t)(fq + 4 * i) * np + 16 * c + fr] = acc[c][i];
}

// ---- full inverses of the factored diagonal tiles, all at once (the multi-launch paths; the one-launch-per-column path
//      computes them in a spare workgroup of every launch) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void chol_tile_inverse_kernel(CholBatch cb)
{
  const int slot = blockIdx.y, k = blockIdx.x, sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int nt = cb.np / NB;
  if (k * NB > cb.n[sys]) return;
  __shared__ __attribute__((aligned(16))) double Lk[NB * LD];
  __shared__ __attribute__((aligned(16))) double Di[4 * DB * LDD];
  tile_g2s<256, false>(cb.Ldiag + ((size_t)sys * nt + k) * (NB * NB), NB, Lk);
  const double* Dg = cb.Dinv + ((size_t)sys * nt + k) * 4 * (DB * DB);
  for (int idx = threadIdx.x; idx < 4 * DB * DB; idx += 256) Di[(idx >> 8) * DB * LDD + ((idx >> 4) & 15) * LDD + (idx & 15)] = Dg[idx];
  __syncthreads();
  tile_inverse(Lk, Di, cb.Linv + ((size_t)sys * nt + k) * (NB * NB));
}

// ---- back substitution with the inverted diagonal tiles ----------------------------------------------------------------
// L^T x = y by block columns from the last:  x_k = (L_kk^-1)^T t_k;  t_j -= L_kj^T x_k for the tiles (k, j), j < k, of the
// structure.  Both are the same operation -- out[c] (-)= sum_r M[r][c] v[r] over a 64 x 64 tile -- so the kernel runs ONE
// list of work groups (the inverse of tile k alone, then the tiles of row k four at a time): thread = (slot, quarter of the
// rows, column), coalesced 512-byte row reads straight from global memory (each tile is read exactly once), the four
// quarter sums of a column meet in LDS in a fixed order.  The tile data does not depend on the vectors, so the loads of
// the next TWO groups are always in flight while a group is reduced: the kernel streams L at the rate one compute unit
// can pull, instead of paying a cold-miss latency per dependent step.  One workgroup per system: the steps depend on each
// other, and a hand-off between workgroups costs more than a step.
constexpr int BI_THREADS = 512;   // thread = (slot, quarter of the rows, PAIR of columns)
constexpr int BI_RED = 1024;      // partial sums of a group: [slot][quarter][column]

// Two columns per thread with 16-byte loads: the kernel is bound by instruction issue (one compute unit streams the whole factor),
// and a thread per column spent ~185 instructions per 16 multiply-adds.  Every (quarter, column) partial sum is the expression it
// always was, so the bits are unchanged.
__device__ __forceinline__ void bs_load(const BsItem it, const double* Lm, const double* Li, int q, int c2, double2 (&v)[16])
{
  if (it.kind == 0) return;
  const double* col = (it.kind == 1 ? Li : Lm) + it.off + (size_t)(16 * q) * it.ld + c2;
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = *reinterpret_cast<const double2*>(col + (size_t)r * it.ld);
}
// Round 5: the four quarter sums of a column meet INSIDE a wave -- a wave is (quarter = lane / 16) x (16 column pairs), so (s0 + s1)
// is one v_permlane16_swap away and (s0 + s1) + (s2 + s3) one v_permlane32_swap further: the same sums in the same order as the LDS
// meeting place they replace, without its two barriers per group.  What still needs a barrier is the vector t itself: an inverse
// group (kind 1) reads t_k in all its lanes and writes x_k over it (barrier before, between and after), the update groups of a row
// (kind 2) only read x_k and write distinct t_j -- no barrier among them.  C2: 24 barriers per back-substitution instead of 50.
__device__ __forceinline__ void bs_partial(const BsItem it, const double* t, int q, const double2 (&v)[16], double& suma, double& sumb)
{
  double pa = 0, pb = 0;
  if (it.kind != 0) {
    const double* xin = t + it.in_off + 16 * q;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      a0 += v[r].x * xin[r];
      a1 += v[r + 1].x * xin[r + 1];
      a2 += v[r + 2].x * xin[r + 2];
      a3 += v[r + 3].x * xin[r + 3];
      b0 += v[r].y * xin[r];
      b1 += v[r + 1].y * xin[r + 1];
      b2 += v[r + 2].y * xin[r + 2];
      b3 += v[r + 3].y * xin[r + 3];
    }
    pa = (a0 + a1) + (a2 + a3);
    pb = (b0 + b1) + (b2 + b3);
  }
  // quarters q and q ^ 1 (lane distance 16), then the pairs (distance 32): lanes of quarter 0 end with (s0 + s1) + (s2 + s3)
  { double u = pa; swap_rows16(pa, u); pa += u; }
  { double u = pb; swap_rows16(pb, u); pb += u; }
  { double u = pa; swap_halves32(pa, u); pa += u; }
  { double u = pb; swap_halves32(pb, u); pb += u; }
  suma = pa; sumb = pb;
}
__device__ __forceinline__ void bs_store(const BsItem it, double* t, int n, int q, int c2, double suma, double sumb)
{
  if (q == 0 && it.kind != 0) {
    double* out = t + it.out_off + c2;
    if (it.kind == 1) { out[0] = (it.out_off + c2 < n) ? suma : 0.0; out[1] = (it.out_off + c2 + 1 < n) ? sumb : 0.0; }
    else { out[0] -= suma; out[1] -= sumb; }
  }
}
// one group: group_kind = kind of its first item (a group is all inverses or all updates); prev_kind = the group before it (0: none)
__device__ __forceinline__ void bs_apply(const BsItem it, int group_kind, int prev_kind, double* t, int n, int q, int c2, const double2 (&v)[16])
{
  if (group_kind == 1 && prev_kind != 1) __syncthreads();  // the updates of the rows above are in t (behind an inverse group the barrier is already there)
  double suma, sumb;
  bs_partial(it, t, q, v, suma, sumb);
  if (group_kind == 1) __syncthreads();                    // every lane has read t_k before x_k goes over it
  bs_store(it, t, n, q, c2, suma, sumb);
  if (group_kind == 1) __syncthreads();                    // x_k is there for the updates that follow
}

// LIST: the work list is built once in LDS and the loads run two groups ahead.  Systems with so many block columns that the
// list does not fit (more than ~60, i.e. ~1000 views) walk the structure on the fly instead, one group at a time.
template <bool LIST>
__global__ __launch_bounds__(BI_THREADS) void chol_backsolve_kernel(CholBatch cb, double* xout, int max_groups)
{
  const int slot = blockIdx.y, sys = chol_system_of(cb, slot);
  if (sys < 0 || (cb.active && !cb.active[sys])) return;
  const int np = cb.np, nt = np / NB;
  const int n = cb.n[sys];
  const double* Lm = cb.L ? cb.L + (size_t)slot * np * np : cb.A + (size_t)sys * np * np;  // off-diagonal tiles of L
  const double* Li = cb.Linv + (size_t)sys * nt * (NB * NB);
  const unsigned char* tm = cb.tmask ? cb.tmask + (size_t)sys * nt * nt : nullptr;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* t = smem;          // [np] y, overwritten by x
  double* red = t + np;      // [BI_RED]
  BsItem* items = reinterpret_cast<BsItem*>(red + BI_RED);  // LIST: [max_groups][4]
  __shared__ int n_groups;
  // Two workgroups per system (CholBatch::bs_split, chol_backsolve_arcs): this one skips the items the OTHER arc owns -- they become
  // empty slots, whose loads and sums are not made -- and writes the solution of the tiles it owns (the separator's: workgroup 0).
  const int wgi = blockIdx.x;             // 0, or 1 when the launch has two workgroups per system
  __shared__ unsigned char tile_owner[64];
  __shared__ unsigned char group_kind_s[1024];  // kind of a group's first item as the list has it (the barriers of an inverse group are every workgroup's)
  __shared__ int has_owners;
  const int tid = threadIdx.x;
  // wave w: slot w / 2, column half w % 2; lane: quarter of the rows = lane / 16, column pair lane % 16 (c: the first of the two columns)
  const int c = 32 * ((tid >> 6) & 1) + 2 * (tid & 15), q = (tid >> 4) & 3, sl = tid >> 7;
  if (!(LIST && cb.bs_items)) {  // owners come with the host's list only
    if (wgi == 1) return;
    if (tid == 0) has_owners = 0;
  }
  if (LIST && cb.bs_items) {  // the list was made with the structure (chol_backsolve_plan): one coalesced copy instead of wave 0's walk
    const int G = cb.bs_groups[sys];
    const long long* src = reinterpret_cast<const long long*>(cb.bs_items + (size_t)sys * 4 * max_groups);
    long long* dst = reinterpret_cast<long long*>(items);
    static_assert(sizeof(BsItem) == 24, "three 8-byte words per item");
    for (int i = tid; i < 12 * G; i += BI_THREADS) dst[i] = src[i];
    if (tid == 0) n_groups = G;
    if (tid < 64) tile_owner[tid] = 0;
    if (tid == 0) has_owners = 0;
    __syncthreads();
    for (int i = tid; i < 4 * G; i += BI_THREADS) {  // owners out of the kinds: the item keeps its kind if this workgroup takes it
      const int kd = items[i].kind, ow = kd >> 4;
      if (ow) { has_owners = 1; if ((kd & 15) == 1) tile_owner[items[i].out_off / NB] = (unsigned char)ow; }
    }
    __syncthreads();
    if (!has_owners && wgi == 1) return;  // (a system without two arcs in a launch that has them: one workgroup does it all)
    for (int g = tid; g < G && g < 1024; g += BI_THREADS) group_kind_s[g] = (unsigned char)(items[4 * g].kind & 15);
    __syncthreads();
    for (int i = tid; i < 4 * G; i += BI_THREADS) {
      const int kd = items[i].kind, ow = kd >> 4;
      items[i].kind = (ow == 0 || ow == wgi + 1) ? (kd & 15) : 0;
    }
  }
  else if (LIST && tid < 64) {  // the work list, in execution order; made by wave 0, 64 candidate tiles at a time (ballot compaction)
    // Backward over the steps of the factorisation.  The block columns of one step (the two arcs of a dissected system) do not
    // couple, so their diagonal inverses share a group and their rows' tiles fill groups together: the chain of dependent
    // groups is as long as the step schedule, not as the number of block columns.
    int g = 0;
    const int n_steps = cb.sched ? cb.n_steps : nt;
    for (int st = n_steps - 1; st >= 0; --st) {
      int col[CHOL_STEP_COLS];
      chol_step_columns(cb, sys, st, nt, col);
      bool any_col = false;
#pragma unroll
      for (int c = 0; c < CHOL_STEP_COLS; ++c) {  // padding columns drop out (their slot of the group stays empty)
        if (col[c] >= 0 && col[c] * NB >= n) col[c] = -1;
        any_col |= col[c] >= 0;
      }
      if (!any_col) continue;
      static_assert(CHOL_STEP_COLS <= 4, "the diagonal inverses of a step share one group of four items");
      if (tid < 4) {
        const int kd = tid == 0 ? col[0] : (tid == 1 ? col[1] : (tid == 2 ? col[2] : col[3]));
        items[4 * g + tid] = kd >= 0 ? BsItem{(long long)kd * (NB * NB), NB, kd * NB, kd * NB, 1} : BsItem{0, 0, 0, 0, 0};
      }
      ++g;
      int filled = 0;
#pragma unroll
      for (int c = 0; c < CHOL_STEP_COLS; ++c) {
        const int k = col[c];
        if (k < 0) continue;
        for (int t0 = 0; t0 < k; t0 += 64) {
          const int tj = t0 + tid;
          const bool ok = tj < k && (!tm || tm[k * nt + tj]);
          const unsigned long long m = __ballot(ok);
          if (ok) items[4 * g + filled + __popcll(m & ((1ull << tid) - 1ull))] = BsItem{(long long)(k * NB) * np + (long long)tj * NB, np, k * NB, tj * NB, 2};
          filled += __popcll(m);
        }
      }
      const int padded = (filled + 3) & ~3;
      if (tid < padded - filled) items[4 * g + filled + tid] = BsItem{0, 0, 0, 0, 0};
      g += padded / 4;
    }
    if (tid == 0) n_groups = g;
  }
  {
    const int kt = n / NB;
    const double* Ldn = cb.Ldiag + ((size_t)sys * nt + kt) * (NB * NB) + (size_t)(n - kt * NB) * NB;
    for (int j = tid; j < np; j += BI_THREADS) t[j] = (j < n) ? ((j >= kt * NB) ? Ldn[j - kt * NB] : Lm[(size_t)n * np + j]) : 0.0;
  }
  __syncthreads();
  if (LIST) {
    const int G = n_groups;
    double2 r0[16], r1[16], r2[16];
    if (0 < G) bs_load(items[sl], Lm, Li, q, c, r0);
    if (1 < G) bs_load(items[4 + sl], Lm, Li, q, c, r1);
    const bool host_list = cb.bs_items != nullptr;
    auto kind_of = [&](int g) { return g >= 0 && g < G ? (host_list ? (int)group_kind_s[g] : (int)items[4 * g].kind) : 0; };
    for (int g = 0; g < G; g += 3) {
      if (g + 2 < G) bs_load(items[4 * (g + 2) + sl], Lm, Li, q, c, r2);
      bs_apply(items[4 * g + sl], kind_of(g), kind_of(g - 1), t, n, q, c, r0);
      if (g + 1 >= G) break;
      if (g + 3 < G) bs_load(items[4 * (g + 3) + sl], Lm, Li, q, c, r0);
      bs_apply(items[4 * (g + 1) + sl], kind_of(g + 1), kind_of(g), t, n, q, c, r1);
      if (g + 2 >= G) break;
      if (g + 4 < G) bs_load(items[4 * (g + 4) + sl], Lm, Li, q, c, r1);
      bs_apply(items[4 * (g + 2) + sl], kind_of(g + 2), kind_of(g + 1), t, n, q, c, r2);
    }
    __syncthreads();  // the last updates are in t before it is copied out
  }
  else {
    double2 r0[16];
    for (int k = nt - 1; k >= 0; --k) {
      const int c0 = k * NB;
      if (c0 >= n) continue;
      BsItem it = BsItem{(long long)k * (NB * NB), NB, c0, c0, sl == 0 ? 1 : 0};
      bs_load(it, Lm, Li, q, c, r0);
      bs_apply(it, 1, 2, t, n, q, c, r0);
      for (int tj = 0; tj < k;) {  // tiles (k, tj) of the structure, four at a time, in the order the list would hold them
        int mine = -1, ns = 0;
        while (tj < k && ns < 4) {
          if (!tm || tm[k * nt + tj]) { if (ns == sl) mine = tj; ++ns; }
          ++tj;
        }
        if (ns == 0) break;
        it = BsItem{(long long)c0 * np + (long long)(mine < 0 ? 0 : mine) * NB, np, c0, (mine < 0 ? 0 : mine) * NB, mine >= 0 ? 2 : 0};
        bs_load(it, Lm, Li, q, c, r0);
        bs_apply(it, 2, 1, t, n, q, c, r0);
      }
    }
    __syncthreads();
  }
  // (two workgroups: each writes the solution of the tiles it owns; the separator's tiles and the padding are workgroup 0's)
  const bool split = has_owners != 0;
  auto mine = [&](int e) { return !split || (tile_owner[e & 63] == 0 ? wgi == 0 : (int)tile_owner[e & 63] == wgi + 1); };
  if (cb.xperm) {  // in the caller's numbering (CholBatch::xperm)
    const int* xp = cb.xperm + (size_t)sys * nt;
    for (int j = tid; j < np; j += BI_THREADS) {
      const int e = xp[j / NB];
      if (mine(e)) xout[(size_t)sys * np + j] = (j < n) ? t[e * NB + j % NB] : 0.0;
    }
    return;
  }
  for (int j = tid; j < np; j += BI_THREADS)
    if (mine(j / NB)) xout[(size_t)sys * np + j] = (j < n) ? t[j] : 0.0;
}

}  // namespace

void chol_clear(const CholBatch& cb, hipStream_t stream)
{
  if (cb.tmask) {
    // only the tiles of the structure are ever written (by the assembly and by the fill of the factorisation); the rest
    // of A was zeroed once when the batch was created and stays zero
    const int nt = cb.np / NB;
    launch(chol_clear_tiles_kernel, dim3(nt * nt, cb.count), dim3(256), 0, stream, cb);
  }
  else {
    (void)hipMemsetAsync(cb.A, 0, sizeof(double) * (size_t)cb.count * cb.np * cb.np, stream);
  }
  dim3 grid((cb.np + 255) / 256, cb.count);
  launch(chol_pad_kernel, grid, dim3(256), 0, stream, cb);
}

void chol_panel_launch(const CholBatch& cb, int k, hipStream_t stream, bool diag_done)
{
  if (!diag_done) launch(chol_diag_kernel, dim3(1, cb.count), dim3(256), 0, stream, cb, k);
  const int m = cb.np / NB - k - 1;
  if (m > 0) launch(chol_trsm_kernel, dim3(m, cb.count), dim3(256), 0, stream, cb, (const double*)cb.Dinv, k);
}
void chol_syrk_launch(const CholBatch& cb, int k, hipStream_t stream, int mode, bool fuse_diag)
{
  const int m = cb.np / NB - k - 1;
  const int tiles = mode == 0 ? m * (m + 1) / 2 : (mode == 1 ? m : m * (m - 1) / 2);
  if (tiles > 0) launch(chol_syrk_kernel, dim3(tiles, cb.count), dim3(256), 0, stream, cb, k, mode, fuse_diag ? 1 : 0);
}
void chol_update_col_launch(const CholBatch& cb, int j, hipStream_t stream, bool fuse_diag)
{
  const int m = cb.np / NB - j;
  if (j > 0 && m > 0) launch(chol_update_col_h_kernel, dim3(m, cb.count), dim3(256), 0, stream, cb, j, fuse_diag ? 1 : 0);
}
void chol_col_step_launch(const CholBatch& cb, int step, hipStream_t stream)
{
  const int nt = cb.np / NB;
  const size_t smem = sizeof(double) * (3 * NB * LD + 4 * DB * LDD + 4 * DB * LDD + 2);
  {  // > 64 KiB of dynamic LDS: the cap is raised once per device
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute((const void*)chol_col_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      done.fetch_or(bit, std::memory_order_release);
    }
  }
  const int kmin = cb.sched ? cb.sched_kmin[step] : step;
  const int m = nt - kmin - 1;
  if (m > 0) launch(chol_col_step_kernel, dim3(m * (m + 1) / 2 + (cb.Linv ? (cb.sched ? CHOL_STEP_COLS : 1) : 0), cb.count), dim3(256), smem, stream, cb, step, kmin);
}
bool chol_chain_fits(int count, int np)
{
  // PTZ_BA_CHOL_CHAIN=0 brings the one-launch-per-step path back (A/B measurements)
  const char* e = getenv("PTZ_BA_CHOL_CHAIN");
  const bool on = !e || atoi(e) != 0;
  // The workgroups take their tiles in elimination order (ticket = tile ordinal x system), so a tile only ever waits for
  // workgroups that started before it: any number of tiles is SAFE.  What it costs when the tiles are not all on the chip from
  // the start (135 KB of LDS: one workgroup per compute unit; 91 tiles per 800 x 800 system): a tile that starts late applies
  // its whole update list in one go at the end of the chain (measured, 800 x 800: 8 systems 11.6 ms against 10.2 ms with one
  // launch per step, 3 systems 8.66 / 8.55; 1 and 2 systems 7.7 / 8.0 against 8.0 / 8.3; 3-4 rigs of 80-110 views 1-2 % faster
  // with it, 6 of 60 views even: tools/probes/probe_chain_small.py).  Up to eight systems: as many as have all their tiles on
  // the chip at once.  Nine to CHOL_CHAIN_SLOTS systems (the view batches of the incremental pipeline: ~20 growing rigs per lock
  // step, each step of the per-step path a launch that 20 small systems cannot fill): one launch as well, up to a tile count
  // beyond which the per-step kernels' throughput wins.
  const int nt = np / NB;
  const int tiles = count * (nt * (nt + 1) / 2);
  int mid_tiles = 3072;
  if (const char* m = getenv("PTZ_BA_CHOL_CHAIN_TILES")) mid_tiles = atoi(m);
  bool fits = count <= 8 ? tiles <= (count <= 2 ? 256 : 192) : (count <= CHOL_CHAIN_SLOTS && tiles <= mid_tiles);
  if (const char* m = getenv("PTZ_BA_CHOL_CHAIN_MAX")) fits = count <= std::max(1, std::min(CHOL_CHAIN_SLOTS, atoi(m)));
  return on && fits && nt <= 1024;
}
bool chol_chain_enabled(const CholBatch& cb) { return cb.L && cb.Linv && cb.chain_ctl && chol_chain_fits(cb.count, cb.np); }
void chol_chain_launch(const CholBatch& cb, hipStream_t stream)
{
  const int nt = cb.np / NB;
  const size_t smem = sizeof(double) * (3 * NB * LD + 4 * DB * LDD + 4 * DB * LDD + 2) + sizeof(int) * 4 + sizeof(short) * 2048;  // (klist + kstep)
  {  // > 64 KiB of dynamic LDS: the cap is raised once per device
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute((const void*)chol_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      done.fetch_or(bit, std::memory_order_release);
    }
  }
  launch(chol_chain_kernel, dim3(nt * (nt + 1) / 2 * cb.count), dim3(256), smem, stream, cb);
}
#ifdef PTZ_CHOL_TIMELINE
void chol_chain_timeline_print(int nt) { hipLaunchKernelGGL(chol_chain_tl_print, dim3(1), dim3(1), 0, 0, nt); (void)hipDeviceSynchronize(); }
#endif
void chol_diag_launch(const CholBatch& cb, int k, hipStream_t stream)
{
  launch(chol_diag_kernel, dim3(k < 0 && cb.sched ? CHOL_STEP_COLS : 1, cb.count), dim3(256), 0, stream, cb, k);
}
void chol_tile_inverse_launch(const CholBatch& cb, hipStream_t stream)
{
  launch(chol_tile_inverse_kernel, dim3(cb.np / NB, cb.count), dim3(256), 0, stream, cb);
}
void chol_backsolve_launch(const CholBatch& cb, double* x, hipStream_t stream)
{
  const int nt = cb.np / NB;
  const int max_groups = chol_backsolve_max_groups(cb.np);
  (void)nt;
  const size_t base = sizeof(double) * ((size_t)cb.np + BI_RED);
  const size_t list = sizeof(BsItem) * 4 * (size_t)max_groups;
  const bool use_list = base + list <= 150 * 1024;
  {  // large systems: the dynamic LDS goes beyond 64 KiB
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
      auto raise = [](const void* fn) {  // (the statically declared part counts against the same 160 KB)
        hipFuncAttributes fa;
        const int stat = hipFuncGetAttributes(&fa, fn) == hipSuccess ? (int)fa.sharedSizeBytes : 4096;
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - stat);
      };
      raise((const void*)chol_backsolve_kernel<true>);
      raise((const void*)chol_backsolve_kernel<false>);
      done.fetch_or(bit, std::memory_order_release);
    }
  }
  if (use_list) launch(chol_backsolve_kernel<true>, dim3((cb.bs_items && cb.bs_split) ? 2 : 1, cb.count), dim3(BI_THREADS), base + list, stream, cb, x, max_groups);
  else launch(chol_backsolve_kernel<false>, dim3(1, cb.count), dim3(BI_THREADS), base + 64, stream, cb, x, 0);
}

void chol_factor_solve(const CholBatch& cb, double* x, hipStream_t stream)
{
  const int nt = cb.np / NB;
  if (cb.L) {  // a few systems: one launch for the whole factorisation, or one per step of the schedule
    if (chol_chain_enabled(cb)) chol_chain_launch(cb, stream);
    else {
      chol_diag_launch(cb, -1, stream);
      for (int st = 0; st + 1 < chol_step_count(cb); ++st) chol_col_step_launch(cb, st, stream);  // (the last step's column has nothing behind it)
    }
    chol_backsolve_launch(cb, x, stream);
    return;
  }
  // every trailing update also factors the diagonal tile of the next block column (it is final by then)
  for (int k = 0; k < nt; ++k) {
    chol_panel_launch(cb, k, stream, /*diag_done=*/k > 0);
    chol_syrk_launch(cb, k, stream, 0, /*fuse_diag=*/true);
  }
  chol_tile_inverse_launch(cb, stream);
  chol_backsolve_launch(cb, x, stream);
}

}  // namespace ptz

// ---- FP64 MFMA peak micro-benchmark -----------------------------------------------------------------------
// Every wave keeps eight independent 16x16 accumulators busy with v_mfma_f64_16x16x4_f64 (2048 flop each); nothing but
// registers is touched inside the loop.  The result is the rate the reduced-camera solve is priced against.
namespace ptz {
namespace {
__global__ __launch_bounds__(256) void mfma_f64_peak_kernel(double* out, int iters)
{
  d4 acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = d4{0.0, 0.0, 0.0, 0.0};
  double a = 1.0 + 1e-9 * threadIdx.x, bq = 1.0 - 1e-9 * threadIdx.x;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq, acc[k], 0, 0, 0);
  }
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) sum += acc[k][0] + acc[k][1] + acc[k][2] + acc[k][3];
  if (sum == 123.456) out[0] = sum;  // keeps the loop alive; never true
}
}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_mfma_f64_peak(int32_t device_id, double* tflops)
{
  using namespace ptz;
  clear_stale_error(__func__);
  if (!tflops) return PTZ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  hipDeviceProp_t prop;
  PTZ_HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  double* d_out = nullptr;
  PTZ_HIP_TRY(hipMalloc(&d_out, sizeof(double)));
  hipEvent_t e0, e1;
  PTZ_HIP_TRY(hipEventCreate(&e0));
  PTZ_HIP_TRY(hipEventCreate(&e1));
  const int blocks = prop.multiProcessorCount * 8, iters = 20000;
  hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, nullptr, d_out, 100);  // warm-up
  PTZ_HIP_TRY(hipEventRecord(e0, nullptr));
  hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, nullptr, d_out, iters);
  PTZ_HIP_TRY(hipEventRecord(e1, nullptr));
  PTZ_HIP_TRY(hipEventSynchronize(e1));
  PTZ_HIP_TRY(hipGetLastError());
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flop = (double)blocks * 4.0 /*waves*/ * iters * 8.0 * 2048.0;  // 16 x 16 x 4 x 2 per instruction
  *tflops = flop / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d_out);
  return PTZ_OK;
}

// ---- HBM bandwidth micro-benchmark ------------------------------------------------------------------------
// Streaming read (16 bytes per lane per load, sum kept in registers) and streaming copy over a buffer far larger than the
// 256 MB memory-side cache: the rates the HBM-bound kernels are held against.
namespace ptz {
namespace {
__global__ __launch_bounds__(256) void hbm_read_kernel(const double2* __restrict__ src, size_t n, double* out)
{
  double acc = 0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const double2 v = src[i]; acc += v.x + v.y; }
  if (acc == 123.456) out[0] = acc;  // never true: keeps the loads alive
}
__global__ __launch_bounds__(256) void hbm_copy_kernel(const double2* __restrict__ src, double2* __restrict__ dst, size_t n)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}
}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_hbm_bandwidth(int32_t device_id, double* read_gbps, double* copy_gbps)
{
  using namespace ptz;
  clear_stale_error(__func__);
  if (!read_gbps || !copy_gbps) return PTZ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  hipDeviceProp_t prop;
  PTZ_HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  const size_t bytes = (size_t)4 << 30, n = bytes / sizeof(double2);
  double2 *a = nullptr, *bq = nullptr;
  double* d_out = nullptr;
  PTZ_HIP_TRY(hipMalloc(&a, bytes));
  if (hipMalloc(&bq, bytes) != hipSuccess) { (void)hipFree(a); return PTZ_ENOMEM; }
  PTZ_HIP_TRY(hipMalloc(&d_out, sizeof(double)));
  PTZ_HIP_TRY(hipMemset(a, 0, bytes));
  PTZ_HIP_TRY(hipMemset(bq, 0, bytes));
  hipEvent_t e0, e1;
  PTZ_HIP_TRY(hipEventCreate(&e0));
  PTZ_HIP_TRY(hipEventCreate(&e1));
  const int blocks = prop.multiProcessorCount * 16;
  float ms = 0, best_r = 1e30f, best_c = 1e30f;
  for (int rep = 0; rep < 4; ++rep) {
    PTZ_HIP_TRY(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(hbm_read_kernel, dim3(blocks), dim3(256), 0, nullptr, a, n, d_out);
    PTZ_HIP_TRY(hipEventRecord(e1, nullptr));
    PTZ_HIP_TRY(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best_r) best_r = ms;
    PTZ_HIP_TRY(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(hbm_copy_kernel, dim3(blocks), dim3(256), 0, nullptr, a, bq, n);
    PTZ_HIP_TRY(hipEventRecord(e1, nullptr));
    PTZ_HIP_TRY(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (rep > 0 && ms < best_c) best_c = ms;
  }
  PTZ_HIP_TRY(hipGetLastError());
  *read_gbps = (double)bytes / (best_r * 1e-3) / 1e9;
  *copy_gbps = 2.0 * (double)bytes / (best_c * 1e-3) / 1e9;  // read + write
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(a); (void)hipFree(bq); (void)hipFree(d_out);
  return PTZ_OK;
}

// ---- C-ABI test / micro-benchmark entry ---------------------------------------------------------------
extern "C" int32_t ptz_chol_solve_batch(int32_t count, int32_t n, const double* A, const double* rhs, double* x,
                                        int32_t* fail, int32_t device_id, double* device_ms)
{
  using namespace ptz;
  if (count <= 0 || n <= 0 || !A || !rhs || !x) return PTZ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  CholBatch cb;
  cb.count = count;
  cb.np = chol_padded_order(n);
  const int np = cb.np, nt = np / CHOL_NB;
  double *dA = nullptr, *dL = nullptr, *dx = nullptr, *dD = nullptr;
  int *dn = nullptr, *dfail = nullptr;
  PTZ_HIP_TRY(hipMalloc(&dA, sizeof(double) * (size_t)count * np * np));
  PTZ_HIP_TRY(hipMalloc(&dL, sizeof(double) * (size_t)count * nt * CHOL_NB * CHOL_NB));
  PTZ_HIP_TRY(hipMalloc(&dx, sizeof(double) * (size_t)count * np));
  PTZ_HIP_TRY(hipMalloc(&dD, sizeof(double) * (size_t)count * nt * 4 * 16 * 16));
  PTZ_HIP_TRY(hipMalloc(&dn, sizeof(int) * count));
  PTZ_HIP_TRY(hipMalloc(&dfail, sizeof(int) * count));
  cb.A = dA; cb.Ldiag = dL; cb.Dinv = dD; cb.n = dn; cb.fail = dfail;
  double *dL2 = nullptr, *dLi = nullptr;
  int* dctl = nullptr;
  if (count < 8) {  // the path a few bundle-adjustment scenes take
    PTZ_HIP_TRY(hipMalloc(&dL2, sizeof(double) * (size_t)count * np * np));
    PTZ_HIP_TRY(hipMemset(dL2, 0, sizeof(double) * (size_t)count * np * np));
    cb.L = dL2;
    PTZ_HIP_TRY(hipMalloc(&dctl, sizeof(int) * chol_chain_ctl_ints(np)));
    PTZ_HIP_TRY(hipMemset(dctl, 0, sizeof(int) * chol_chain_ctl_ints(np)));
    cb.chain_ctl = dctl;
  }
  PTZ_HIP_TRY(hipMalloc(&dLi, sizeof(double) * (size_t)count * nt * CHOL_NB * CHOL_NB));
  cb.Linv = dLi;
  {
    int* hn = new int[count];
    for (int i = 0; i < count; ++i) hn[i] = n;
    PTZ_HIP_TRY(hipMemcpy(dn, hn, sizeof(int) * count, hipMemcpyHostToDevice));
    delete[] hn;
  }
  hipStream_t stream;
  PTZ_HIP_TRY(hipStreamCreate(&stream));
  hipEvent_t e0, e1;
  PTZ_HIP_TRY(hipEventCreate(&e0));
  PTZ_HIP_TRY(hipEventCreate(&e1));
  chol_clear(cb, stream);
  for (int s = 0; s < count; ++s) {
    PTZ_HIP_TRY(hipMemcpy2DAsync(dA + (size_t)s * np * np, sizeof(double) * np, A + (size_t)s * n * n, sizeof(double) * n,
                                 sizeof(double) * n, n, hipMemcpyHostToDevice, stream));
    PTZ_HIP_TRY(hipMemcpyAsync(dA + (size_t)s * np * np + (size_t)n * np, rhs + (size_t)s * n, sizeof(double) * n,
                               hipMemcpyHostToDevice, stream));
  }
  PTZ_HIP_TRY(hipEventRecord(e0, stream));
  chol_factor_solve(cb, dx, stream);
  PTZ_HIP_TRY(hipEventRecord(e1, stream));
  PTZ_HIP_TRY(hipStreamSynchronize(stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (device_ms) *device_ms = ms;
  for (int s = 0; s < count; ++s)
    PTZ_HIP_TRY(hipMemcpy(x + (size_t)s * n, dx + (size_t)s * np, sizeof(double) * n, hipMemcpyDeviceToHost));
  bool lost = false;
  {
    int* hf = new int[count];
    PTZ_HIP_TRY(hipMemcpy(hf, dfail, sizeof(int) * count, hipMemcpyDeviceToHost));
    for (int s = 0; s < count; ++s) { lost |= (hf[s] & 2) != 0; if (fail) fail[s] = hf[s] & 1; }
    delete[] hf;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(stream);
  (void)hipFree(dA); (void)hipFree(dL); (void)hipFree(dD); (void)hipFree(dx); (void)hipFree(dn); (void)hipFree(dfail);
  if (dL2) (void)hipFree(dL2);
  if (dLi) (void)hipFree(dLi);
  if (dctl) (void)hipFree(dctl);
  return lost ? PTZ_ENODEVICE : PTZ_OK;  // (a tile hand-over of the one-launch factorisation that did not arrive)
}

// ---- diagnostic entry: every factorisation family, chosen by the caller -----------------------------------
// The same dense solve as ptz_chol_solve_batch with three things the tests of the kernels need and the product never asks for:
// the launch path is the caller's (0: chol_factor_solve's own choice, 1: chol_chain_kernel, 2: chol_col_step_kernel per step,
// 3: right-looking panel + syrk, 4: left-looking chol_update_col_h_kernel + panel), every system has its own order n[i] inside
// one padded order np = chol_padded_order(max n), and the buffers the kernels write before they read can start from garbage.
//
// What has to start at zero, read off the kernels: chain_ctl (tickets, generation and flags of chol_chain_kernel: a flag counts
// as raised when it holds the launch's generation) and A, which chol_clear zeroes in front of every assembly.  L, the second
// matrix of paths 1 and 2, is handed over as the bundle adjustment hands it over, zeroed once at creation like chain_ctl: the
// kernels write its strictly-lower tiles of the block columns that hold rows <= n and the back-substitution reads those and
// the right-hand-side row's, so a dense system may well not need the zeros -- that is not tried here.  Ldiag, Dinv, Linv and
// x are written by the factorisation / back-substitution before anything reads them; flags bit 0 fills them with 0xFF bytes
// (NaNs) first so that a read of stale memory shows in the solution (the tests' poisoned runs return the unpoisoned bits).
// An inactive system (active[i] == 0) is skipped by every kernel: x[i] and fail[i] come back as the caller passed them.
namespace {
struct DebugCholBuffers {
  std::vector<void*> p;
  hipStream_t stream = nullptr;
  template <class T> hipError_t get(T** out, size_t bytes) { void* q = nullptr; const hipError_t e = hipMalloc(&q, bytes); if (e == hipSuccess) p.push_back(q); *out = (T*)q; return e; }
  ~DebugCholBuffers() { if (stream) (void)hipStreamDestroy(stream); for (void* q : p) (void)hipFree(q); }
};
}  // namespace

extern "C" int32_t ptz_debug_chol_solve(int32_t count, const int32_t* n, int32_t ld, const double* A, const double* rhs, double* x, int32_t* fail,
                                        const int32_t* active, int32_t path, int32_t flags, int32_t device_id)
{
  using namespace ptz;
  if (count <= 0 || !n || !A || !rhs || !x || !fail || path < 0 || path > 4) return PTZ_EINVAL;
  int n_max = 0;
  for (int i = 0; i < count; ++i) { if (n[i] <= 0) return PTZ_EINVAL; n_max = std::max(n_max, (int)n[i]); }
  if (ld < n_max) return PTZ_EINVAL;
  if (path == 1 && count > CHOL_CHAIN_SLOTS) return PTZ_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  clear_stale_error(__func__);
  CholBatch cb;
  cb.count = count;
  cb.np = chol_padded_order(n_max);
  const size_t np = cb.np, nt = np / CHOL_NB;
  const size_t tile_bytes = sizeof(double) * (size_t)count * nt * CHOL_NB * CHOL_NB, dinv_bytes = sizeof(double) * (size_t)count * nt * 4 * 16 * 16;
  const size_t mat_bytes = sizeof(double) * (size_t)count * np * np, x_bytes = sizeof(double) * (size_t)count * np;
  DebugCholBuffers buf;
  double *dx = nullptr;
  int *dn = nullptr, *dact = nullptr;
  PTZ_HIP_TRY(buf.get(&cb.A, mat_bytes));
  PTZ_HIP_TRY(buf.get(&cb.Ldiag, tile_bytes));
  PTZ_HIP_TRY(buf.get(&cb.Dinv, dinv_bytes));
  PTZ_HIP_TRY(buf.get(&cb.Linv, tile_bytes));
  PTZ_HIP_TRY(buf.get(&dx, x_bytes));
  PTZ_HIP_TRY(buf.get(&dn, sizeof(int) * count));
  PTZ_HIP_TRY(buf.get(&cb.fail, sizeof(int) * count));
  cb.n = dn;
  // the second matrix marks the one-launch / one-launch-per-step paths (chol_factor_solve); path 0 has it where
  // ptz_chol_solve_batch has it
  if (path == 1 || path == 2 || (path == 0 && count < 8)) {
    PTZ_HIP_TRY(buf.get(&cb.L, mat_bytes));
    PTZ_HIP_TRY(hipMemset(cb.L, 0, mat_bytes));
    PTZ_HIP_TRY(buf.get(&cb.chain_ctl, sizeof(int) * chol_chain_ctl_ints((int)np)));
    PTZ_HIP_TRY(hipMemset(cb.chain_ctl, 0, sizeof(int) * chol_chain_ctl_ints((int)np)));
  }
  if (flags & 1) {
    PTZ_HIP_TRY(hipMemset(cb.Ldiag, 0xFF, tile_bytes));
    PTZ_HIP_TRY(hipMemset(cb.Dinv, 0xFF, dinv_bytes));
    PTZ_HIP_TRY(hipMemset(cb.Linv, 0xFF, tile_bytes));
    PTZ_HIP_TRY(hipMemset(dx, 0xFF, x_bytes));
  }
  PTZ_HIP_TRY(hipMemcpy(dn, n, sizeof(int) * count, hipMemcpyHostToDevice));
  PTZ_HIP_TRY(hipMemcpy(cb.fail, fail, sizeof(int) * count, hipMemcpyHostToDevice));
  if (active) {
    PTZ_HIP_TRY(buf.get(&dact, sizeof(int) * count));
    PTZ_HIP_TRY(hipMemcpy(dact, active, sizeof(int) * count, hipMemcpyHostToDevice));
    cb.active = dact;
    for (int s = 0; s < count; ++s)  // what a skipped system's row of x must still hold afterwards
      if (!active[s]) PTZ_HIP_TRY(hipMemcpy(dx + (size_t)s * np, x + (size_t)s * ld, sizeof(double) * n[s], hipMemcpyHostToDevice));
  }
  PTZ_HIP_TRY(hipStreamCreate(&buf.stream));
  hipStream_t stream = buf.stream;
  chol_clear(cb, stream);
  for (int s = 0; s < count; ++s) {
    if (active && !active[s]) continue;
    const size_t ns = (size_t)n[s];
    PTZ_HIP_TRY(hipMemcpy2DAsync(cb.A + (size_t)s * np * np, sizeof(double) * np, A + (size_t)s * ld * ld, sizeof(double) * ld,
                                 sizeof(double) * ns, ns, hipMemcpyHostToDevice, stream));
    PTZ_HIP_TRY(hipMemcpyAsync(cb.A + (size_t)s * np * np + ns * np, rhs + (size_t)s * ld, sizeof(double) * ns, hipMemcpyHostToDevice, stream));
  }
  const int ntile = (int)nt;
  switch (path) {
    case 0:
      chol_factor_solve(cb, dx, stream);
      break;
    case 1:
      chol_chain_launch(cb, stream);
      chol_backsolve_launch(cb, dx, stream);
      break;
    case 2:
      chol_diag_launch(cb, -1, stream);
      for (int st = 0; st + 1 < chol_step_count(cb); ++st) chol_col_step_launch(cb, st, stream);
      chol_backsolve_launch(cb, dx, stream);
      break;
    case 3:
      for (int k = 0; k < ntile; ++k) {
        chol_panel_launch(cb, k, stream, /*diag_done=*/k > 0);
        chol_syrk_launch(cb, k, stream, 0, /*fuse_diag=*/true);
      }
      chol_tile_inverse_launch(cb, stream);
      chol_backsolve_launch(cb, dx, stream);
      break;
    default:
      // The left-looking loop of chol_factor_solve_profiled (ptz_ba.hip, the path of every large bundle-adjustment batch)
      // without its profiling brackets: a change to either loop belongs in both.
      for (int k = 0; k < ntile; ++k) {
        if (k > 0) chol_update_col_launch(cb, k, stream, /*fuse_diag=*/true);
        chol_panel_launch(cb, k, stream, /*diag_done=*/k > 0);
      }
      chol_tile_inverse_launch(cb, stream);
      chol_backsolve_launch(cb, dx, stream);
      break;
  }
  PTZ_HIP_TRY(hipStreamSynchronize(stream));
  PTZ_HIP_TRY(hipGetLastError());
  for (int s = 0; s < count; ++s)
    PTZ_HIP_TRY(hipMemcpy(x + (size_t)s * ld, dx + (size_t)s * np, sizeof(double) * n[s], hipMemcpyDeviceToHost));
  bool lost = false;
  {
    std::vector<int> hf(count);
    PTZ_HIP_TRY(hipMemcpy(hf.data(), cb.fail, sizeof(int) * count, hipMemcpyDeviceToHost));
    for (int s = 0; s < count; ++s) {
      if (active && !active[s]) continue;
      lost |= (hf[s] & 2) != 0;
      fail[s] = hf[s] & 1;
    }
  }
  return lost ? PTZ_ENODEVICE : PTZ_OK;  // (a tile hand-over of the one-launch factorisation that did not arrive)
}
