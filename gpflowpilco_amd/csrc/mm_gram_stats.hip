// Streamed Gram statistics of the collapsed (SGPR) bound, Phi = K K^T [L,M,M] and Psi = K R [L,M,Q], and their adjoint
// (models.SVGP.collapsed_elbo through autodiff.GramStatsSEFunction); f64.  The schedule is mm_gram_stats.h's; K [L,M,N] is never
// stored: its tiles are formed from differences (mm_gram.h) where they are used.
//
// Forward, k_stats_fwd: one workgroup per item (latent, block pair (ib, jb <= ib), split).  It stages its two blocks of Z once; per
// chunk of 64 points it stages X, forms K[ib] row-major (the A operand, row stride 66) and K[jb] transposed (the B operand, row
// stride 80) in LDS, and wave w adds rows 16 w .. 16 w + 15 x 64 columns of the product into 4 accumulators of
// v_mfma_f64_16x16x4_f64.  Items with jb == 0 add K[ib] R on the vector pipe.  k_stats_fwd_sum adds the splits' partials in index
// order and writes Phi from the lower triangle alone: symmetric to the bit.
//
// Adjoint: k_stats_sym writes Gs = GPhi + GPhi^T once; k_stats_bwd walks (latent, chunk) items as k_predict_se does, the K strip in
// the workgroup's workspace slice, acc = sum_jb Gs[ib][jb] K[jb] + GPsi[ib] R^T on the matrix pipe, t = acc o K[ib] in LDS, then
// k_gram_se_bwd's second phase (one thread per (row, dimension) pair, columns in index order) into the workgroup's own partial
// slice; k_stats_bwd_sum adds the slices in index order.  No atomics anywhere: two calls are bit-equal.
#include <hip/hip_runtime.h>
#include <atomic>
#include "mm_common.h"
#include "mm_gram_stats.h"

typedef double f64x4s __attribute__((ext_vector_type(4)));

#define MGS_AS 66        /* row stride of an A-operand tile: lanes (row l15, k kq) fall in distinct banks */
#define MGS_BS 80        /* row stride of a B-operand tile: lanes (k kq, column l15) likewise */
#define MGS_XS 65        /* row stride of the dimension-major points of the adjoint's pair phase */
#define MGS_PSI_ACC ((MGS_B * MGS_QMAX + MGS_THREADS - 1) / MGS_THREADS)      /* (row, column) pairs of Psi per thread: 9 */
#define MGS_PAIR_ACC (MGS_B * MM_DMAX / MGS_THREADS)                          /* (row, dimension) pairs per thread: 8 */

static_assert(MGS_B == 64 && MGS_TN == 64 && MGS_THREADS == 256, "4 waves x 16 rows; thread (c, h) forms 16 entries of column c");
static_assert(MM_DMAX + MM_DMAX * MGS_XS + MM_DMAX * MGS_B <= MGS_B * MGS_BS, "the pair phase stages il, xs and zs in the B tile");
static_assert(MGS_B * MM_DMAX <= MGS_B * MGS_AS && MGS_THREADS <= MGS_B * MGS_AS, "reduction buffers in the A tile");

// ---- forward ----
// LDS, in doubles: A tile [64][66] | B tile [64][80] | il [MM_DMAX] | xs [d][64] | zi [d][64] | zj [d][64] | rs [64][Q]
static inline size_t mgs_fwd_lds_bytes(int d, int Q) {
  return ((size_t)MGS_B * MGS_AS + (size_t)MGS_TN * MGS_BS + MM_DMAX + 3 * (size_t)d * 64 + (size_t)MGS_TN * Q) * sizeof(double);
}

__global__ __launch_bounds__(MGS_THREADS) void k_stats_fwd(int L, int M, int N, int d, int Q, int S, int cps,
                                                           const double* __restrict__ X, const double* __restrict__ R,
                                                           const double* __restrict__ Z, const double* __restrict__ ls,
                                                           const double* __restrict__ var, double* __restrict__ wsPhi,
                                                           double* __restrict__ wsPsi) {
  extern __shared__ double mgs_sm[];
  double* As = mgs_sm;                       // K[ib]: [row m][point]
  double* Bs = As + MGS_B * MGS_AS;          // K[jb] transposed: [point][row m]
  double* il = Bs + MGS_TN * MGS_BS;
  double* xs = il + MM_DMAX;
  double* zi = xs + d * 64;
  double* zj = zi + d * 64;
  double* rs = zj + d * 64;
  const int tid = (int)threadIdx.x;
  const int c = tid & 63, h = tid >> 6;
  const int l15 = tid & 15, kq = (tid >> 4) & 3, wv = tid >> 6;
  const long long pairs = mgs_pairs(M);
  const long long item = blockIdx.x;
  const int s = (int)(item % S);
  const long long lp = item / S;
  const int l = (int)(lp / pairs);
  int ib, jb;
  mgs_pair_blocks(lp - (long long)l * pairs, ib, jb);
  const bool with_psi = Q > 0 && jb == 0;
  const int nch = mgs_chunks(N);
  const int c0 = s * cps, c1 = c0 + cps < nch ? c0 + cps : nch;
  const double* Zl = Z + (size_t)l * M * d;
  const double v = var[l];

  if (tid < d) il[tid] = 1.0 / ls[(size_t)l * d + tid];
  for (int idx = tid; idx < MGS_B * d; idx += MGS_THREADS) {
    const int r = idx / d, k = idx - r * d;
    zi[k * 64 + r] = mgs_row_valid(M, ib, r) ? Zl[((size_t)ib * MGS_B + r) * d + k] : 0.0;
    zj[k * 64 + r] = mgs_row_valid(M, jb, r) ? Zl[((size_t)jb * MGS_B + r) * d + k] : 0.0;
  }
  f64x4s acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = (f64x4s){0.0, 0.0, 0.0, 0.0};
  double pacc[MGS_PSI_ACC];
#pragma unroll
  for (int i = 0; i < MGS_PSI_ACC; ++i) pacc[i] = 0.0;

  for (int ch = c0; ch < c1; ++ch) {
    const long long n0 = (long long)ch * MGS_TN;
    __syncthreads();                                            // the previous chunk's tiles, xs and rs have been read
    for (int idx = tid; idx < MGS_TN * d; idx += MGS_THREADS) {
      const int cc = idx / d, k = idx - cc * d;
      xs[k * 64 + cc] = mgs_col_valid(N, ch, cc) ? X[(size_t)(n0 + cc) * d + k] : 0.0;
    }
    if (with_psi) {
      for (int idx = tid; idx < MGS_TN * Q; idx += MGS_THREADS) {
        const int cc = idx / Q;
        rs[idx] = mgs_col_valid(N, ch, cc) ? R[(size_t)n0 * Q + idx] : 0.0;
      }
    }
    __syncthreads();
    // K[ib]: thread (c, h) forms rows 16 h .. 16 h + 15 of point c; K[jb]^T: thread (c, h) forms points 16 h .. of row c
    for (int q = 0; q < 4; ++q) {
      double a4[4] = {0.0, 0.0, 0.0, 0.0}, b4[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < d; ++k) {
        const double ilk = il[k];
        const double xk = xs[k * 64 + c], zk = zj[k * 64 + c];
        const double* zr = zi + k * 64 + h * 16 + q * 4;
        const double* xr = xs + k * 64 + h * 16 + q * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a4[r] = mmg_sq_acc(xk, zr[r], ilk, a4[r]);
          b4[r] = mmg_sq_acc(xr[r], zk, ilk, b4[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = h * 16 + q * 4 + r;
        const bool a_ok = mgs_row_valid(M, ib, rr) && mgs_col_valid(N, ch, c);
        const bool b_ok = mgs_row_valid(M, jb, c) && mgs_col_valid(N, ch, rr);
        As[rr * MGS_AS + c] = a_ok ? v * mmg_profile(a4[r]) : 0.0;
        Bs[rr * MGS_BS + c] = b_ok ? v * mmg_profile(b4[r]) : 0.0;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < MGS_TN / 4; ++st) {
      const double a = As[(wv * 16 + l15) * MGS_AS + 4 * st + kq];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(4 * st + kq) * MGS_BS + ct * 16 + l15], acc[ct], 0, 0, 0);
    }
    if (with_psi) {
      // pair e = 256 i + tid: row e & 63, column e >> 6 (one column of R per wave and step: a broadcast)
#pragma unroll
      for (int i = 0; i < MGS_PSI_ACC; ++i) {
        const int e = i * MGS_THREADS + tid, q = e >> 6;
        if (q < Q) {
          double sum = pacc[i];
          for (int j = 0; j < MGS_TN; ++j) sum = fma(As[c * MGS_AS + j], rs[j * Q + q], sum);
          pacc[i] = sum;
        }
      }
    }
  }
  // accumulator: lane (l15 = column, kq), register r <-> row kq + 4 r of the wave's 16
  double* part = wsPhi + ((size_t)lp * S + s) * (MGS_B * MGS_B);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(wv * 16 + kq + 4 * r) * MGS_B + ct * 16 + l15] = acc[ct][r];
  if (with_psi) {
    double* pp = wsPsi + (((size_t)l * mgs_blocks(M) + ib) * S + s) * ((size_t)MGS_B * Q);
#pragma unroll
    for (int i = 0; i < MGS_PSI_ACC; ++i) {
      const int e = i * MGS_THREADS + tid, q = e >> 6;
      if (q < Q) pp[(size_t)c * Q + q] = pacc[i];
    }
  }
}

// Phi[l][i][j] and Psi[l][m][q] from the splits' partials, in index order; Phi from the lower triangle (of the blocks and inside
// the diagonal blocks)
__global__ __launch_bounds__(MGS_THREADS) void k_stats_fwd_sum(int L, int M, int Q, int S, const double* __restrict__ wsPhi,
                                                               const double* __restrict__ wsPsi, double* __restrict__ Phi,
                                                               double* __restrict__ Psi) {
  const size_t mm = (size_t)M * M, nphi = (size_t)L * mm, npsi = (size_t)L * M * Q;
  size_t i = (size_t)blockIdx.x * MGS_THREADS + threadIdx.x;
  double sum = 0.0;
  if (i < nphi) {
    const size_t l = i / mm, rem = i - l * mm;
    int a = (int)(rem / M), b = (int)(rem - (size_t)a * M);
    if (b > a) { const int t = a; a = b; b = t; }
    const int ib = a / MGS_B, jb = b / MGS_B;
    const double* p = wsPhi + ((l * (size_t)mgs_pairs(M) + (size_t)mgs_pair_index(ib, jb)) * S) * (MGS_B * MGS_B)
                      + (size_t)(a - ib * MGS_B) * MGS_B + (b - jb * MGS_B);
    for (int s = 0; s < S; ++s) sum += p[(size_t)s * (MGS_B * MGS_B)];
    Phi[i] = sum;
    return;
  }
  i -= nphi;
  if (i < npsi) {
    const size_t mq = (size_t)M * Q, l = i / mq, rem = i - l * mq;
    const int m = (int)(rem / Q), q = (int)(rem - (size_t)m * Q), ib = m / MGS_B;
    const double* p = wsPsi + ((l * mgs_blocks(M) + ib) * S) * ((size_t)MGS_B * Q) + (size_t)(m - ib * MGS_B) * Q + q;
    for (int s = 0; s < S; ++s) sum += p[(size_t)s * MGS_B * Q];
    Psi[i] = sum;
  }
}

// ---- adjoint ----
__global__ __launch_bounds__(MGS_THREADS) void k_stats_sym(int M, size_t total, const double* __restrict__ G, double* __restrict__ Gs) {
  const size_t i = (size_t)blockIdx.x * MGS_THREADS + threadIdx.x;
  if (i >= total) return;
  const size_t mm = (size_t)M * M, l = i / mm, rem = i - l * mm, a = rem / M, b = rem - a * M;
  Gs[i] = G[i] + G[l * mm + b * M + a];
}

#define MGS_BWD_LDS_DOUBLES (MGS_B * MGS_AS + MGS_B * MGS_BS)

// (two workgroups per CU by LDS: at most 256 registers a lane)
__global__ __launch_bounds__(MGS_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_stats_bwd(
    int L, int M, int N, int d, int Q, int groups, const double* __restrict__ Gs, const double* __restrict__ GPsi,
    const double* __restrict__ X, const double* __restrict__ R, const double* __restrict__ Z, const double* __restrict__ ls,
    const double* __restrict__ var, double* __restrict__ strips, double* __restrict__ slices) {
  extern __shared__ double mgs_sm[];
  double* As = mgs_sm;                       // block of Gs (or of GPsi); then the t tile [64][66]; then the pairs' gls sums
  double* Bs = mgs_sm + MGS_B * MGS_AS;      // tile of K (or of R^T); strip and pair phases: il | xs [d][65] | zs [d][64]
  double* il = Bs;
  double* xs = il + MM_DMAX;
  double* zs = xs + d * MGS_XS;
  const int tid = (int)threadIdx.x;
  const int c = tid & 63, h = tid >> 6;
  const int l15 = tid & 15, kq = (tid >> 4) & 3, wv = tid >> 6;
  const int l = (int)blockIdx.x / groups, w = (int)blockIdx.x - l * groups;
  const int nb = mgs_blocks(M), nch = mgs_chunks(N);
  const int Qp = (Q + 3) & ~3;
  const double* Zl = Z + (size_t)l * M * d;
  const double* Gl = Gs + (size_t)l * M * M;
  const double v = var[l];
  double* strip = strips + (size_t)blockIdx.x * mgs_strip(M);
  double* slZ = slices + (size_t)blockIdx.x * mgs_slice(M, d);
  double* slL = slZ + (size_t)M * d;
  double* slV = slL + d;
  for (size_t i = tid; i < mgs_slice(M, d); i += MGS_THREADS) slZ[i] = 0.0;
  double gv = 0.0;

  for (int ch = w; ch < nch; ch += groups) {
    const long long n0 = (long long)ch * MGS_TN;
    const bool col_ok = mgs_col_valid(N, ch, c);
    // ---- the K strip ----
    __syncthreads();                                            // the previous item's last reads of As and Bs
    if (tid < d) il[tid] = 1.0 / ls[(size_t)l * d + tid];
    for (int idx = tid; idx < MGS_TN * d; idx += MGS_THREADS) {
      const int cc = idx / d, k = idx - cc * d;
      xs[k * MGS_XS + cc] = mgs_col_valid(N, ch, cc) ? X[(size_t)(n0 + cc) * d + k] : 0.0;
    }
    for (int jb = 0; jb < nb; ++jb) {
      __syncthreads();                                          // the previous block's zs has been read
      for (int idx = tid; idx < MGS_B * d; idx += MGS_THREADS) {
        const int r = idx / d, k = idx - r * d;
        zs[k * MGS_B + r] = mgs_row_valid(M, jb, r) ? Zl[((size_t)jb * MGS_B + r) * d + k] : 0.0;
      }
      __syncthreads();
      for (int q = 0; q < 4; ++q) {
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < d; ++k) {
          const double xk = xs[k * MGS_XS + c], ilk = il[k];
          const double* zk = zs + k * MGS_B + h * 16 + q * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) a4[r] = mmg_sq_acc(xk, zk[r], ilk, a4[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = h * 16 + q * 4 + r;
          strip[((size_t)jb * MGS_B + rr) * MGS_TN + c] = (col_ok && mgs_row_valid(M, jb, rr)) ? v * mmg_profile(a4[r]) : 0.0;
        }
      }
    }
    // ---- per row block: acc on the matrix pipe, t = acc o K[ib], the sums ----
    for (int ib = 0; ib < nb; ++ib) {
      f64x4s acc[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = (f64x4s){0.0, 0.0, 0.0, 0.0};
      for (int jb = 0; jb <= nb; ++jb) {                        // jb == nb: the block of GPsi against R^T
        if (jb == nb && Q == 0) break;
        __syncthreads();                                        // the previous operands (the strip's writes, too) are done with
        if (jb < nb) {
          const bool cc_ok = mgs_row_valid(M, jb, c);
          const double* gp = Gl + ((size_t)ib * MGS_B + h) * M + (size_t)jb * MGS_B + c;
#pragma unroll 4
          for (int i = 0; i < 16; ++i)                          // row 4 i + h, column c
            As[(4 * i + h) * MGS_AS + c] = (cc_ok && mgs_row_valid(M, ib, 4 * i + h)) ? gp[(size_t)(4 * i) * M] : 0.0;
          const double* kp = strip + (size_t)jb * MGS_B * MGS_TN;
#pragma unroll 4
          for (int i = 0; i < 16; ++i) Bs[(4 * i + h) * MGS_BS + c] = kp[(4 * i + h) * MGS_TN + c];
        } else {
          const double* gp = GPsi + ((size_t)l * M + (size_t)ib * MGS_B) * Q;
          for (int idx = tid; idx < MGS_B * Qp; idx += MGS_THREADS) {
            const int r = idx / Qp, q = idx - r * Qp;
            As[r * MGS_AS + q] = (q < Q && mgs_row_valid(M, ib, r)) ? gp[(size_t)r * Q + q] : 0.0;
          }
          for (int idx = tid; idx < MGS_TN * Qp; idx += MGS_THREADS) {
            const int cc = idx / Qp, q = idx - cc * Qp;
            Bs[q * MGS_BS + cc] = (q < Q && mgs_col_valid(N, ch, cc)) ? R[(size_t)(n0 + cc) * Q + q] : 0.0;
          }
        }
        __syncthreads();
        const int steps = jb < nb ? MGS_B / 4 : Qp / 4;
        for (int st = 0; st < steps; ++st) {
          const double a = As[(wv * 16 + l15) * MGS_AS + 4 * st + kq];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct)
            acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[(4 * st + kq) * MGS_BS + ct * 16 + l15], acc[ct], 0, 0, 0);
        }
      }
      __syncthreads();                                          // the operands have been read: As takes t, Bs the points
      const double* kp = strip + (size_t)ib * MGS_B * MGS_TN;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wv * 16 + kq + 4 * r, col = ct * 16 + l15;
          const double t = acc[ct][r] * kp[row * MGS_TN + col];
          As[row * MGS_AS + col] = t;
          gv += t;
        }
      if (tid < d) il[tid] = 1.0 / ls[(size_t)l * d + tid];
      for (int idx = tid; idx < MGS_TN * d; idx += MGS_THREADS) {
        const int cc = idx / d, k = idx - cc * d;
        xs[k * MGS_XS + cc] = mgs_col_valid(N, ch, cc) ? X[(size_t)(n0 + cc) * d + k] : 0.0;
      }
      for (int idx = tid; idx < MGS_B * d; idx += MGS_THREADS) {
        const int r = idx / d, k = idx - r * d;
        zs[k * MGS_B + r] = mgs_row_valid(M, ib, r) ? Zl[((size_t)ib * MGS_B + r) * d + k] : 0.0;
      }
      __syncthreads();
      // (row, dimension) pairs p = r d + k; rows past M and columns past N carry t = 0
      const int P = MGS_B * d;
      double alr[MGS_PAIR_ACC];
#pragma unroll
      for (int i = 0; i < MGS_PAIR_ACC; ++i) {
        const int p = i * MGS_THREADS + tid;
        alr[i] = 0.0;
        if (p < P) {
          const int r = p / d, k = p - r * d;
          const double z = zs[k * MGS_B + r];
          double az = 0.0, al = 0.0;
          for (int j = 0; j < MGS_TN; ++j) mmg_adj_acc(As[r * MGS_AS + j], xs[k * MGS_XS + j], z, az, al);
          alr[i] = al;
          if (mgs_row_valid(M, ib, r)) slZ[((size_t)ib * MGS_B + r) * d + k] += az;
        }
      }
      __syncthreads();                                          // the t tile is dead: its space takes the pairs' gls sums
#pragma unroll
      for (int i = 0; i < MGS_PAIR_ACC; ++i) {
        const int p = i * MGS_THREADS + tid;
        if (p < P) As[p] = alr[i];
      }
      __syncthreads();
      if (tid < d) {
        double sum = 0.0;
        for (int r = 0; r < MGS_B; ++r) sum += As[r * d + tid];
        slL[tid] += sum;
      }
    }
  }
  // gvar's sum of the workgroup: the threads' sums in a fixed order
  __syncthreads();
  As[tid] = gv;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int j = 0; j < MGS_THREADS; ++j) sum += As[j];
    slV[0] = sum;
  }
}

// the slices of a latent's workgroups, added in index order, and what turns the sums into gradients
__global__ __launch_bounds__(MGS_THREADS) void k_stats_bwd_sum(int L, int M, int d, int groups, const double* __restrict__ slices,
                                                               const double* __restrict__ ls, const double* __restrict__ var,
                                                               double* __restrict__ gZ, double* __restrict__ gls,
                                                               double* __restrict__ gvar) {
  const size_t md = (size_t)M * d, nz = (size_t)L * md, nl = (size_t)L * d, sl = mgs_slice(M, d);
  size_t i = (size_t)blockIdx.x * MGS_THREADS + threadIdx.x;
  double sum = 0.0;
  if (i < nz) {
    const size_t l = i / md, rem = i - l * md, k = rem % d;
    for (int w = 0; w < groups; ++w) sum += slices[(l * groups + w) * sl + rem];
    gZ[i] = mmg_gz_scale(sum, 1.0 / ls[l * d + k]);
    return;
  }
  i -= nz;
  if (i < nl) {
    const size_t l = i / d, k = i - l * d;
    for (int w = 0; w < groups; ++w) sum += slices[(l * groups + w) * sl + md + k];
    gls[i] = mmg_gl_scale(sum, 1.0 / ls[i]);
    return;
  }
  i -= nl;
  if (i < (size_t)L) {
    for (int w = 0; w < groups; ++w) sum += slices[(i * groups + w) * sl + md + d];
    gvar[i] = sum / var[i];
  }
}

static int mgs_check_dims(int L, int M, int N, int d, int Q) {
  if (L <= 0 || M <= 0 || N <= 0 || d <= 0 || d > MM_DMAX || Q < 0 || Q > MGS_QMAX) return MM_E_DIM;
  if (M > MGS_M_MAX || L > 65535) return MM_E_DIM;
  if ((long long)L * mgs_pairs(M) * mgs_splits_max(L, M) > 0x7fffffffLL) return MM_E_DIM;          // the forward grid
  return 0;
}

extern "C" size_t mm_gram_stats_workspace_bytes(int L, int M, int N, int d, int Q) {
  if (mgs_check_dims(L, M, N, d, Q)) return 0;
  return mm_align_up(mgs_workspace(L, M, d, Q).total * sizeof(double), 256);
}

// hipFuncAttributeMaxDynamicSharedMemorySize once per device and kernel (a bitmap over the device ordinals)
static hipError_t mgs_set_max_lds_once(const void* fn, int bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && bit) done.fetch_or(bit, std::memory_order_release);
  return e;
}

extern "C" int mm_gram_stats_se(int L, int M, int N, int d, int Q, const double* X, const double* R, const double* Z,
                                const double* ls, const double* var, double* Phi, double* Psi, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (int rc = mgs_check_dims(L, M, N, d, Q)) return rc;
  if (!X || !Z || !ls || !var || !Phi || !workspace) return MM_E_ARG;
  if ((Q == 0) != (R == nullptr) || (Q == 0) != (Psi == nullptr)) return MM_E_ARG;
  const MGSWs w = mgs_workspace(L, M, d, Q);
  if (workspace_bytes < w.total * sizeof(double)) return MM_E_WORKSPACE;
  static std::atomic<unsigned long long> done{0};
  if (hipError_t e = mgs_set_max_lds_once((const void*)k_stats_fwd, (int)mgs_fwd_lds_bytes(MM_DMAX, MGS_QMAX), done)) return (int)e;
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int S = mgs_splits(L, M, N), cps = mgs_chunks_per_split(L, M, N);
  const long long items = (long long)L * mgs_pairs(M) * S;
  k_stats_fwd<<<(unsigned)items, MGS_THREADS, mgs_fwd_lds_bytes(d, Q), st>>>(L, M, N, d, Q, S, cps, X, R, Z, ls, var, ws + w.phi,
                                                                             ws + w.psi);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const size_t nout = (size_t)L * M * M + (size_t)L * M * Q;
  k_stats_fwd_sum<<<(unsigned)((nout + MGS_THREADS - 1) / MGS_THREADS), MGS_THREADS, 0, st>>>(L, M, Q, S, ws + w.phi, ws + w.psi, Phi,
                                                                                              Psi);
  return (int)hipGetLastError();
}

extern "C" int mm_gram_stats_se_backward(int L, int M, int N, int d, int Q, const double* GPhi, const double* GPsi, const double* X,
                                         const double* R, const double* Z, const double* ls, const double* var, double* gZ,
                                         double* gls, double* gvar, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = mgs_check_dims(L, M, N, d, Q)) return rc;
  if (!GPhi || !X || !Z || !ls || !var || !gZ || !gls || !gvar || !workspace) return MM_E_ARG;
  if ((Q == 0) != (R == nullptr) || (Q == 0) != (GPsi == nullptr)) return MM_E_ARG;
  const MGSWs w = mgs_workspace(L, M, d, Q);
  if (workspace_bytes < w.total * sizeof(double)) return MM_E_WORKSPACE;
  const int lds = MGS_BWD_LDS_DOUBLES * (int)sizeof(double);
  static std::atomic<unsigned long long> done{0};
  if (hipError_t e = mgs_set_max_lds_once((const void*)k_stats_bwd, lds, done)) return (int)e;
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const size_t lmm = (size_t)L * M * M;
  k_stats_sym<<<(unsigned)((lmm + MGS_THREADS - 1) / MGS_THREADS), MGS_THREADS, 0, st>>>(M, lmm, GPhi, ws + w.gs);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const int groups = mgs_bwd_groups(L, N);
  k_stats_bwd<<<(unsigned)(L * groups), MGS_THREADS, lds, st>>>(L, M, N, d, Q, groups, ws + w.gs, GPsi, X, R, Z, ls, var,
                                                               ws + w.strips, ws + w.slices);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  const size_t nout = (size_t)L * M * d + (size_t)L * d + (size_t)L;
  k_stats_bwd_sum<<<(unsigned)((nout + MGS_THREADS - 1) / MGS_THREADS), MGS_THREADS, 0, st>>>(L, M, d, groups, ws + w.slices, ls, var,
                                                                                              gZ, gls, gvar);
  return (int)hipGetLastError();
}
