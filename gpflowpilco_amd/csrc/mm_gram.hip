// SE-ARD Gram matrix K [L, M, N] of the SVGP ELBO and its adjoint (models.SVGP.elbo through autodiff.GramSEFunction); f64.
//
// One workgroup owns one (latent l, tile of MMG_TM rows, chunk of MMG_TN columns): grid (chunks, tiles, L).  It stages its MMG_TN data
// points dimension-major in LDS (xs[k][n], row stride MMG_TN + 1) and its MMG_TM inducing points as zs[k][r]; in the entry phase
// thread (c, h) forms the 8 entries of column c, rows 8 h .. 8 h + 7, so every access to K and G has consecutive lanes on
// consecutive n.  The adjoint RECOMPUTES K from the operands (3 d + 30 flops against 8 bytes per entry), leaves t = G K in LDS and
// turns to a second phase with one thread per (row, dimension) -- a tile with fewer than 256 such pairs splits each pair's columns over
// 256 / pairs threads, combined in a fixed order.  A workgroup writes its partial gZ, gls and gvar to the workspace and a second
// launch (k_gram_bwd_sum) adds the partials of the chunks and tiles in index order: no atomics, two calls are bit-equal.
#include <hip/hip_runtime.h>
#include "mm_common.h"
#include "mm_gram.h"

#define MMG_XS (MMG_TN + 1)       /* row stride of xs and of the t tile: 129 doubles, consecutive rows two banks apart */
#define MMG_RED 512               /* >= MMG_TM * MM_DMAX (row, dimension) pairs */

static_assert(MMG_TM * MM_DMAX <= MMG_RED && MMG_THREADS <= MMG_RED, "pair buffers");
static_assert(MMG_THREADS == 2 * MMG_TN && MMG_RPT * 2 == MMG_TM, "entry phase: thread (c, h) owns MMG_RPT rows of one column");

// LDS, in doubles: il [MM_DMAX] | zs [d][MMG_TM] | xs [d][MMG_XS] ( | t [MMG_TM][MMG_XS] | redz [MMG_RED] | redl [MMG_RED] )
static inline size_t mmg_lds_bytes(int d, bool backward) {
  size_t n = MM_DMAX + (size_t)d * MMG_TM + (size_t)d * MMG_XS;
  if (backward) n += (size_t)MMG_TM * MMG_XS + 2 * MMG_RED;
  return n * sizeof(double);
}

// the operands of tile (m0, n0) of latent l into LDS (zero beyond M and N); Xp == Zl in self mode
__device__ __forceinline__ void mmg_stage(int M, int N, int d, int m0, int n0, const double* __restrict__ Xp,
                                          const double* __restrict__ Zl, const double* __restrict__ lsl, double* il, double* zs,
                                          double* xs) {
  const int tid = (int)threadIdx.x;
  if (tid < d) il[tid] = 1.0 / lsl[tid];
  for (int idx = tid; idx < MMG_TM * d; idx += MMG_THREADS) {
    const int r = idx / d, k = idx - r * d, m = m0 + r;
    zs[k * MMG_TM + r] = m < M ? Zl[(size_t)m * d + k] : 0.0;
  }
  for (int idx = tid; idx < MMG_TN * d; idx += MMG_THREADS) {       // the chunk's rows of X are one contiguous range
    const int c = idx / d, k = idx - c * d, n = n0 + c;
    xs[k * MMG_XS + c] = n < N ? Xp[(size_t)n * d + k] : 0.0;
  }
}

// e[r] = exp(-1/2 |(x_c - z_{8 h + r}) / l|^2), r < MMG_RPT
__device__ __forceinline__ void mmg_entries(int d, const double* il, const double* zs, const double* xs, int c, int h,
                                            double (&e)[MMG_RPT]) {
  double acc[MMG_RPT];
#pragma unroll
  for (int r = 0; r < MMG_RPT; ++r) acc[r] = 0.0;
  for (int k = 0; k < d; ++k) {
    const double xk = xs[k * MMG_XS + c], ilk = il[k];
    const double* zk = zs + k * MMG_TM + h * MMG_RPT;
#pragma unroll
    for (int r = 0; r < MMG_RPT; ++r) acc[r] = mmg_sq_acc(xk, zk[r], ilk, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < MMG_RPT; ++r) e[r] = mmg_profile(acc[r]);
}

__global__ __launch_bounds__(MMG_THREADS) void k_gram_se(int M, int N, int d, const double* __restrict__ X,
                                                         const double* __restrict__ Z, const double* __restrict__ ls,
                                                         const double* __restrict__ var, double* __restrict__ K) {
  extern __shared__ double mmg_sm[];
  double* il = mmg_sm;
  double* zs = il + MM_DMAX;
  double* xs = zs + d * MMG_TM;
  const int l = (int)blockIdx.z, m0 = (int)blockIdx.y * MMG_TM, n0 = (int)blockIdx.x * MMG_TN;
  const double* Zl = Z + (size_t)l * M * d;
  mmg_stage(M, N, d, m0, n0, X ? X : Zl, Zl, ls + (size_t)l * d, il, zs, xs);
  __syncthreads();
  const int c = (int)threadIdx.x & (MMG_TN - 1), h = (int)threadIdx.x / MMG_TN, n = n0 + c;
  double e[MMG_RPT];
  mmg_entries(d, il, zs, xs, c, h, e);
  const double v = var[l];
  if (n < N) {
#pragma unroll
    for (int r = 0; r < MMG_RPT; ++r) {
      const int m = m0 + h * MMG_RPT + r;
      if (m < M) K[((size_t)l * M + m) * N + n] = v * e[r];
    }
  }
}

// self != 0: X is Z_l (N == M), G a general [M, M] matrix: t = (G_mn + G_nm) K_mn carries both argument slots into gZ, half of it
// goes into gls; gvar needs G alone
__global__ __launch_bounds__(MMG_THREADS) void k_gram_se_bwd(int M, int N, int d, int self, const double* __restrict__ G,
                                                             const double* __restrict__ X, const double* __restrict__ Z,
                                                             const double* __restrict__ ls, const double* __restrict__ var,
                                                             double* __restrict__ wsZ, double* __restrict__ wsL,
                                                             double* __restrict__ wsV) {
  extern __shared__ double mmg_sm[];
  double* il = mmg_sm;
  double* zs = il + MM_DMAX;
  double* xs = zs + d * MMG_TM;
  double* tt = xs + d * MMG_XS;
  double* redz = tt + MMG_TM * MMG_XS;
  double* redl = redz + MMG_RED;
  const int tid = (int)threadIdx.x;
  const int l = (int)blockIdx.z, rt = (int)blockIdx.y, ch = (int)blockIdx.x, m0 = rt * MMG_TM, n0 = ch * MMG_TN;
  const int nch = (int)gridDim.x, nrt = (int)gridDim.y;
  const double* Zl = Z + (size_t)l * M * d;
  const double* Gl = G + (size_t)l * M * N;
  mmg_stage(M, N, d, m0, n0, self ? Zl : X, Zl, ls + (size_t)l * d, il, zs, xs);
  if (self) {
    // G^T's tile: 16 consecutive lanes read the 16 consecutive entries m0 .. m0 + 15 of row n
    for (int idx = tid; idx < MMG_TM * MMG_TN; idx += MMG_THREADS) {
      const int r = idx & (MMG_TM - 1), c = idx / MMG_TM, m = m0 + r, n = n0 + c;
      tt[r * MMG_XS + c] = (m < M && n < N) ? Gl[(size_t)n * M + m] : 0.0;
    }
  }
  __syncthreads();
  const int c = tid & (MMG_TN - 1), h = tid / MMG_TN, n = n0 + c;
  double e[MMG_RPT];
  mmg_entries(d, il, zs, xs, c, h, e);
  const double v = var[l];
  double gv = 0.0;
#pragma unroll
  for (int r = 0; r < MMG_RPT; ++r) {
    const int rr = h * MMG_RPT + r, m = m0 + rr;
    double g = 0.0;
    if (m < M && n < N) g = Gl[(size_t)m * N + n];
    gv = fma(g, e[r], gv);
    const double gs = self ? g + tt[rr * MMG_XS + c] : g;
    tt[rr * MMG_XS + c] = gs * (v * e[r]);
  }
  // gvar of the tile: the threads' sums in a fixed order
  redz[tid] = gv;
  __syncthreads();
  if (tid < 16) {
    double s = 0.0;
    for (int j = 0; j < MMG_THREADS / 16; ++j) s += redz[tid * (MMG_THREADS / 16) + j];
    redl[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += redl[j];
    wsV[((size_t)l * nrt + rt) * nch + ch] = s;
  }
  __syncthreads();
  // (row, dimension) pairs: p = r d + k; S column slices per pair when the pairs leave threads idle
  const int P = MMG_TM * d, S = P >= MMG_THREADS ? 1 : MMG_THREADS / P, W = P * S;
  const int ncols = N - n0 < MMG_TN ? N - n0 : MMG_TN;
  for (int w = tid; w < W; w += MMG_THREADS) {
    const int s = w / P, p = w - s * P, r = p / d, k = p - r * d;
    const double z = zs[k * MMG_TM + r];
    double az = 0.0, al = 0.0;
    for (int j = s; j < ncols; j += S) mmg_adj_acc(tt[r * MMG_XS + j], xs[k * MMG_XS + j], z, az, al);
    redz[w] = az;
    redl[w] = al;
  }
  __syncthreads();                       // the t tile is dead from here: its space takes the pairs' gls sums
  for (int p = tid; p < P; p += MMG_THREADS) {
    double az = 0.0, al = 0.0;
    for (int s = 0; s < S; ++s) { az += redz[s * P + p]; al += redl[s * P + p]; }
    const int r = p / d, k = p - r * d, m = m0 + r;
    if (m < M) wsZ[(((size_t)l * nch + ch) * M + m) * d + k] = mmg_gz_scale(az, il[k]);
    tt[p] = al;
  }
  __syncthreads();
  if (tid < d) {
    double s = 0.0;
    for (int r = 0; r < MMG_TM; ++r) s += tt[r * d + tid];           // rows beyond M hold zeros
    wsL[(((size_t)l * nrt + rt) * nch + ch) * d + tid] = (self ? 0.5 : 1.0) * mmg_gl_scale(s, il[tid]);
  }
}

// the partials of the chunks (gZ) and of the tiles and chunks (gls, gvar), added in index order: one thread per output
__global__ __launch_bounds__(MMG_THREADS) void k_gram_bwd_sum(int L, int M, int d, int nch, int nrt, const double* __restrict__ wsZ,
                                                              const double* __restrict__ wsL, const double* __restrict__ wsV,
                                                              double* __restrict__ gZ, double* __restrict__ gls,
                                                              double* __restrict__ gvar) {
  const size_t md = (size_t)M * d, nz = (size_t)L * md, nl = (size_t)L * d, nb = (size_t)nrt * nch;
  size_t i = (size_t)blockIdx.x * MMG_THREADS + threadIdx.x;
  double s = 0.0;
  if (i < nz) {
    const size_t l = i / md, rem = i - l * md;
    for (int c = 0; c < nch; ++c) s += wsZ[(l * nch + c) * md + rem];
    gZ[i] = s;
    return;
  }
  i -= nz;
  if (i < nl) {
    const size_t l = i / d, k = i - l * d;
    for (size_t j = 0; j < nb; ++j) s += wsL[(l * nb + j) * d + k];
    gls[i] = s;
    return;
  }
  i -= nl;
  if (i < (size_t)L) {
    for (size_t j = 0; j < nb; ++j) s += wsV[i * nb + j];
    gvar[i] = s;
  }
}

static int mmg_check_dims(int L, int M, int N, int d) {
  if (L <= 0 || M <= 0 || N <= 0 || d <= 0 || d > MM_DMAX) return MM_E_DIM;
  if (L > 65535 || mmg_tiles(M) > 65535) return MM_E_DIM;          // grid y, z
  return 0;
}

extern "C" size_t mm_gram_workspace_bytes(int L, int M, int N, int d) {
  if (mmg_check_dims(L, M, N, d)) return 0;
  return mm_align_up(mmg_workspace(L, M, N, d).total * sizeof(double), 256);
}

extern "C" int mm_gram_se(int L, int M, int N, int d, const double* X, const double* Z, const double* ls, const double* var,
                          double* K, void* stream) {
  if (int rc = mmg_check_dims(L, M, N, d)) return rc;
  if (!Z || !ls || !var || !K) return MM_E_ARG;
  if (!X && N != M) return MM_E_ARG;                                // self mode: K is [L, M, M]
  k_gram_se<<<dim3(mmg_chunks(N), mmg_tiles(M), L), MMG_THREADS, mmg_lds_bytes(d, false), (hipStream_t)stream>>>(M, N, d, X, Z, ls,
                                                                                                                   var, K);
  return (int)hipGetLastError();
}

extern "C" int mm_gram_se_backward(int L, int M, int N, int d, const double* G, const double* X, const double* Z, const double* ls,
                                   const double* var, double* gZ, double* gls, double* gvar, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (int rc = mmg_check_dims(L, M, N, d)) return rc;
  if (!G || !Z || !ls || !var || !gZ || !gls || !gvar || !workspace) return MM_E_ARG;
  if (!X && N != M) return MM_E_ARG;
  const MMGramWs w = mmg_workspace(L, M, N, d);
  if (workspace_bytes < w.total * sizeof(double)) return MM_E_WORKSPACE;
  double* ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int nch = mmg_chunks(N), nrt = mmg_tiles(M);
  k_gram_se_bwd<<<dim3(nch, nrt, L), MMG_THREADS, mmg_lds_bytes(d, true), s>>>(M, N, d, X ? 0 : 1, G, X, Z, ls, var, ws + w.gz,
                                                                              ws + w.gl, ws + w.gv);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const size_t nout = (size_t)L * M * d + (size_t)L * d + (size_t)L;
  k_gram_bwd_sum<<<(unsigned)((nout + MMG_THREADS - 1) / MMG_THREADS), MMG_THREADS, 0, s>>>(L, M, d, nch, nrt, ws + w.gz, ws + w.gl,
                                                                                           ws + w.gv, gZ, gls, gvar);
  return (int)hipGetLastError();
}
