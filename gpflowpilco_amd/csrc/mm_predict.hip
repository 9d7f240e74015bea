// Predictive mean and variance of SE-ARD latents at N deterministic points (models.SVGP.predict_f / GPR.predict_f through
// ops.predict_se); f64.  From beta = Kuu^-1 u and the symmetric C = Kuu^-1 (S - Kuu) Kuu^-1 of `precompute`:
//
//   mean[n][l] = sum_m K_l[m][n] beta_l[m] (+ mean_c[l]),      fvar[n][l] = var_l + sum_ij K_l[i][n] C_l[i][j] K_l[j][n]
//
// A persistent grid of at most MMP_GRID_CAP workgroups walks the work items (latent l, tile of MMP_TN = 64 points) in index order;
// the schedule of one item is mm_predict.h's.  Phase 1 stages the tile's points and, block by block, the inducing points in LDS,
// forms the entries of K from differences (mm_gram.h), adds the mean in registers and leaves the K strip [blocks * 64][64] in the
// workgroup's own slice of the workspace (the only buffer; nothing is proportional to N).  Phase 2 visits the blocks (ib, jb <= ib)
// of C: the 64 x 64 block of C and the 64 x 64 tile of K go through LDS (the next pair's global loads are in flight during the
// matrix instructions), wave w owns rows 16 w .. 16 w + 15 of the block and all 64 points, 4 accumulators of
// v_mfma_f64_16x16x4_f64.  At the diagonal block the row's accumulator is doubled first (the off-diagonal blocks stand for their
// mirror images), and after it the K tile still in LDS multiplies the accumulator: the epilogue of row ib, added to per-lane sums
// in a fixed order.  The 16 partial sums of a point (4 waves x 4 row groups) are added in index order: no atomics, two calls are
// bit-equal.
#include <hip/hip_runtime.h>
#include <atomic>
#include "mm_common.h"
#include "mm_predict.h"

typedef double f64x4p __attribute__((ext_vector_type(4)));

#define MMP_CS 66        /* row stride of the C block in LDS: lanes (row l15, k kq) of an A operand fall in distinct banks */
#define MMP_KS 80        /* row stride of the K tile: lanes (k kq, column l15) of a B operand likewise */
#define MMP_LDS_DOUBLES (MMP_B * MMP_CS + MMP_B * MMP_KS)

static_assert(MMP_B == 64 && MMP_TN == 64 && MMP_THREADS == 256, "4 waves x 16 rows; thread (c, h) of phase 1 owns 16 rows of point c");
static_assert(MM_DMAX + 2 * MM_DMAX * 64 <= MMP_B * MMP_CS, "phase 1 stages il, xs and zs in the C block's space");
static_assert(16 * MMP_TN <= MMP_B * MMP_CS && 4 * MMP_TN <= MMP_B * MMP_KS, "reduction buffers");

// (two workgroups per CU by LDS: at most 256 registers a lane)
__global__ __launch_bounds__(MMP_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_predict_se(
    int L, int M, int N, int d, const double* __restrict__ X, const double* __restrict__ Z, const double* __restrict__ ls,
    const double* __restrict__ var, const double* __restrict__ beta, const double* __restrict__ C,
    const double* __restrict__ mean_c, double* __restrict__ mean, double* __restrict__ fvar, double* __restrict__ ws) {
  extern __shared__ double mmp_sm[];
  double* Cs = mmp_sm;                       // phase 2: block of C; phase 1: il | xs [d][64] | zs [d][64]; end of item: 16 x 64 sums
  double* Ks = mmp_sm + MMP_B * MMP_CS;      // phase 2: tile of K; phase 1: 4 x 64 sums of the mean
  double* il = Cs;
  double* xs = Cs + MM_DMAX;
  double* zs = xs + d * MMP_TN;
  const int tid = (int)threadIdx.x;
  const int c = tid & (MMP_TN - 1), h = tid >> 6;                 // phase 1: point c, rows 16 h .. 16 h + 15 of a block
  const int l15 = tid & 15, kq = (tid >> 4) & 3, wv = tid >> 6;   // phase 2: the lane's place in the matrix instruction
  const int nb = mmp_blocks(M), tiles = mmp_tiles(N);
  const long long items = mmp_items(L, N);
  double* strip = ws + (size_t)blockIdx.x * mmp_strip(M);

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int l = (int)(item / tiles), t = (int)(item - (long long)l * tiles);
    const long long n0 = (long long)t * MMP_TN;
    const double* Zl = Z + (size_t)l * M * d;
    const double* bl = beta + (size_t)l * M;
    const double v = var[l];
    // ---- phase 1: the K strip and the mean ----
    if (tid < d) il[tid] = 1.0 / ls[(size_t)l * d + tid];
    for (int idx = tid; idx < MMP_TN * d; idx += MMP_THREADS) {         // the tile's rows of X are one contiguous range
      const int cc = idx / d, k = idx - cc * d;
      xs[k * MMP_TN + cc] = mmp_col_valid(N, t, cc) ? X[(size_t)(n0 + cc) * d + k] : 0.0;
    }
    const bool col_ok = mmp_col_valid(N, t, c);
    double msum = 0.0;
    for (int jb = 0; jb < nb; ++jb) {
      __syncthreads();                                                  // the previous block's zs has been read
      for (int idx = tid; idx < MMP_B * d; idx += MMP_THREADS) {
        const int r = idx / d, k = idx - r * d;
        zs[k * MMP_B + r] = mmp_row_valid(M, jb, r) ? Zl[((size_t)jb * MMP_B + r) * d + k] : 0.0;
      }
      __syncthreads();
      for (int q = 0; q < 4; ++q) {                                     // 4 rows at a time: 16 h + 4 q + r
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < d; ++k) {
          const double xk = xs[k * MMP_TN + c], ilk = il[k];
          const double* zk = zs + k * MMP_B + h * 16 + q * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = mmg_sq_acc(xk, zk[r], ilk, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rr = h * 16 + q * 4 + r;
          const bool row_ok = mmp_row_valid(M, jb, rr);
          const double kv = (col_ok && row_ok) ? v * mmg_profile(acc[r]) : 0.0;
          const double b = row_ok ? bl[jb * MMP_B + rr] : 0.0;
          msum = fma(kv, b, msum);
          if (C) strip[((size_t)jb * MMP_B + rr) * MMP_TN + c] = kv;
        }
      }
    }
    Ks[h * MMP_TN + c] = msum;
    __syncthreads();                            // ... and the strip is visible to the workgroup; xs, zs and il are dead
    if (tid < MMP_TN && col_ok) {
      double s = Ks[c];
      for (int j = 1; j < 4; ++j) s += Ks[j * MMP_TN + c];
      mean[(size_t)(n0 + c) * L + l] = mean_c ? s + mean_c[l] : s;
    }
    if (!C) { __syncthreads(); continue; }
    // ---- phase 2: the blocks (ib, jb <= ib) of C against the strip ----
    const double* Cl = C + (size_t)l * M * M;
    double rc[16];
    double rk[16];
    auto load_regs = [&](MMPBlock b) {
      // element e = 256 i + tid of the block: row 4 i + (tid >> 6), column tid & 63 -- consecutive lanes on consecutive columns
      const int r0 = tid >> 6, cc = tid & 63;
      const bool cc_ok = mmp_row_valid(M, b.jb, cc);
      const double* cp = Cl + ((size_t)b.ib * MMP_B + r0) * M + (size_t)b.jb * MMP_B + cc;
#pragma unroll
      for (int i = 0; i < 16; ++i) rc[i] = (cc_ok && mmp_row_valid(M, b.ib, 4 * i + r0)) ? cp[(size_t)(4 * i) * M] : 0.0;
      const double2* kp = reinterpret_cast<const double2*>(strip + (size_t)b.jb * MMP_B * MMP_TN);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const double2 k2 = kp[i * MMP_THREADS + tid];
        rk[2 * i] = k2.x;
        rk[2 * i + 1] = k2.y;
      }
    };
    f64x4p acc[4];
    double vs[4] = {0.0, 0.0, 0.0, 0.0};
    MMPBlock blk = mmp_first();
    load_regs(blk);
    while (!mmp_done(blk, M)) {
      __syncthreads();                          // the previous pair's operands (and the mean's sums) have been read
#pragma unroll
      for (int i = 0; i < 16; ++i) Cs[(4 * i + (tid >> 6)) * MMP_CS + (tid & 63)] = rc[i];
#pragma unroll
      for (int i = 0; i < 8; ++i)               // double2 e = 256 i + tid of the tile: row 8 i + (tid >> 5), columns 2 (tid & 31), + 1
        *reinterpret_cast<double2*>(&Ks[(8 * i + (tid >> 5)) * MMP_KS + 2 * (tid & 31)]) = make_double2(rk[2 * i], rk[2 * i + 1]);
      __syncthreads();
      const MMPBlock nxt = mmp_next(blk);
      if (!mmp_done(nxt, M)) load_regs(nxt);    // in flight during the matrix instructions
      if (blk.jb == 0) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = (f64x4p){0.0, 0.0, 0.0, 0.0};
      }
      const double scale = mmp_row_scale(blk);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] *= scale;
      // (a block that M cuts multiplies its zero columns too: one code path, a constant trip count)
#pragma unroll 4
      for (int s = 0; s < MMP_B / 4; ++s) {
        const double a = Cs[(wv * 16 + l15) * MMP_CS + 4 * s + kq];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ks[(4 * s + kq) * MMP_KS + ct * 16 + l15], acc[ct], 0, 0, 0);
      }
      if (mmp_is_diagonal(blk)) {
        // accumulator: lane (l15 = point, kq), register r <-> row kq + 4 r of the wave's 16; the K tile in LDS is row ib's
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) vs[ct] = fma(Ks[(wv * 16 + kq + 4 * r) * MMP_KS + ct * 16 + l15], acc[ct][r], vs[ct]);
      }
      blk = nxt;
    }
    __syncthreads();                            // the last operands have been read: their space takes the 16 sums per point
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) Cs[(wv * 4 + kq) * MMP_TN + ct * 16 + l15] = vs[ct];
    __syncthreads();
    if (tid < MMP_TN && col_ok) {
      double s = Cs[c];
      for (int j = 1; j < 16; ++j) s += Cs[j * MMP_TN + c];
      fvar[(size_t)(n0 + c) * L + l] = v + s;
    }
    __syncthreads();                            // before the next item stages over the sums and rewrites the strip
  }
}

static int mmp_check_dims(int L, int M, int N, int d) {
  if (L <= 0 || M <= 0 || N <= 0 || d <= 0 || d > MM_DMAX) return MM_E_DIM;
  if (M > MMP_M_MAX || mmp_items(L, N) > 0x7fffffffLL) return MM_E_DIM;
  return 0;
}

extern "C" size_t mm_predict_workspace_bytes(int L, int M, int N, int d) {
  if (mmp_check_dims(L, M, N, d)) return 0;
  return mm_align_up((size_t)MMP_GRID_CAP * mmp_strip(M) * sizeof(double), 256);      // one strip per workgroup of the capped grid
}

// hipFuncAttributeMaxDynamicSharedMemorySize once per device (a bitmap over the device ordinals; devices >= 64 set it every call)
static hipError_t mmp_set_max_lds_once(int bytes) {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
  e = hipFuncSetAttribute((const void*)k_predict_se, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && bit) done.fetch_or(bit, std::memory_order_release);
  return e;
}

extern "C" int mm_predict_se(int L, int M, int N, int d, const double* X, const double* Z, const double* ls, const double* var,
                             const double* beta, const double* C, const double* mean_c, double* mean, double* fvar,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = mmp_check_dims(L, M, N, d)) return rc;
  if (!X || !Z || !ls || !var || !beta || !mean || !workspace) return MM_E_ARG;
  if ((C == nullptr) != (fvar == nullptr)) return MM_E_ARG;
  if (workspace_bytes < (size_t)MMP_GRID_CAP * mmp_strip(M) * sizeof(double)) return MM_E_WORKSPACE;
  const int lds = MMP_LDS_DOUBLES * (int)sizeof(double);
  if (hipError_t e = mmp_set_max_lds_once(lds)) return (int)e;
  k_predict_se<<<mmp_grid(L, N), MMP_THREADS, lds, (hipStream_t)stream>>>(L, M, N, d, X, Z, ls, var, beta, C, mean_c, mean, fvar,
                                                                         (double*)workspace);
  return (int)hipGetLastError();
}
