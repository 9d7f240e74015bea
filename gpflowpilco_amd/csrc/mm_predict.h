// Block schedule of the fused predictive mean and variance (mm_predict.hip; f64):
//
//   mean[n][l] = sum_m K_l[m][n] beta_l[m] (+ mean_c[l]),      fvar[n][l] = var_l + sum_ij K_l[i][n] C_l[i][j] K_l[j][n],   C_l symmetric
//
// Written once for the device kernel and for the one-thread CPU build that tests/test_predict_host.py checks against torch
// (tests/hostcheck/mm_predict_host.hip): the host side walks the same blocks in the same order with scalar fma for the matrix
// instruction and std::exp for mm_exp_f64 (mm_gram.h's entry arithmetic on both sides).
//
// One work item is (latent l, tile of MMP_TN points).  The M inducing points are cut into blocks of MMP_B.  The item first forms its
// K strip [blocks * MMP_B][MMP_TN] (rows past M and columns past N masked to zero) and the mean from it, then visits the blocks
// (ib, jb) of C with jb <= ib, row by row:
//
//   acc_ib = 0;   jb < ib : acc_ib += C[ib][jb] K[jb]        (an off-diagonal block, standing for its mirror image too: weight 2)
//                 jb == ib: acc_ib  = 2 acc_ib + C[ib][ib] K[ib]                          (the weight, applied once per row, exact)
//   fvar_part += sum_i K[ib][i][n] acc_ib[i][n]                                            (the epilogue of row ib, i ascending)
//
// so the blocks above the diagonal are never read: M (M + 1) multiply-adds per point and latent for the quadratic form instead of
// 2 M^2, and nothing of size M x N exists outside the strip of the item in flight.
#pragma once
#include "mm_gram.h"

#define MMP_B 64                 /* rows and columns of a block of C */
#define MMP_TN 64                /* points of a work item */
#define MMP_THREADS 256
#define MMP_GRID_CAP 512         /* workgroups of the persistent grid: each owns one K strip in the workspace */
#define MMP_M_MAX (1 << 20)

struct MMPBlock { int ib, jb; };

MMG_FN int mmp_blocks(int M) { return (M + MMP_B - 1) / MMP_B; }
MMG_FN int mmp_tiles(int N) { return (N + MMP_TN - 1) / MMP_TN; }
// the walk over the visited blocks: (0,0), (1,0), (1,1), (2,0), ...
MMG_FN MMPBlock mmp_first() { MMPBlock b; b.ib = 0; b.jb = 0; return b; }
MMG_FN MMPBlock mmp_next(MMPBlock b) {
  if (b.jb == b.ib) { b.ib += 1; b.jb = 0; } else { b.jb += 1; }
  return b;
}
MMG_FN bool mmp_done(MMPBlock b, int M) { return b.ib >= mmp_blocks(M); }
MMG_FN bool mmp_is_diagonal(MMPBlock b) { return b.jb == b.ib; }
// weight of a visited block in the quadratic form
MMG_FN double mmp_weight(MMPBlock b) { return mmp_is_diagonal(b) ? 1.0 : 2.0; }
// ... applied as one scaling of the row's accumulator when the walk reaches the diagonal block (every block before it in the row
// is an off-diagonal one)
MMG_FN double mmp_row_scale(MMPBlock b) { return mmp_is_diagonal(b) ? 2.0 : 1.0; }
// masks: row r of block b lies inside M; point c of tile t inside N
MMG_FN bool mmp_row_valid(int M, int b, int r) { return b * MMP_B + r < M; }
MMG_FN bool mmp_col_valid(int N, int t, int c) { return (long long)t * MMP_TN + c < N; }

// work items and the grid that walks them (item = l * tiles + t: workgroups in flight share a latent's blocks of C)
MMG_FN long long mmp_items(int L, int N) { return (long long)L * mmp_tiles(N); }
static inline int mmp_grid(int L, int N) { const long long it = mmp_items(L, N); return it < MMP_GRID_CAP ? (int)it : MMP_GRID_CAP; }
// doubles of one workgroup's K strip
MMG_FN size_t mmp_strip(int M) { return (size_t)mmp_blocks(M) * MMP_B * MMP_TN; }
