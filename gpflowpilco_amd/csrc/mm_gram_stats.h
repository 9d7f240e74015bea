// Schedule of the streamed Gram statistics of the collapsed (SGPR) bound and of their adjoint (mm_gram_stats.hip; f64):
//
//   Phi_l = K_l K_l^T [M, M],   Psi_l = K_l R [M, Q],   K_l[m][n] = var_l exp(-1/2 |(x_n - z_lm) / ls_l|^2)   (mm_gram.h's entries)
//   G_K   = (GPhi + GPhi^T) K + GPsi R^T,   t = G_K o K,   gZ, gls as mm_gram.h,   gvar = sum t / var
//
// Written once for the device kernels and for the one-thread CPU build that tests/test_gram_stats_host.py checks against torch
// (tests/hostcheck/mm_gram_stats_host.hip): the host side walks the same items, blocks, chunks and splits with scalar fma for the
// matrix instruction and std::exp for mm_exp_f64.  Nothing here or in the kernels has a size proportional to L M N.
//
// Forward.  The M inducing points are cut into blocks of MGS_B, the N points into chunks of MGS_TN.  One work item is (latent l,
// block pair (ib, jb <= ib) of Phi, split s of the chunks): it forms, chunk by chunk, the two K tiles from differences and adds
// their product to its 64 x 64 partial of Phi; the items with jb == 0 also add K[ib] R to their partial of Psi.  A second launch adds
// the partials of the splits in index order and mirrors the lower triangle (diagonal blocks included, so that Phi is symmetric to
// the bit).  The number of splits fills the machine at small M and does not depend on N beyond being at most the chunk count.
//
// Adjoint.  mgs_bwd_groups(L) workgroups per latent walk that latent's chunks (chunk c of group w: c = w, w + groups, ...).  A
// workgroup forms the chunk's K strip [blocks * 64][64] in its own workspace slice, then per row block ib the 64 x 64 tile
// acc = sum_jb Gs[ib][jb] K[jb] + GPsi[ib] R^T, t = acc o K[ib], and mm_gram.h's sums over the chunk's columns in index order,
// added to the workgroup's own partial slice; a last launch adds the slices in index order.
#pragma once
#include "mm_gram.h"

#define MGS_B 64                 /* rows and columns of a block of Phi */
#define MGS_TN 64                /* points of a chunk */
#define MGS_THREADS 256
#define MGS_QMAX 33              /* columns of R: at most MM_DMAX outputs and the column of ones */
#define MGS_FWD_TARGET 512       /* forward work items aimed at when the block pairs alone are fewer (two per compute unit) */
#define MGS_BWD_CAP 512          /* workgroups of the adjoint's grid over all latents (each owns a K strip and a partial slice) */
#define MGS_M_MAX (1 << 15)

MMG_FN int mgs_blocks(int M) { return (M + MGS_B - 1) / MGS_B; }
MMG_FN int mgs_chunks(int N) { return (N + MGS_TN - 1) / MGS_TN; }
MMG_FN long long mgs_pairs(int M) { const long long nb = mgs_blocks(M); return nb * (nb + 1) / 2; }
// pair index p = ib (ib + 1) / 2 + jb  <->  (ib, jb <= ib)
MMG_FN void mgs_pair_blocks(long long p, int& ib, int& jb) {
  int i = 0;
  while ((long long)(i + 1) * (i + 2) / 2 <= p) ++i;
  ib = i;
  jb = (int)(p - (long long)i * (i + 1) / 2);
}
MMG_FN long long mgs_pair_index(int ib, int jb) { return (long long)ib * (ib + 1) / 2 + jb; }

// splits the workspace is sized for: a function of (L, M) alone
MMG_FN int mgs_splits_max(int L, int M) {
  const long long lp = (long long)L * mgs_pairs(M);
  return lp >= MGS_FWD_TARGET ? 1 : (int)((MGS_FWD_TARGET + lp - 1) / lp);
}
// chunks per split and the splits in use (no split is empty)
MMG_FN int mgs_chunks_per_split(int L, int M, int N) {
  const int nch = mgs_chunks(N), s0 = mgs_splits_max(L, M);
  return (nch + s0 - 1) / s0;
}
MMG_FN int mgs_splits(int L, int M, int N) {
  const int cps = mgs_chunks_per_split(L, M, N);
  return (mgs_chunks(N) + cps - 1) / cps;
}
MMG_FN bool mgs_row_valid(int M, int b, int r) { return b * MGS_B + r < M; }
MMG_FN bool mgs_col_valid(int N, int c, int j) { return (long long)c * MGS_TN + j < N; }

// workgroups per latent of the adjoint: the workspace is sized by mgs_bwd_groups_max, the launch uses at most the chunk count
MMG_FN int mgs_bwd_groups_max(int L) { return L >= MGS_BWD_CAP ? 1 : MGS_BWD_CAP / L; }
MMG_FN int mgs_bwd_groups(int L, int N) { const int g = mgs_bwd_groups_max(L), c = mgs_chunks(N); return c < g ? c : g; }
MMG_FN size_t mgs_strip(int M) { return (size_t)mgs_blocks(M) * MGS_B * MGS_TN; }
// doubles of one workgroup's partial slice of the adjoint: [M][d] sums of gZ | [d] of gls | 1 of gvar
MMG_FN size_t mgs_slice(int M, int d) { return (size_t)M * d + d + 1; }

// workspace, in doubles.  Forward: [L][pairs][splits][64][64] partials of Phi | [L][blocks][splits][64][Q] partials of Psi.
// Adjoint: [L][M][M] symmetrised GPhi | [L][groups] K strips | [L][groups] partial slices.  One buffer serves both.
struct MGSWs { size_t phi, psi, fwd_total, gs, strips, slices, bwd_total, total; };
static inline MGSWs mgs_workspace(int L, int M, int d, int Q) {
  const size_t s0 = (size_t)mgs_splits_max(L, M), g0 = (size_t)mgs_bwd_groups_max(L);
  MGSWs w;
  w.phi = 0;
  w.psi = w.phi + (size_t)L * (size_t)mgs_pairs(M) * s0 * MGS_B * MGS_B;
  w.fwd_total = w.psi + (size_t)L * mgs_blocks(M) * s0 * MGS_B * (size_t)Q;
  w.gs = 0;
  w.strips = w.gs + (size_t)L * M * M;
  w.slices = w.strips + (size_t)L * g0 * mgs_strip(M);
  w.bwd_total = w.slices + (size_t)L * g0 * mgs_slice(M, d);
  w.total = w.fwd_total > w.bwd_total ? w.fwd_total : w.bwd_total;
  return w;
}
