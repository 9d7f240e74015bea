// f32 MFMA fused reduce of the off-diagonal kernel pairs (a < a') on gfx950.
//
// For every (b, pair) the reference's eKuffu slice Q_aa' (utils/kernel_expectation.py:72-187, then
// models.py:219-248) is never stored; with b_ij = A_i . zc_j, what_i = w_i e^{rho'_i}, what'_j = w'_j e^{gamma_j}
//     S = sum_ij w_i expm1(delta_ij) w'_j,   delta_ij = rho'_i + gamma_j + b_ij
//       = sum_ij what_i what'_j (1 + b_ij + b_ij^2/2)  - (sum w)(sum w')        exact, f64 moments (O(M d^2))
//       + sum_ij what_i what'_j r(b_ij),   r(x) = expm1(x) - x - x^2/2            THIS kernel, f32, O(M^2)
// Where the model's input dimension allows the moment tables (d <= 8) and a (b, pair)'s Cauchy-Schwarz bound on |b_ij| is
// <= 1/2 (MM_COLLAPSE_BOUND2: nearly all of its tiles are then inside 1/4), the (b, pair) is COLLAPSED (mm_common.h,
// mm_moments.hip, mm_moments6.hip): p6(x) = x^3 (C0 + .. + C3 x^3) -- this kernel's own degree-3 tier, |p6 - r| <= 5.8e-10 on
// |x| <= 1/4 -- is taken from weight moments as well, every wave tile whose max|b| is inside 1/4 (known after ONE screening
// MFMA per 32 x 32 block, the (h, h + m) part of the split product) contributes nothing and is skipped, and the other tiles
// reduce the correction r(x) - p6(x) with the same range tiers.
// The bilinear part runs on the bf16 matrix pipe as a 3-way split product with f32 accuracy
// (v_mfma_f32_32x32x16_bf16), the remainder polynomial + weighted reduction on the VALU in packed
// f32 (v_pk_fma_f32); MFMA and f32 FMA-class VALU time add on a gfx950 SIMD (tools/ubench_overlap.hip).
//
// Work decomposition: workgroup = 4 waves = 256 rows of one (b, pair); a wave owns 64 rows
// (two 32x32 MFMA row tiles; split A operands, rho' (the MFMA C operand) and the 32 row weights
// stay in registers) and sweeps all columns in tiles of 32, software-prefetching the next
// tile's pre-split inducing inputs (two 16-B loads per lane) and gamma_j / w_j.  Partial sums
// are flushed to f64 once per column tile and written to a slab (no atomics: bitwise
// reproducible).  The 1-D grid is remapped so that the row panels of one (b, pair) land on the
// same XCD and share its L2.
// Where the whole column latent fits in LDS (d <= 8, Mp <= 2048) k_qred_f32_mfma_persist (below) takes over: a work list of the
// items with a tile to visit and one workgroup per CU with every column operand in LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "mm_common.h"
#include "mm_mono.h"
#include "mm_f32_tile.h"

__device__ __forceinline__ void mm_decode_pair_o(int p, int L, int& a, int& a2) {
  int r = p - L, i = 0;
  while (r >= L - 1 - i) { r -= L - 1 - i; ++i; }
  a = i; a2 = i + 1 + r;
}

// BOUND-BASED SKIPPING of a collapsed row group's column tiles.  For any positive scale vector s, |A_i . zc'_j| <= |A_i o s| |zc'_j / s|
// (Cauchy-Schwarz in the scaled metric).  With s = l_a' (the column latent's lengthscales) the column factor is the pack's sort key
// (MMModelLayout::zt2s per 32-column tile) and the row factor is MMWorkspaceLayout::gmax2s per 64-row group (k_pairvec_reg); with
// lengthscales spread over a decade |A_i| and |zc'_j| are dominated by different dimensions and the Euclidean product (gmax2 x zt2)
// is loose: on the BASELINE recipe at C3 it leaves 13 x the wave tiles to the screening product that the scaled one does
// (tools/pack_order_study.py section 4).  gmax2s == nullptr (d > 8 has no row groups; MM_ISTAGE_OLD_SKIP_BOUND): the Euclidean test.
// The collapse DECISION (gflag, amax, amaxc, gmax2, MM_COLLAPSE_BOUND2), thr_skip and the error estimate stay Euclidean.
//
// the largest zt2s of a latent (every lane of the wave calls; the result is wave-uniform)
__device__ __forceinline__ float mm_wave_max_tiles(const float* __restrict__ zt, int nct, int lane) {
  float m = 0.0f;
  for (int c = lane; c < nct; c += 64) m = fmaxf(m, zt[c]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  return m;
}
// group gi has no tile to visit: its bound with the latent's largest point is inside the collapsed range (zsmax: mm_wave_max_tiles
// of zt2s, read where gmax2s != nullptr only).  The same products, factor by factor, as the tile scan at ct_first: a group is
// inside exactly when that scan finds no tile (f32 multiplication by a2w >= 0 is monotone)
__device__ __forceinline__ bool mm_group_inside(const float* __restrict__ gmax2, const float* __restrict__ gmax2s, size_t gi,
                                                double zmax2a, float zsmax) {
  return gmax2s ? (gmax2s[gi] * 1.000001f) * zsmax <= MM_INSIDE_BOUND2
                : mm_collapse_bound2(__float_as_uint(gmax2[gi]), zmax2a) <= MM_INSIDE_BOUND2;
}

// largest tile range max|b| for which the 2-way (h + m) product is used without the (h,l)/(l,h) terms
// (measured at C3: 1/64, 1/32 and 1/16 all leave the Sff error at 3.5e-6; 1/32 keeps a factor 4 in hand)
#ifndef MM_TWO_WAY_MAX
#define MM_TWO_WAY_MAX 0.03125f
#endif
// LDS-staged sweep: workgroups per (b, pair), each paying the 64 KB fill for its share of the row panels.  Measured
// at C3 (off-diagonal segment, pilco / BASELINE recipe): 1 -> 0.574 / 6.66 ms, 2 -> 0.444 / 6.27, 4 -> 0.380 / 6.19,
// 8 -> 0.420 / 6.31: with most (b, pair) items leaving at once (wholly inside the collapsed range) the few that sweep
// are the grid's tail, and finer items balance it.  Round 5, with a workgroup's panels interleaved over the (norm-ordered) rows
// and the Cauchy-Schwarz skipping (BASELINE recipe): 1 -> 1.135, 2 -> 0.99, 4 -> 1.03, 8 -> 1.09 ms
#ifndef MM_F32_PPW_DIV
#define MM_F32_PPW_DIV 2
#endif
// 0: the sweep without its rounding-error estimate (A/B measurement of what the accuracy contract costs: nothing is ever routed)
#ifndef MM_ROUTE_EST
#define MM_ROUTE_EST 1
#endif
#ifndef MM_F32_WAVES
#define MM_F32_WAVES 2
#endif
// sum_r w_r * x_r^3 * R_DEG(x_r) over the 16 register pairs of a wave tile.  The Horner steps run
// "vertically" over the pairs so that consecutive v_pk_fma_f32 are independent.
// CC: the (b, pair) is collapsed -- its moments already carry p6 = x^3 (C0 + C1 x + C2 x^2 + C3 x^3) (mm_common.h), which is
// subtracted from the four leading coefficients at compile time (the corrected polynomial costs no instruction; the
// differences are exact in f32: Sterbenz)
template <int DEG, int CC>
struct MMRemC {
  // CC: what the moments already carry for these rows -- 0: nothing beyond order 2; 1: p6 (a collapsed row group); 2: the cubic
  // term C0 x^3 alone (the other row groups of an item that has collapsed ones: mm_mono.h)
  static constexpr float get(int k) {
    const float c6[4] = {MM_C6_C0, MM_C6_C1, MM_C6_C2, MM_C6_C3};
    return MMRem<DEG>::c[k] - ((CC == 1 && k < 4) ? c6[k] : ((CC == 2 && k == 0) ? c6[0] : 0.0f));
  }
};
template <int DEG, int CC>
__device__ __forceinline__ f32x2 mm_weighted_rem(const f32x2 (&xx)[16], const f32x2 (&wrow)[2][8]) {
  f32x2 parts[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  // two halves of 8 register pairs (one 32-row MFMA tile each): 8 independent chains cover the packed-FMA latency,
  // and the temporaries of one half are dead before the other starts (register pressure)
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    f32x2 pp[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      pp[r] = mm_pkfma(MM_PK((MMRemC<DEG, CC>::get(DEG))), xx[8 * hh + r], MM_PK((MMRemC<DEG, CC>::get(DEG - 1))));
#pragma unroll
    for (int k = DEG - 2; k >= 0; --k)
#pragma unroll
      for (int r = 0; r < 8; ++r)
        pp[r] = mm_pkfma(pp[r], xx[8 * hh + r], MM_PK((MMRemC<DEG, CC>::get(k))));
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const f32x2 wx = wrow[hh][r] * xx[8 * hh + r];                   // w_i * x
      const f32x2 tv = (xx[8 * hh + r] * xx[8 * hh + r]) * pp[r];      // x^2 * R(x)
      parts[r & 3] = mm_pkfma(tv, wx, parts[r & 3]);                   // += w_i * x^3 * R(x)
    }
  }
  return (parts[0] + parts[1]) + (parts[2] + parts[3]);
}

// First tier with the row weight folded into the two coefficients (w c0, w c1 kept per row):
//   w x^3 (c0 + c1 x) = (x^2 x) * fma(w c1, x, w c0):  four packed ops per entry pair instead of five.
__device__ __forceinline__ f32x2 mm_weighted_rem1(const f32x2 (&xx)[16], const f32x2 (&wc0)[2][8],
                                                  const f32x2 (&wc1)[2][8]) {
  f32x2 parts[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    f32x2 t3[8], rw[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) t3[r] = xx[8 * hh + r] * xx[8 * hh + r];
#pragma unroll
    for (int r = 0; r < 8; ++r) rw[r] = mm_pkfma(wc1[hh][r], xx[8 * hh + r], wc0[hh][r]);
#pragma unroll
    for (int r = 0; r < 8; ++r) t3[r] = t3[r] * xx[8 * hh + r];
#pragma unroll
    for (int r = 0; r < 8; ++r) parts[r & 3] = mm_pkfma(t3[r], rw[r], parts[r & 3]);
  }
  return (parts[0] + parts[1]) + (parts[2] + parts[3]);
}

// Where mm_f32_wave_rows reads a column tile's streaming operands: zA(ct, off, nb) / zB(ct, off, nb) are 16 bytes of tile ct's
// (m | h) / (l | h) parts at the lane's byte offset off inside the tile, 8-dimension block nb; wc(j) is what'_j.
// Every operand from LDS (k_qred_f32_mfma_persist, d <= 8) -- z: the column latent's [Mp/32][3 (h, m, l)][32][16] bf16 block, an exact
// copy of the packed model's (conflict-free ds_read_b128); w: the item's what'_j [Mp] f32
struct MMSrcLds {
  const char* z;
  const float* w;
  __device__ __forceinline__ u32x4 zA(int ct, unsigned int off, int nb) const {
    return *reinterpret_cast<const u32x4*>(z + (size_t)ct * 1536u + off + nb * 16);
  }
  __device__ __forceinline__ u32x4 zB(int ct, unsigned int off, int nb) const { return zA(ct, off, nb); }
  __device__ __forceinline__ float wc(int j) const { return w[j]; }
};
// k_qred_f32_mfma's -- zg: the packed model's [Mp/32][3 (h, m, l)][32][16 ND8] block of the column latent in L2; zl (LDSZ): the
// workgroup's LDS image of its (h, m) parts, [Mp/32][2][32][16 ND8], which serves zA; the (l | h) parts and w (what'_j) come from L2
template <int ND8, bool LDSZ>
struct MMSrcL2 {
  const char* zl;
  const char* zg;
  const float* w;
  __device__ __forceinline__ u32x4 zA(int ct, unsigned int off, int nb) const {
    if constexpr (LDSZ) return *reinterpret_cast<const u32x4*>(zl + (size_t)ct * (1024 * ND8) + off + nb * 16);
    else return zB(ct, off, nb);
  }
  __device__ __forceinline__ u32x4 zB(int ct, unsigned int off, int nb) const {
    return *reinterpret_cast<const u32x4*>(zg + (size_t)ct * (1536u * ND8) + off + nb * 16);
  }
  __device__ __forceinline__ float wc(int j) const { return w[j]; }
};
struct MMWaveSum { double sum; float est; };

// The per-wave code of both f32 off-diagonal sweeps (k_qred_f32_mfma, k_qred_f32_mfma_persist): ONE wave's 64 rows row0 .. row0 + 63
// of one (b, pair) against every column, the streaming operands read through src (above).  Returns the per-lane sum (f64) and error
// estimate of the wave, before the cross-lane reduction.  Both kernels run these tiles, tiers, per-lane accumulation and estimate and
// sum a panel's four waves in the same order, so their slabs agree to the bit (tests/test_gpu_offdiag_persist.py).
// The caller hands over per-ITEM values (fewer scalars live across the tile loop than with b, lp and the array bases) -- icoll: the
// item has collapsed row groups; amaxc_i: its amaxc word; gflag_i, g2_i: its first entries of gflag and of gmax2s (scaled) or gmax2;
// zt: zt2s (scaled) or zt2; ra: its [d + 1][Mp] block of row operands A_i, what_i.  (amaxc_i stays a pointer, read where the word is
// used: loaded by the caller, the scalar load can still be pending on one path into the tile loop, and the compiler then makes the
// loop's wait for tile ct's LDS operands a wait for tile ct + 1's prefetch as well -- lgkmcnt(0) instead of (1): the forced worst
// tier took 18.88 instead of 18.63 ms.)
// ND8: number of 8-wide blocks of input dimensions (d <= 8 * ND8).
template <int ND8, class Src>
__device__ __forceinline__ MMWaveSum mm_f32_wave_rows(const Src src, int row0, int a2, int Mp, int d, int force_worst, bool icoll,
                                                      bool scaled, const unsigned int* __restrict__ amaxc_i,
                                                      const unsigned char* __restrict__ gflag_i,
                                                      const float* __restrict__ g2_i, const double* __restrict__ zmax2,
                                                      const float* __restrict__ zt, int noskip, const float* __restrict__ ra) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  double sum = 0.0;
  // running estimate of the sweep's own rounding error (mm_common.h: MM_ROUTE_TOL; mm_route.hip): per lane -- one column,
  // the lane's 32 rows -- sum over the reduced tiles of (max|b|^3 what'_j)^2, two tiles per packed instruction; the rows' sum
  // of squares and the (1 + X + X^2) factor of rho (X = the lane's largest |b|: one v_max3 per tile pair) once per sweep
  f32x2 est2 = {0.0f, 0.0f};
  float rowsq = 0.0f, xall = 0.0f;
  // icoll: the item has collapsed groups -- then the CUBIC term of every row is in the f64 moments (k_spoly), and a group that
  // is not collapsed reduces r(b) - C0 b^3 on every tile.  coll: this wave's 64 rows are a COLLAPSED row group (mm_mono.h:
  // k_pairvec_reg decided, with the Cauchy-Schwarz bound of the group's rows, |b_ij| <= |A_i| |zc_j|); g2: its rows' max |A_i|^2
  const bool coll = icoll && row0 < Mp && gflag_i[row0 >> 6] != 0;
  // (with the scaled skip bound g2 is the group's max |A_i o l_a'|^2, gmax2s)
  const float g2 = coll ? g2_i[row0 >> 6] : 0.0f;
  // A collapsed row group visits the column tiles [ct_first, ct_end) alone: it skips, without touching them, the tiles whose
  // Cauchy-Schwarz bound with ITS rows is inside the collapsed range,
  //     max_i |A_i o l_a'|^2 (this wave's rows: gmax2s) x max_j |zc'_j / l_a'|^2 (the tile's real points: zt2s) <= MM_INSIDE_BOUND2
  // (Euclidean norms, gmax2 x zt2, where scaled is false).  zt2s is the pack's sort key, so the tiles inside are a PREFIX of a sorted
  // pack, then come the tiles to visit, then the tiles of padding alone (zt2s = 0: b = 0 there); whatever the order, every tile
  // before the first and after the last one outside the bound is inside it.  On the BASELINE recipe at C3 the scaled bound leaves
  // 8 % of the wave tiles to the screening product that the Euclidean one does (and the product finds 98 % of those inside).
  // RIGOUR: a skipped tile must be one the screened path leaves without adding anything -- the max |b| of its COMPUTED two-way
  // product is <= MM_C6_MAX, so that process_tile returns at its first or its second check with (emx, ewc) = 0.  The exact
  // |b_ij| = |sum_k (A_ik l_k) (zc'_jk / l_k)| <= |A_i o l| |zc'_j / l| <= sqrt(0.998) / 4 by Cauchy-Schwarz in the scaled metric.
  // What the computed value adds -- the f32 rounding of A_i and zc'_j, the bf16 split product without the terms of its l parts,
  // the f32 accumulation -- is bounded relative to sum_k |A_ik| |zc'_jk| <= |A_i| |zc'_j| (2^-16 of it and less), and that
  // EUCLIDEAN product is <= 1/2 because the group is collapsed (MM_COLLAPSE_BOUND2): <= 1e-5 absolute against the margin
  // (1 - sqrt(0.998)) / 4 = 2.5e-4 of MM_INSIDE_BOUND2, exactly as for the Euclidean skip.  Both arrays are rounded UP from f64
  // (k_pairvec_reg, k_pack_vectors: 1e-6 relative), and a2w adds the same again for the f32-rounded operands (< 2e-7).
  // noskip (MM_ISTAGE_NO_BOUND_SKIP): every tile goes through the screening product
  int ct_first = 0, ct_end = Mp >> 5;
  bool wave_inside = false;
  if (coll && !noskip) {
    const int nctw = Mp >> 5;
    const float a2w = g2 * 1.000001f;
    const float* ztl = zt + (size_t)a2 * nctw;
    int cf = nctw, cl = -1;
    for (int c0 = 0; c0 < nctw; c0 += 64) {
      const int c = c0 + lane;
      const bool outside = c < nctw && a2w * ztl[c < nctw ? c : 0] > MM_INSIDE_BOUND2;
      const unsigned long long bal = __ballot(outside);
      if (bal) {
        if (cf == nctw) cf = c0 + (int)__builtin_ctzll(bal);
        cl = c0 + 63 - (int)__builtin_clzll(bal);
      }
    }
    ct_first = cf & ~1;
    // (the Euclidean test as it was: to the last tile, and a group is inside by the latent's zmax2)
    if (scaled) ct_end = (cl + 2) & ~1;
    // (a collapsed group with every tile inside the collapsed range: nothing to load, nothing to add)
    wave_inside = scaled ? cf >= nctw : mm_collapse_bound2(__float_as_uint(g2), zmax2[a2]) <= MM_INSIDE_BOUND2;
  }
  if (row0 < Mp && !wave_inside) {   // Mp % 128 == 0, so a wave's 64 rows are all inside or all outside
    // bound2: the bound over all collapsed groups of the item (the screening margin)
    const float bound2 = zmax2 ? mm_collapse_bound2(*amaxc_i, zmax2[a2]) : 3.0e38f;
    // a tile is skipped on the screening product alone: its error is <= 2^-9 sum_k |A_k||Z_k| <= 2^-9 sqrt(bound2)
    const float thr_skip = MM_C6_MAX - 0.00390625f * __builtin_sqrtf(bound2) - 1e-6f;

    // ---- stationary operands --------------------------------------------------------------
    bf16x8 a1[2][ND8], a2v[2][ND8], a3[2][ND8];
    f32x2 wrow[2][8], wc0[2][8], wc1[2][8];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int row = row0 + rt * 32 + l31;
#pragma unroll
      for (int nb = 0; nb < ND8; ++nb) {
        unsigned int hh[8], mm[8], ll[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = nb * 8 + j;
          const float v = ra[(size_t)(k < d ? k : d) * Mp + row];
          mm_split3(k < d ? v : 0.0f, hh[j], mm[j], ll[j]);
        }
        u32x4 ph, pm, pl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ph[j] = hh[2 * j] | (hh[2 * j + 1] << 16);
          pm[j] = mm[2 * j] | (mm[2 * j + 1] << 16);
          pl[j] = ll[2 * j] | (ll[2 * j + 1] << 16);
        }
        // MFMA1: (m,m) | (m,h)   MFMA3: (h,m) | (h,h)   MFMA2: (h,l) | (l,h)     [lane half 0 | 1]
        // MFMA1 + MFMA3 alone are the 2-way (16-bit) product; MFMA2 adds the 2^-16 terms
        a1[rt][nb] = __builtin_bit_cast(bf16x8, pm);
        a2v[rt][nb] = __builtin_bit_cast(bf16x8, h ? pl : ph);
        a3[rt][nb] = __builtin_bit_cast(bf16x8, ph);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rr = row0 + rt * 32 + 8 * g + 4 * h;
        const float4 v = *reinterpret_cast<const float4*>(ra + (size_t)d * Mp + rr);   // factored row weights
        wrow[rt][2 * g + 0] = (f32x2){v.x, v.y};
        wrow[rt][2 * g + 1] = (f32x2){v.z, v.w};
        if constexpr (ND8 == 1) {
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            wc0[rt][2 * g + q2] = wrow[rt][2 * g + q2] * MM_PK(MMRem<1>::c[0]);
            wc1[rt][2 * g + q2] = wrow[rt][2 * g + q2] * MM_PK(MMRem<1>::c[1]);
          }
        }
      }
    }
    {
      f32x2 rs = {0.0f, 0.0f};
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 8; ++r) rs = mm_pkfma(wrow[rt][r], wrow[rt][r], rs);
      rowsq = rs[0] + rs[1];
    }

    // ---- streaming operands: lane half 0 reads parts (m, l), half 1 reads (h, h) ------------
    // lane byte offsets inside the latent's [Mp/32][3][32][8 ND8] bf16 block; the tile offset is wave-uniform and each
    // half-wave reads one contiguous 512 ND8-byte part of the tile
    const unsigned int part_bytes = 32u * 16u * ND8;
    const unsigned int offA = (h ? 0u : 1u) * part_bytes + (unsigned int)l31 * (16u * ND8);
    const unsigned int offB = (h ? 0u : 2u) * part_bytes + (unsigned int)l31 * (16u * ND8);
    const int nct = Mp >> 5;                     // Mp % 128 == 0: nct is a multiple of 4

    // zA: the (m | h) parts; zB: the (l | h) parts -- prefetched with the tile for a (b, pair) that is not collapsed, fetched on
    // demand for a collapsed one (where few tiles get that far)
    auto load_zA = [&](int ct, u32x4 (&zA)[ND8]) {
#pragma unroll
      for (int nb = 0; nb < ND8; ++nb) zA[nb] = src.zA(ct, offA, nb);
    };
    auto load_zB = [&](int ct, u32x4 (&zB)[ND8]) {
#pragma unroll
      for (int nb = 0; nb < ND8; ++nb) zB[nb] = src.zB(ct, offB, nb);
    };
    auto load_wc = [&](int j) { return src.wc(j); };

    // b_ij in two stages.  Stage 1: the 2-way split product (h + m parts, 2^-17 relative): enough when the
    // whole tile has |b| <= MM_TWO_WAY_MAX (1/32) -- the kernel only reduces r(b) = O(b^3), whose sensitivity to an error
    // in b is b^2/2.  Stage 2 (wave-uniform, only for larger tiles): the (h,l) and (l,h) terms.
    // screening product = MFMA3 alone: (h, m) | (h, h) = A_h . (Z_h + Z_m), |error| <= 2^-9 sum_k |A_k||Z_k|
    auto mfma_tile_screen = [&](const u32x4 (&zA)[ND8], f32x16 (&acc)[2]) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        f32x16 c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nb = 0; nb < ND8; ++nb)
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[rt][nb], __builtin_bit_cast(bf16x8, zA[nb]), c, 0, 0, 0);
        acc[rt] = c;
      }
    };
    // + MFMA1: (m, m) | (m, h): together with the screening product the 2-way (h + m) product
    auto mfma_tile_m = [&](const u32x4 (&zA)[ND8], f32x16 (&acc)[2]) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        f32x16 c = acc[rt];
#pragma unroll
        for (int nb = 0; nb < ND8; ++nb)
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[rt][nb], __builtin_bit_cast(bf16x8, zA[nb]), c, 0, 0, 0);
        acc[rt] = c;
      }
    };
    auto mfma_tile_l = [&](const u32x4 (&zB)[ND8], f32x16 (&acc)[2]) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        f32x16 c = acc[rt];
#pragma unroll
        for (int nb = 0; nb < ND8; ++nb)
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2v[rt][nb], __builtin_bit_cast(bf16x8, zB[nb]), c, 0, 0, 0);
        acc[rt] = c;
      }
    };
    // max |b| of a finished tile: one v_max3_f32 |a|, |b|, m per entry pair (needs -fno-honor-nans)
    auto tile_max = [&](const f32x16 (&acc)[2]) {
      // four independent v_max3 chains (a single chain of 16 dependent ops is the critical path of a skipped tile)
      float m4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < 16; ++r)
        m4[r & 3] = fmaxf(fmaxf(m4[r & 3], fabsf(acc[r >> 3][2 * (r & 7)])), fabsf(acc[r >> 3][2 * (r & 7) + 1]));
      return fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    };
    // b_ij = acc: a pure bilinear form (rho'_i, gamma_j live in the weights); tile range -> tier.
    // (sub0, sub1) = (c0, c1) of the first tier for a collapsed (b, pair) -- already in the moments -- else (0, 0).
    // collm (compile time): the (b, pair) is collapsed -- the moments already carry c0 x^3 + c1 x^4 of the first tier
    auto reduce_tile = [&](auto collm, const f32x16 (&acc)[2], float mx, float wc) {
      constexpr int CC = decltype(collm)::value;            // 0 / 1 / 2: MMRemC
      f32x2 xx[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) xx[r] = (f32x2){acc[r >> 3][2 * (r & 7)], acc[r >> 3][2 * (r & 7) + 1]};
      f32x2 part2;
      // wave-uniform tier choice (ballots, no cross-lane reduction)
      if (CC == 0 && !__any(mx > MM_TIER1_MAX)) {
        // (the folded coefficients cost 64 more VGPRs: only where the operand registers leave room, d <= 8)
        if constexpr (ND8 == 1) part2 = mm_weighted_rem1(xx, wc0, wc1);
        else part2 = mm_weighted_rem<1, 0>(xx, wrow);
      } else if (!__any(mx > MM_C6_MAX)) {
        // a collapsed row group has nothing left to add below 1/4: its moments carry this tier's own polynomial
        if constexpr (CC == 1) part2 = (f32x2){0.0f, 0.0f};
        else part2 = mm_weighted_rem<3, CC>(xx, wrow);
      } else if (!__any(mx > 0.5f)) {
        part2 = mm_weighted_rem<4, CC>(xx, wrow);
      } else if (!__any(mx > 1.0f)) {
        part2 = mm_weighted_rem<5, CC>(xx, wrow);
      } else {
        part2 = (f32x2){0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int e2 = 0; e2 < 2; ++e2) {
            // |b| > 1: exp2 on the transcendental unit, then the three leading terms subtracted
            const float x = fminf(xx[r][e2], MM_EXP_CAP_F32);     // (mm_common.h: exponent caps)
            const float xs = fminf(fmaxf(x, -1.0f), 1.0f);
            const float big = (__builtin_amdgcn_exp2f(x * 1.44269504f) - 1.0f) - fmaf(0.5f * x, x, x);
            float e = (fabsf(x) <= 1.0f) ? mm_rem_p5(xs) : big;
            if constexpr (CC == 1) e -= (x * x) * x * fmaf(fmaf(fmaf(MM_C6_C3, x, MM_C6_C2), x, MM_C6_C1), x, MM_C6_C0);
            if constexpr (CC == 2) e -= (x * x) * (x * MM_C6_C0);
            part2[e2] = fmaf(wrow[r >> 3][r & 7][e2], e, part2[e2]);
          }
      }
      sum += (double)wc * (double)(part2[0] + part2[1]);
    };
    // one wave tile: screening product; a collapsed (b, pair) stops here when the whole tile is inside the collapsed
    // range; else the rest of the split product, the range tier and the weighted reduction
    // collc (compile time): SCREENED sweep -- the screening check, and neither the column weight nor the (l | h) parts
    // prefetched (few tiles of such an item need them, and a prefetched global load would put its latency on every tile
    // of a sweep that is otherwise 2 MFMAs long); collm: collapsed coefficients (reduce_tile)
    // (emx, ewc): what the error estimate takes from this tile -- its max|b| of the lane and the column weight; zeros for a
    // tile that contributes exact moments only
    auto process_tile = [&](auto collc, auto collm, int ct, const u32x4 (&zA)[ND8], u32x4 (&zB)[ND8], float wc, float& emx, float& ewc) __attribute__((always_inline)) {
      constexpr bool CM = decltype(collc)::value;
      f32x16 acc[2];
      emx = 0.0f; ewc = 0.0f;
      mfma_tile_screen(zA, acc);
      if constexpr (CM) {
        const float ms = tile_max(acc);
        if (!__any(ms > thr_skip)) return;
      }
      mfma_tile_m(zA, acc);
      const float mx = force_worst ? 2.0f : tile_max(acc);       // MM_FORCE_WORST_TIER: wave-uniform override
      if constexpr (CM) {
        if (!__any(mx > MM_C6_MAX)) return;                           // inside the collapsed range: all in the moments
      }
      if constexpr (CM) wc = load_wc(ct * 32 + l31);
      emx = mx; ewc = wc;
      if (__any(mx > MM_TWO_WAY_MAX)) {
        if constexpr (CM) load_zB(ct, zB);
        mfma_tile_l(zB, acc);
      }
      reduce_tile(collm, acc, mx, wc);
    };

    // two-stage register ping-pong: tile ct + 1 is in flight while tile ct is reduced.  (Issuing the MFMAs
    // of tile ct + 1 interleaved with the v_max3 range check of tile ct -- a second accumulator set,
    // 182 VGPRs -- was measured: 4.27 ms against 4.25 ms; three waves per SIMD already overlap the two.)
    // (a collapsed row group sweeps [ct_first, ct_end): above)
    auto sweep = [&](auto collc, auto collm) __attribute__((always_inline)) {
      constexpr bool CM = decltype(collc)::value;
      u32x4 zA0[ND8], zB0[ND8], zA1[ND8], zB1[ND8];
      float w0, w1;
      w0 = w1 = 0.0f;
      const int ct0 = CM ? ct_first : 0, cte = CM ? ct_end : nct;
      if (ct0 >= cte) return;
      load_zA(ct0, zA0);
      if constexpr (!CM) { load_zB(0, zB0); w0 = load_wc(l31); }
      for (int ct = ct0; ct < cte; ct += 2) {
        load_zA(ct + 1, zA1);
        if constexpr (!CM) { load_zB(ct + 1, zB1); w1 = load_wc((ct + 1) * 32 + l31); }
        float emx0, ewc0, emx1, ewc1;
        process_tile(collc, collm, ct, zA0, zB0, w0, emx0, ewc0);
        const int cn = ct + 2 < cte ? ct + 2 : ct;               // clamped: the last pass re-reads its own tile
        load_zA(cn, zA0);
        if constexpr (!CM) { load_zB(cn, zB0); w0 = load_wc(cn * 32 + l31); }
        process_tile(collc, collm, ct + 1, zA1, zB1, w1, emx1, ewc1);
#if MM_ROUTE_EST
        {
          const f32x2 emx = {emx0, emx1}, ewc = {ewc0, ewc1};
          const f32x2 u = (emx * emx) * (emx * ewc);             // both tiles at once: 4 packed instructions per tile pair
          est2 = mm_pkfma(u, u, est2);
          xall = fmaxf(fmaxf(xall, emx0), emx1);
        }
#endif
      }
    };
    // A (b, pair) is collapsed only where its bound lets the screening skip most tiles (MM_COLLAPSE_BOUND2 = (1/2)^2: on the
    // BASELINE recipe items with a bound in (1/4, 1/2] have 98 % of their wave tiles under 1/4, items beyond 1/2 a third,
    // tools/tile_hist_baseline.py).
    // (Two instantiations, not a run-time flag: a non-collapsed item must not pay for the collapsed coefficients -- as a flag
    // they cost the exp2 branch 4 more ops per entry: forced-worst C3 12.5 -> 16.8 ms)
    // (the third: the dense row groups of an item that has collapsed ones, cubic term in the moments)
    if (coll) sweep(mm_true{}, mm_int<1>{});
    else if (icoll) sweep(mm_false{}, mm_int<2>{});
    else sweep(mm_false{}, mm_int<0>{});
  }
  {
    const float xf = fminf(xall, 8.0f);                     // (beyond |b| = 8 the estimate is astronomically large anyway)
    const float pf = fmaxf(fmaf(xf, xf, xf) + 1.0f, __expf(xf));   // e^X <= 1 + X + X^2 only up to X = 1.79: the larger of the two (X <= 8)
    return {sum, ((est2[0] + est2[1]) * rowsq) * (pf * pf)};
  }
}

// An item (or a workgroup's panels of it) has no tile to visit: zeros in the panels first, first + stride, ... of its partB and
// estO rows pB, eO (exact -- all of it is in the f64 moments: nothing to estimate; eO may be null)
__device__ __forceinline__ void mm_zero_panels(double* __restrict__ pB, float* __restrict__ eO, int npanel, int first, int stride) {
  for (int panel = first; panel < npanel; panel += stride) {
    pB[panel] = 0.0;
    if (eO) eO[panel] = 0.0f;
  }
}

// The slot sweep: one grid slot per (b, pair) and group of row panels (every shape with d > 8 or Mp > MM_F32P_MAX_MP, and the forced
// worst tier; the persistent sweep below takes the others).
//
// The bilinear form A_i . zc_j runs on the bf16 matrix pipe as a 3-way split product
// (h/m/l bf16 parts, six cross terms packed into three K=16 MFMAs per 8 dims: f32-equivalent
// accuracy), because v_mfma_f32_32x32x2_f32 was measured to serialise with the VALU
// on a SIMD (it shares the f32 FMA datapath) while the bf16 MFMA overlaps with it.
//   stationary operand (registers, split once per sweep): A_i = G^T zeta_i of the wave's 64 rows and
//   their factored weights what_i; streaming operand: the model's pre-split centred inducing inputs
//   of latent a' (b-independent, L2-resident) and what'_j per column.
// LDSZ: the (h, m) parts of the column latent's split inputs -- all the screening product and the 2-way product read --
// are staged ONCE per workgroup in LDS (Mp * 32 ND8 bytes: 64 KB at C3) and shared by its four waves: a collapsed
// (b, pair) is a sweep of one MFMA + one range check per 32 x 32 block, which from L2 would be bound by the
// 1 KB per wave tile of operand traffic (measured 2.0 ms at C3 against 0.4 ms of MFMA time).
template <int ND8, bool LDSZ>
__global__ __launch_bounds__(256, (ND8 >= 4 ? 1 : MM_F32_WAVES)) void k_qred_f32_mfma(const unsigned short* __restrict__ Zs3,
                                                          int L, int Mp, int d, int P, int Po, int NS,
                                                          int npanel, int ppw, int nwork, int force_worst,
                                                          const unsigned int* __restrict__ amax,
                                                          const unsigned int* __restrict__ amaxc,
                                                          const unsigned char* __restrict__ gflag, const float* __restrict__ gmax2,
                                                          const double* __restrict__ zmax2, const float* __restrict__ zt2,
                                                          const float* __restrict__ gmax2s, const float* __restrict__ zt2s,
                                                          int noskip,
                                                          const float* __restrict__ rowO,
                                                          const float* __restrict__ colO,
                                                          double* __restrict__ partB, float* __restrict__ estO,
                                                          int* __restrict__ rcount) {
  // XCD-aware remap of the 1-D grid (blocks b and b+8 share an XCD): consecutive work items
  // go to the same XCD.  Bijective for any nwork (cdna guide T1).
  const int orig = blockIdx.x;
  if (orig == 0 && threadIdx.x == 0 && rcount) { rcount[0] = 0; rcount[1] = 0; }   // this pass's route list (k_route_decide follows)
  const int xcd = orig & 7, slot = orig >> 3;
  const int qn = nwork >> 3, rn = nwork & 7;
  const int wi = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
  // a workgroup owns ppw consecutive row panels of one (b, pair) (all of them when the operand image is staged in
  // LDS: the 64 KB fill is then paid once per (b, pair)); npw = ceil(npanel / ppw) workgroups per (b, pair)
  const int npw = (npanel + ppw - 1) / ppw;
  const int pgrp = wi % npw;
  const int t = wi / npw;
  const int lp = t % Po, b = t / Po;
  const int p = L + lp;
  int a, a2;
  mm_decode_pair_o(p, L, a, a2);
  const size_t item = (size_t)b * Po + lp, slab = ((size_t)b * P + p) * NS;

  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if constexpr (ND8 == 1) {
    // Cauchy-Schwarz already bounds every |b_ij| of this (b, pair) by MM_C6_MAX: the remainder is p6 everywhere, which the
    // moments carry (k_spoly, k_spoly56) -- every tile would be skipped: no sweep at all
    // (noskip -- MM_ISTAGE_NO_BOUND_SKIP: an item with collapsed groups stays and its tiles go through the screening product)
    if (!force_worst && zmax2 && mm_collapse_bound2(amax[item], zmax2[a2]) <= MM_INSIDE_BOUND2 &&
        !(noskip && mm_item_collapsed(amaxc[item]))) {
      mm_zero_panels(partB + slab, estO ? estO + item * npanel : nullptr, npanel, pgrp + (int)threadIdx.x * npw, 256 * npw);
      return;
    }
  }
  // Row-group collapse (mm_mono.h): does any wave of this workgroup have a tile to visit?  A collapsed group whose Cauchy-Schwarz
  // bound with the column latent's LARGEST point is inside the collapsed range has none (gmax2: its rows' max |A_i|^2 from
  // k_pairvec_reg) -- with the pack in norm order those are the first panels of most items; a workgroup of such groups alone
  // writes its zero partials and leaves before the 64 KB fill
  const bool icoll = (ND8 == 1) && !force_worst && zmax2 != nullptr && zt2 != nullptr && gmax2 != nullptr &&
                     mm_item_collapsed(amaxc[item]);
  const size_t grp0 = item * (size_t)(Mp / MM_GROUP_ROWS);
  // scaled: the skip sites take the lengthscale-scaled bound (gmax2s x zt2s), else the Euclidean one (wave-uniform)
  const bool scaled = gmax2s != nullptr && zt2s != nullptr;
  if constexpr (ND8 == 1) {
    if (icoll && !noskip) {
      const float zsmax = scaled ? mm_wave_max_tiles(zt2s + (size_t)a2 * (Mp >> 5), Mp >> 5, lane) : 0.0f;
      bool need = false;
      for (int panel = pgrp; panel < npanel; panel += npw) {
        const int g = (panel * MM_PANEL_ROWS + wv * 64) >> 6;
        if (g < Mp / MM_GROUP_ROWS)
          need = need || !(gflag[grp0 + g] != 0 && mm_group_inside(gmax2, scaled ? gmax2s : nullptr, grp0 + g, zmax2[a2], zsmax));
      }
      if (!__syncthreads_or(need ? 1 : 0)) {
        mm_zero_panels(partB + slab, estO ? estO + item * npanel : nullptr, npanel, pgrp + (int)threadIdx.x * npw, 256 * npw);
        return;
      }
    }
  }
  extern __shared__ __align__(16) char zlds[];     // LDSZ: [Mp/32 tiles][2 parts (h, m)][32 columns][16 ND8 bytes]
  if constexpr (LDSZ) {
    // the first two parts of every tile are contiguous in the packed model ([tile][h, m, l][32][16 ND8]): copy
    // 1024 ND8 of every 1536 ND8 bytes, 16 bytes per thread and pass
    const char* src = reinterpret_cast<const char*>(Zs3 + (size_t)a2 * Mp * (24 * ND8));
    const int nchunk = (Mp >> 5) * 64 * ND8;         // 16-byte chunks
    // batches of 8 chunks per thread: all loads of a batch are issued before its LDS stores (a load -> store loop
    // would pay one memory latency per chunk)
    for (int c0 = 0; c0 < nchunk; c0 += 8 * 256) {
      u32x4 tmp[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int c = c0 + u * 256 + (int)threadIdx.x;
        c = c < nchunk ? c : nchunk - 1;
        const int tile = c / (64 * ND8), within = c - tile * (64 * ND8);
        tmp[u] = *reinterpret_cast<const u32x4*>(src + (size_t)tile * (1536 * ND8) + (size_t)within * 16);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u * 256 + (int)threadIdx.x;
        if (c < nchunk) *reinterpret_cast<u32x4*>(zlds + (size_t)c * 16) = tmp[u];
      }
    }
    __syncthreads();
  }
  __shared__ double red[4];
  __shared__ float redf[4];
  // the item's operands: the pre-split centred inducing inputs of latent a' ([Mp/32][3 (h,m,l)][32][8 ND8] bf16), what'_j, the
  // rows' [d+1][Mp] block (A_i, what_i) and its entries of gflag and of the skip bound's row factor
  const MMSrcL2<ND8, LDSZ> src = {zlds, reinterpret_cast<const char*>(Zs3 + (size_t)a2 * Mp * (24 * ND8)), colO + item * Mp};
  const float* ra = rowO + item * (size_t)(d + 1) * Mp;
  const unsigned char* gflag_i = gflag + grp0;
  const float* g2_i = (scaled ? gmax2s : gmax2) + grp0;
  // the workgroup's panels are INTERLEAVED (pgrp, pgrp + npw, ...): with the pack in norm order the rows of large |A_i| -- the
  // tiles that are not skipped -- are the last panels, and consecutive panels would give one workgroup of four all of an item's work
  for (int panel = pgrp; panel < npanel; panel += npw) {
    MMWaveSum ws = mm_f32_wave_rows<ND8>(src, panel * MM_PANEL_ROWS + wv * 64, a2, Mp, d, force_worst, icoll, scaled, amaxc + item,
                                         gflag_i, g2_i, zmax2, scaled ? zt2s : zt2, noskip, ra);
    // workgroup reduction -> slab
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ws.sum += __shfl_down(ws.sum, off, 64); ws.est += __shfl_down(ws.est, off, 64); }
    __syncthreads();                               // (the previous panel's red[] has been read)
    if (lane == 0) { red[wv] = ws.sum; redf[wv] = ws.est; }
    __syncthreads();
    if (threadIdx.x == 0) {
      partB[slab + panel] = red[0] + red[1] + red[2] + red[3];
      if (estO) estO[item * npanel + panel] = (redf[0] + redf[1]) + (redf[2] + redf[3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The persistent sweep (d <= 8, Mp <= MM_F32P_MAX_MP): a work list of the (b, pair) items that have a tile to visit, and one
// workgroup per CU that takes items from it.
//
// k_qred_f32_mfma above pays, per (b, pair), a grid slot even where every wave leaves at once (53 % of the BASELINE recipe's items),
// a 64 KB LDS fill of an image that depends on the column latent alone (7 distinct images per step at C3, ~6.7 k fills), and, in
// the dense row groups, per-tile (l | h) operand and column-weight loads from L2 that two waves per SIMD cannot hide (half of their
// ~1 870 SIMD-cycles per wave tile).  Here:
//   k_offdiag_worklist (one wave per item) applies the same "does any wave have a tile to visit" predicate, writes the zero slabs of
//   the items without work, and lists the others by column latent a' -- bucket a' holds the B a' items of the pairs (a < a', a'),
//   those with dense (not collapsed) row groups from its front, the others from its back;
//   k_qred_f32_mfma_persist (MM_F32P_WAVES waves, one workgroup per CU) takes items through an atomic counter in list order, so that
//   it refills the 96 KB latent image only when the column latent changes, copies the item's what'_j (8 KB) beside it, and hands the
//   item's 64-row groups to its waves through an LDS counter, last group (largest |A_i|: the dense ones) first.  Each wave runs
//   mm_f32_wave_rows with every operand from LDS and leaves its reduced (sum, estimate) in the group's LDS slot; after one barrier
//   the panel sums are red[4 p] + .. + red[4 p + 3] left to right, as in k_qred_f32_mfma: the slabs are bit-identical.
// Workspace: MMWorkspaceLayout::plist ([0] the queue counter, [4 + 2 a'] / [5 + 2 a'] the front / back counts of bucket a', zeroed
// before every pass; the list behind them).
// ---------------------------------------------------------------------------------------------------------------------------
#ifndef MM_F32P_WAVES
#define MM_F32P_WAVES 8
#endif
// largest Mp whose latent image (Mp * 48 bytes), column weights (Mp * 4) and group slots fit the 160 KB of LDS
#define MM_F32P_MAX_MP 2048
static inline size_t mm_f32p_lds_bytes(int Mp) {
  return (size_t)Mp * 48 + (size_t)Mp * 4 + (size_t)mm_mfma_groups(Mp) * 12;
}

__global__ __launch_bounds__(256) void k_offdiag_worklist(int L, int Mp, int P, int Po, int NS, int npanel, int B, int force_worst,
                                                          const unsigned int* __restrict__ amax, const unsigned int* __restrict__ amaxc,
                                                          const unsigned char* __restrict__ gflag, const float* __restrict__ gmax2,
                                                          const double* __restrict__ zmax2, const float* __restrict__ gmax2s,
                                                          const float* __restrict__ zt2s, int noskip, double* __restrict__ partB,
                                                          float* __restrict__ estO, int* __restrict__ plist, int* __restrict__ rcount) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { rcount[0] = 0; rcount[1] = 0; }   // this pass's route list (k_route_decide follows)
  const int item = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= B * Po) return;                                 // (wave-uniform)
  const int b = item / Po, lp = item - b * Po, p = L + lp;
  int a, a2;
  mm_decode_pair_o(p, L, a, a2);
  bool work = true, dense = true;
  if (!force_worst) {
    const bool ic = mm_item_collapsed(amaxc[item]);
    if (mm_collapse_bound2(amax[item], zmax2[a2]) <= MM_INSIDE_BOUND2 && !(noskip && ic)) {
      work = false;                                           // every |b_ij| inside the collapsed range
    } else if (ic) {
      // row groups (k_qred_f32_mfma's need / wave_inside): a collapsed group inside by its own bound has no tile to visit -- the
      // lengthscale-scaled bound where gmax2s / zt2s are given, else the Euclidean one; noskip: every such item is listed
      const int ng = Mp / MM_GROUP_ROWS;
      const size_t grp0 = (size_t)item * ng;
      const bool scaled = gmax2s != nullptr && zt2s != nullptr;
      const float zsmax = (scaled && !noskip) ? mm_wave_max_tiles(zt2s + (size_t)a2 * (Mp >> 5), Mp >> 5, lane) : 0.0f;
      bool need = false, dn = false;
      for (int g = lane; g < ng; g += 64) {
        const bool coll = gflag[grp0 + g] != 0;
        need = need || noskip || !(coll && mm_group_inside(gmax2, scaled ? gmax2s : nullptr, grp0 + g, zmax2[a2], zsmax));
        dn = dn || !coll;
      }
      work = __any(need);
      dense = __any(dn);
    }
  }
  if (!work) {
    mm_zero_panels(partB + ((size_t)b * P + p) * NS, estO + (size_t)item * npanel, npanel, lane, 64);
    return;
  }
  if (lane == 0) {
    int* list = plist + mm_f32p_list_off(L);
    const int off = B * (a2 * (a2 - 1) / 2), cap = B * a2;    // bucket a2: the B a2 items of the pairs (a < a2, a2)
    if (dense) list[off + atomicAdd(plist + 4 + 2 * a2, 1)] = item;
    else list[off + cap - 1 - atomicAdd(plist + 5 + 2 * a2, 1)] = item;
  }
}

__global__ __launch_bounds__(64 * MM_F32P_WAVES, 1) void k_qred_f32_mfma_persist(const unsigned short* __restrict__ Zs3, int L, int Mp,
                                                                               int d, int P, int Po, int NS, int npanel, int B,
                                                                               int force_worst, const unsigned int* __restrict__ amaxc,
                                                                               const unsigned char* __restrict__ gflag,
                                                                               const float* __restrict__ gmax2,
                                                                               const double* __restrict__ zmax2,
                                                                               const float* __restrict__ zt2,
                                                                               const float* __restrict__ gmax2s,
                                                                               const float* __restrict__ zt2s, int noskip,
                                                                               const float* __restrict__ rowO,
                                                                               const float* __restrict__ colO,
                                                                               double* __restrict__ partB, float* __restrict__ estO,
                                                                               int* __restrict__ plist) {
  constexpr int NT = 64 * MM_F32P_WAVES;
  // LDS: the column latent's [Mp/32][3 (h, m, l)][32][16] image | the item's what'_j [Mp] f32 | per 64-row group: sum f64, estimate f32
  extern __shared__ __align__(16) char zlds[];
  __shared__ int s_next, s_gcur;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ngrp = mm_mfma_groups(Mp);
  float* wlds = reinterpret_cast<float*>(zlds + (size_t)Mp * 48);
  double* red = reinterpret_cast<double*>(wlds + Mp);
  float* redf = reinterpret_cast<float*>(red + ngrp);
  const int* cnt = plist + 4;                                 // [L][front, back]
  const int* list = plist + mm_f32p_list_off(L);
  int total = 0;
  for (int c = 1; c < L; ++c) total += cnt[2 * c] + cnt[2 * c + 1];
  if (tid == 0) s_next = atomicAdd(plist, 1);
  __syncthreads();
  int cur = -1;                                               // the column latent of the LDS image
  for (;;) {
    int r = __builtin_amdgcn_readfirstlane(s_next);
    if (r >= total) break;
    // list position -> item: bucket c (column latent), dense items from its front, the others from its back
    int c = 1;
    while (r >= cnt[2 * c] + cnt[2 * c + 1]) { r -= cnt[2 * c] + cnt[2 * c + 1]; ++c; }
    const int boff = B * (c * (c - 1) / 2);
    const int item = __builtin_amdgcn_readfirstlane(list[boff + (r < cnt[2 * c] ? r : B * c - 1 - (r - cnt[2 * c]))]);
    const int b = item / Po, lp = item - b * Po, p = L + lp;
    int a, a2;
    mm_decode_pair_o(p, L, a, a2);
    // (the fills' per-thread offsets are recomputed per item: hoisted out of the item loop they took registers of the tile loop)
    int ft = tid;
    asm volatile("" : "+v"(ft));
    if (a2 != cur) {
      // the latent's three parts are one contiguous block of the packed model: 16-byte chunks, 8 in flight per thread
      const char* src = reinterpret_cast<const char*>(Zs3 + (size_t)a2 * Mp * 24);
      const int nchunk = Mp * 3;
      for (int c0 = 0; c0 < nchunk; c0 += 8 * NT) {
        u32x4 tmp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int ch = c0 + u * NT + ft;
          tmp[u] = *reinterpret_cast<const u32x4*>(src + (size_t)(ch < nchunk ? ch : nchunk - 1) * 16);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int ch = c0 + u * NT + ft;
          if (ch < nchunk) *reinterpret_cast<u32x4*>(zlds + (size_t)ch * 16) = tmp[u];
        }
      }
      cur = a2;
    }
    {
      const float* src = colO + (size_t)item * Mp;
      for (int ch = ft; ch < Mp / 4; ch += NT)
        reinterpret_cast<u32x4*>(wlds)[ch] = *reinterpret_cast<const u32x4*>(src + (size_t)ch * 4);
    }
    if (tid == 0) s_gcur = 0;
    __syncthreads();                                          // image, what'_j, s_gcur ready; everyone has read s_next
    if (tid == 0) s_next = atomicAdd(plist, 1);               // (the next item, read after the barrier below)
    const bool icoll = !force_worst && mm_item_collapsed(amaxc[item]);
    const size_t grp0 = (size_t)item * (size_t)(Mp / MM_GROUP_ROWS);
    const bool scaled = gmax2s != nullptr && zt2s != nullptr;   // (the skip bound's metric: k_qred_f32_mfma)
    const float* ra = rowO + (size_t)item * (size_t)(d + 1) * Mp;
    // (every lane takes part in the LDS atomic -- lane 0 adds 1, the others 0 -- and lane 0's old value is the wave's: no
    // lane-divergent branch around it, so the loop stays wave-uniform for the compiler as it is at run time)
    for (int gi = __builtin_amdgcn_readfirstlane(atomicAdd(&s_gcur, lane == 0 ? 1 : 0)); gi < ngrp;
         gi = __builtin_amdgcn_readfirstlane(atomicAdd(&s_gcur, lane == 0 ? 1 : 0))) {
      const int g = ngrp - 1 - gi;
      MMWaveSum ws = mm_f32_wave_rows<1>(MMSrcLds{zlds, wlds}, g * 64, a2, Mp, d, force_worst, icoll, scaled, amaxc + item, gflag + grp0,
                                         (scaled ? gmax2s : gmax2) + grp0, zmax2, scaled ? zt2s : zt2, noskip, ra);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { ws.sum += __shfl_down(ws.sum, off, 64); ws.est += __shfl_down(ws.est, off, 64); }
      if (lane == 0) { red[g] = ws.sum; redf[g] = ws.est; }
    }
    __syncthreads();                                          // every group's slot written
    for (int panel = tid; panel < npanel; panel += NT) {
      const double* rp = red + 4 * panel;
      const float* rf = redf + 4 * panel;
      partB[((size_t)b * P + p) * NS + panel] = rp[0] + rp[1] + rp[2] + rp[3];
      estO[(size_t)item * npanel + panel] = (rf[0] + rf[1]) + (rf[2] + rf[3]);
    }
    // (the next item's writes of red[] follow its first barrier; its image / what'_j writes touch nothing read here)
  }
}

extern "C" int mm_mfma_supported(int d) { return d >= 1 && d <= 32; }

// Diagnostics of the bound-based skipping (include/gpflowpilco_mm.h).
__global__ void k_worklist_len(const int* __restrict__ plist, int L, int32_t* __restrict__ out) {
  int n = 0;
  for (int c = 1; c < L; ++c) n += plist[4 + 2 * c] + plist[5 + 2 * c];
  out[0] = n;
}

extern "C" int mm_offdiag_worklist_len(int L, int M, int d, int dtype, int B, int flags, const void* workspace, size_t workspace_bytes,
                                       int32_t* out, void* stream) {
  if (!workspace || !out || L <= 0 || M <= 0 || d <= 0 || d > MM_DMAX || B <= 0) return MM_E_ARG;
  const MMWorkspaceLayout wl = mm_workspace_layout(B, L, M, d, dtype, flags);
  if (workspace_bytes < wl.total) return MM_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(out, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  if (dtype != MM_F32 || wl.Po == 0 || d > 8 || wl.Mp > MM_F32P_MAX_MP) return 0;      // (no persistent sweep: no list)
  hipLaunchKernelGGL(k_worklist_len, dim3(1), dim3(1), 0, s, (const int*)((const char*)workspace + wl.plist), L, out);
  const hipError_t el = hipGetLastError();
  return el == hipSuccess ? 0 : (int)el;
}

extern "C" int mm_offdiag_skip_bounds(const void* packed, size_t packed_bytes, int L, int M, int d, int dtype, int B, int flags,
                                      const void* workspace, size_t workspace_bytes, float* zt2s_out, float* gmax2s_out, void* stream) {
  if (!packed || !workspace || !zt2s_out || !gmax2s_out || L <= 0 || M <= 0 || d <= 0 || d > MM_DMAX || B <= 0) return MM_E_ARG;
  if (dtype != MM_F32 || d > 8) return MM_E_DIM;
  const MMModelLayout ml = mm_model_layout(L, M, d, dtype, 1);
  const MMWorkspaceLayout wl = mm_workspace_layout(B, L, M, d, dtype, flags);
  if (packed_bytes < ml.Cm || workspace_bytes < wl.total) return MM_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(zt2s_out, (const char*)packed + ml.zt2s, (size_t)L * (ml.Mp / 32) * 4, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && wl.Po > 0)
    e = hipMemcpyAsync(gmax2s_out, (const char*)workspace + wl.gmax2s, (size_t)B * wl.Po * (wl.Mp / MM_GROUP_ROWS) * 4,
                       hipMemcpyDeviceToDevice, s);
  return e == hipSuccess ? 0 : (int)e;
}

int mm_mfma_num_slots(int Mp) { return (Mp + MM_PANEL_ROWS - 1) / MM_PANEL_ROWS; }

int mm_launch_qred_mfma(const char* packed, const MMModelLayout& ml, char* ws, const MMWorkspaceLayout& wl,
                        int B, int L, int d, int flags, hipStream_t stream) {
  const int npanel = mm_mfma_num_slots(wl.Mp);
  const int force_worst = (flags & MM_FORCE_WORST_TIER) ? 1 : 0;
  const unsigned int* amax = (const unsigned int*)(ws + wl.amax);
  const double* zmax2 = mm_moment_deg(d) >= 4 ? (const double*)(packed + ml.zmax2) : nullptr;
  // the skip bound's metric: lengthscale-scaled where the row groups exist (d <= 8), unless MM_ISTAGE_OLD_SKIP_BOUND asks for the
  // Euclidean test at every site (null pointers); MM_ISTAGE_NO_BOUND_SKIP: no bound-based skipping
  const bool scaled = zmax2 != nullptr && ml.nd8 == 1 && !(flags & MM_ISTAGE_OLD_SKIP_BOUND);
  const float* gmax2s = scaled ? (const float*)(ws + wl.gmax2s) : nullptr;
  const float* zt2s = scaled ? (const float*)(packed + ml.zt2s) : nullptr;
  const int noskip = (flags & MM_ISTAGE_NO_BOUND_SKIP) ? 1 : 0;
  // the (h, m) parts of one latent in LDS when they fit beside a second workgroup (<= 64 KB): d <= 8 and M <= 2048
  const size_t zbytes = (size_t)wl.Mp * 32 * ml.nd8;
  const bool ldsz = ml.nd8 == 1 && zbytes <= 65536;
  // LDS-staged: one workgroup per (b, pair) (the fill is paid once) as long as that still leaves >= 8 rounds of
  // 512 resident workgroups; else one per panel
  int ppw = 1;
  if (ldsz && (long long)wl.Po * B >= 4096) ppw = (npanel + MM_F32_PPW_DIV - 1) / MM_F32_PPW_DIV;
  const long long nwork_ll = (long long)((npanel + ppw - 1) / ppw) * wl.Po * B;
  if (nwork_ll <= 0 || nwork_ll > 0x7fffffffLL) return MM_E_DIM;
  const int nwork = (int)nwork_ll;
  const unsigned short* Zs3 = (const unsigned short*)(packed + ml.Zs3);
  const float* rowO = (const float*)(ws + wl.rowO);
  const float* colO = (const float*)(ws + wl.colO);
  double* partB = (double*)(ws + wl.partB);
  float* estO = (float*)(ws + wl.estO);
  // (not with the forced worst tier: every group is dense there and the per-item fill and barriers cost more than the staged
  // operands save -- measured at C3, worst regime 18.64 -> 19.07 ms per step)
  if (ml.nd8 == 1 && zmax2 && wl.Mp <= MM_F32P_MAX_MP && !force_worst && !(flags & MM_ISTAGE_OLD_OFFDIAG)) {
    // the work list (zeroed header first), then the persistent sweep over it: one workgroup per CU
    int* plist = (int*)(ws + wl.plist);
    const int nitem = wl.Po * B;                       // (<= nwork above)
    const hipError_t em = hipMemsetAsync(plist, 0, (size_t)mm_f32p_list_off(L) * 4, stream);
    if (em != hipSuccess) return (int)em;
    hipLaunchKernelGGL(k_offdiag_worklist, dim3((nitem + 3) / 4), dim3(256), 0, stream, L, wl.Mp, wl.P, wl.Po, wl.NS, npanel, B,
                       force_worst, amax, (const unsigned int*)(ws + wl.amaxc), (const unsigned char*)(ws + wl.gflag),
                       (const float*)(ws + wl.gmax2), zmax2, gmax2s, zt2s, noskip, partB, estO, plist, (int*)(ws + wl.rcount));
    const hipError_t el = hipGetLastError();
    if (el != hipSuccess) return (int)el;
    // (raise the dynamic-LDS limit and read the CU count once per device: the calls are slow)
    const size_t shm = mm_f32p_lds_bytes(wl.Mp);
    static std::atomic<unsigned long long> attr_done{0ull};
    static std::atomic<int> ncu_cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 64;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
    int ncu = bit ? ncu_cached[dev].load() : 0;
    if (!bit || !(attr_done.load() & bit)) {
      const hipError_t ea = hipFuncSetAttribute((const void*)k_qred_f32_mfma_persist, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)mm_f32p_lds_bytes(MM_F32P_MAX_MP));
      if (ea != hipSuccess) return (int)ea;
      int v = 0;
      if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev < 64 ? dev : 0) != hipSuccess || v <= 0) v = 256;
      ncu = v;
      if (bit) { ncu_cached[dev].store(v); attr_done.fetch_or(bit); }
    }
    if (ncu <= 0) ncu = 256;
    hipLaunchKernelGGL(k_qred_f32_mfma_persist, dim3(nitem < ncu ? nitem : ncu), dim3(64 * MM_F32P_WAVES), shm, stream, Zs3, L, wl.Mp,
                       d, wl.P, wl.Po, wl.NS, npanel, B, force_worst, (const unsigned int*)(ws + wl.amaxc),
                       (const unsigned char*)(ws + wl.gflag), (const float*)(ws + wl.gmax2), zmax2, (const float*)(packed + ml.zt2),
                       gmax2s, zt2s, noskip, rowO, colO, partB, estO, plist);
    const hipError_t ep = hipGetLastError();
    return ep == hipSuccess ? 0 : (int)ep;
  }
#define MM_LAUNCH_ND(ND_, LZ_, SH_)                                                                          \
  hipLaunchKernelGGL((k_qred_f32_mfma<ND_, LZ_>), dim3(nwork), dim3(256), SH_, stream, Zs3, L, wl.Mp, d,    \
                     wl.P, wl.Po, wl.NS, npanel, ppw, nwork, force_worst, amax, (const unsigned int*)(ws + wl.amaxc), \
                     (const unsigned char*)(ws + wl.gflag), (const float*)(ws + wl.gmax2), zmax2, (const float*)(packed + ml.zt2), gmax2s, zt2s, noskip, rowO, colO, partB, estO, (int*)(ws + wl.rcount))
  switch (ml.nd8) {
    case 1: if (ldsz) MM_LAUNCH_ND(1, true, zbytes); else MM_LAUNCH_ND(1, false, 0); break;
    case 2: MM_LAUNCH_ND(2, false, 0); break;
    case 3: MM_LAUNCH_ND(3, false, 0); break;
    default: MM_LAUNCH_ND(4, false, 0); break;
  }
#undef MM_LAUNCH_ND
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
