// Path GENERATION for the pathwise sampler on gfx950 (pathwise.PathSampler) -- SURVEY.md row f-3.
// PathwisePILCO draws new sample paths on every optimiser step (gpflow_pilco/loops/pilco.py:281-284); what torch does per draw
// around the two GEMMs and the two triangular solves is reformatting: ~a dozen elementwise ops for the random-Fourier basis, and
// pad / concatenate / permute / cast / copy of the whole [S, L, Kp + Mp] weight array for the blocked stream of mm_pathwise.hip.
// Two kernels replace it:
//
//   k_pw_basis   n [L,K,d], b [L,K] (the draws), Z, ls, var  ->  omega_t [L,d,Kp] T, phase [L,Kp] T (what the evaluation kernels read)
//                and Phi_Z [L,M,K] f64 = sqrt(2 var / K) cos(Z omega^T + b) (what the update's right-hand side is formed from)
//   k_pw_pack_*  w [S,L,K] f64 (prior weights as drawn), v [L,M,S] f64 (update weights as the triangular solves leave them)
//                ->  wb [G][L][NB][4][BT] T, every element written exactly once (padding included: no memset between draws)
//
// The pack is HBM-bound with no arithmetic: 8 bytes read and sizeof(T) written per weight.  Its prior blocks are a cast of
// contiguous rows.  Its update blocks are a TRANSPOSE (s is the fast axis of v, t = m the fast axis of wb): a workgroup takes
// BT inducing points x 32 samples, reads v in 256-byte runs along s, casts, and stages the tile in LDS as [32 samples][BT] T with a
// row stride of 1024 + 16 bytes -- a thread holds 4 consecutive m of one sample and stores them with 16-byte ds_writes, whose
// 8-lane groups (8 consecutive samples, 260 dwords apart = 4 banks apart) then cover the 32 banks once -- and writes each of the
// 8 sample groups' [4][BT] block as one contiguous 4 KB piece with 16-byte stores (a wave reads one whole LDS row: contiguous).
#include <hip/hip_runtime.h>
#include <math.h>
#include "mm_common.h"

#define PWS_THREADS 256
#define PWS_MROWS 16        // k_pw_basis: inducing points per workgroup
#define PWS_TS 32           // k_pw_pack_update: samples per tile (256-byte runs of v)
#define PWS_ROW_BYTES 1040  // LDS row of the tile: BT * sizeof(T) = 1024 bytes + 16 (see above)

template <typename T> struct PwsVec;
template <> struct PwsVec<float> { typedef float4 type; static constexpr int W = 4; };
template <> struct PwsVec<double> { typedef double2 type; static constexpr int W = 2; };

__device__ __forceinline__ void pws_set(float4& o, const double (&x)[4]) { o = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]); }
__device__ __forceinline__ void pws_set(double2& o, const double (&x)[2]) { o = make_double2(x[0], x[1]); }

// grid (ceil(Kp / 256), ceil(M / PWS_MROWS), L); thread = one basis function k of latent l.  DK: d rounded up (registers, static
// indices).  Loads are branch-free: out-of-range indices are clamped to a valid element and the value is replaced afterwards, so
// that a thread's loads are issued together instead of one per guarded block.
template <typename T, int DK>
__global__ __launch_bounds__(PWS_THREADS) void k_pw_basis(int K, int Kp, int M, int d, double inv_two_pi,
                                                          const double* __restrict__ n, const double* __restrict__ b,
                                                          const double* __restrict__ Z, const double* __restrict__ ls,
                                                          const double* __restrict__ var, T* __restrict__ omega_out,
                                                          T* __restrict__ phase_out, double* __restrict__ phiZ) {
  const int k = blockIdx.x * PWS_THREADS + threadIdx.x, l = blockIdx.z;
  if (k >= Kp) return;
  const bool live = k < K;
  const int kc = live ? k : K - 1;
  double om[DK];
#pragma unroll
  for (int j = 0; j < DK; ++j) {
    const int jc = j < d ? j : d - 1;
    const double q = n[((size_t)l * K + kc) * d + jc] / ls[(size_t)l * d + jc];
    om[j] = (live && j < d) ? q : 0.0;
  }
  const double bk = live ? b[(size_t)l * K + kc] : 0.0;
  if (blockIdx.y == 0) {
    // x / (2 pi) as torch evaluates a division by a host scalar on the device: x * (1 / (2 pi)), the reciprocal rounded once
#pragma unroll
    for (int j = 0; j < DK; ++j)
      if (j < d) omega_out[((size_t)l * d + j) * Kp + k] = (T)(om[j] * inv_two_pi);
    phase_out[(size_t)l * Kp + k] = (T)(bk * inv_two_pi);
  }
  if (!live) return;
  const double amp = sqrt(2.0 * var[l] / (double)K);
  const int m0 = blockIdx.y * PWS_MROWS;
  const int m1 = m0 + PWS_MROWS < M ? m0 + PWS_MROWS : M;
  for (int m = m0; m < m1; ++m) {
    const double* __restrict__ z = Z + ((size_t)l * M + m) * d;     // uniform over the workgroup
    double arg = 0.0;
#pragma unroll
    for (int j = 0; j < DK; ++j)
      arg = fma(z[j < d ? j : d - 1], om[j], arg);                  // om[j] = 0 for j >= d: those terms add exactly nothing
    phiZ[((size_t)l * M + m) * K + k] = amp * cos(arg + bk);
  }
}

// prior blocks: grid (G, L); wave sl = sample 4 g + sl; out[g][l][nb][sl][t] = (T) w[4 g + sl][l][nb BT + t]
template <typename T>
__global__ __launch_bounds__(PWS_THREADS) void k_pw_pack_prior(int S, int L, int K, int nbK, int NB,
                                                               const double* __restrict__ w, T* __restrict__ wb) {
  typedef typename PwsVec<T>::type VT;
  constexpr int W = PwsVec<T>::W, BT = 64 * W;
  const int g = blockIdx.x, l = blockIdx.y, sl = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = 4 * g + sl;
  const bool sok = s < S;                                           // uniform over the wave
  const size_t row = ((size_t)(sok ? s : S - 1) * L + l) * K;
  const bool vec = ((size_t)w & 15) == 0 && (row & 1) == 0;         // 16-byte loads: the row starts on a 16-byte boundary
  T* __restrict__ o = wb + (((size_t)g * L + l) * NB * 4 + sl) * BT + lane * W;
  for (int nb = 0; nb < nbK; ++nb, o += 4 * BT) {
    const int k0 = nb * BT + lane * W;
    double x[W];
    if (vec && nb * BT + BT <= K) {                                 // uniform: the whole block lies inside the row
#pragma unroll
      for (int i = 0; i < W; i += 2) {
        const double2 t = *reinterpret_cast<const double2*>(w + row + k0 + i);
        x[i] = t.x; x[i + 1] = t.y;
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const double t = w[row + (k0 + i < K ? k0 + i : K - 1)];
        x[i] = k0 + i < K ? t : 0.0;
      }
    }
    if (!sok) {
#pragma unroll
      for (int i = 0; i < W; ++i) x[i] = 0.0;
    }
    VT out;
    pws_set(out, x);
    *reinterpret_cast<VT*>(o) = out;
  }
}

// update blocks: grid (ceil(G / 8), nbM, L); out[g][l][nbK + nb][sl][t] = (T) v[l][nb BT + t][4 g + sl]
template <typename T>
__global__ __launch_bounds__(PWS_THREADS) void k_pw_pack_update(int S, int L, int M, int G, int nbK, int NB,
                                                                const double* __restrict__ v, T* __restrict__ wb) {
  typedef typename PwsVec<T>::type VT;
  constexpr int W = PwsVec<T>::W, BT = 64 * W;
  constexpr int RG = BT / 4;                                            // groups of 4 consecutive inducing points
  constexpr int QN = PWS_THREADS / PWS_TS;                              // 8 row groups per sweep of the workgroup
  __shared__ __attribute__((aligned(16))) char tile[PWS_TS * PWS_ROW_BYTES];
  const int gb = blockIdx.x, nb = blockIdx.y, l = blockIdx.z;
  const int sx = threadIdx.x & (PWS_TS - 1), q = threadIdx.x / PWS_TS;  // q = 0..7
  const int s = gb * PWS_TS + sx, m0 = nb * BT;
  const bool sok = s < S;
  const double* __restrict__ vs = v + (size_t)l * M * S + (sok ? s : S - 1);
  // two row groups (8 loads of 8 bytes) in flight per thread; out-of-range rows / samples read a valid element and store zero
#pragma unroll 1
  for (int it = 0; it < RG / QN; it += 2) {
    double x[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + 4 * (q + QN * (it + u)) + j;
        x[u][j] = vs[(size_t)(m < M ? m : M - 1) * S];
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int rg = q + QN * (it + u);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!sok || m0 + 4 * rg + j >= M) x[u][j] = 0.0;
      char* dst = tile + sx * PWS_ROW_BYTES + rg * 4 * sizeof(T);
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4((float)x[u][0], (float)x[u][1], (float)x[u][2], (float)x[u][3]);
      } else {
        reinterpret_cast<double2*>(dst)[0] = make_double2(x[u][0], x[u][1]);
        reinterpret_cast<double2*>(dst)[1] = make_double2(x[u][2], x[u][3]);
      }
    }
  }
  __syncthreads();
  const int sl = threadIdx.x >> 6, lane = threadIdx.x & 63;
  VT t[PWS_TS / 4];
#pragma unroll
  for (int gl = 0; gl < PWS_TS / 4; ++gl)
    t[gl] = *reinterpret_cast<const VT*>(tile + (4 * gl + sl) * PWS_ROW_BYTES + lane * 16);
#pragma unroll
  for (int gl = 0; gl < PWS_TS / 4; ++gl) {
    const int g = gb * (PWS_TS / 4) + gl;
    if (g < G)                                                          // uniform
      *reinterpret_cast<VT*>(wb + ((((size_t)g * L + l) * NB + nbK + nb) * 4 + sl) * BT + lane * W) = t[gl];
  }
}

template <typename T, int DK>
static int pws_basis_launch(int L, int K, int M, int d, const double* n, const double* b, const double* Z, const double* ls,
                            const double* var, void* omega_out, void* phase_out, double* phiZ, hipStream_t s) {
  const int BT = 64 * PwsVec<T>::W, Kp = mm_round_up_int(K, BT);
  dim3 grid((Kp + PWS_THREADS - 1) / PWS_THREADS, (M + PWS_MROWS - 1) / PWS_MROWS, L);
  k_pw_basis<T, DK><<<grid, PWS_THREADS, 0, s>>>(K, Kp, M, d, 1.0 / (2.0 * M_PI), n, b, Z, ls, var, (T*)omega_out,
                                                 (T*)phase_out, phiZ);
  return (int)hipGetLastError();
}

template <typename T>
static int pws_basis(int L, int K, int M, int d, const double* n, const double* b, const double* Z, const double* ls,
                     const double* var, void* omega_out, void* phase_out, double* phiZ, hipStream_t s) {
  if (d <= 8) return pws_basis_launch<T, 8>(L, K, M, d, n, b, Z, ls, var, omega_out, phase_out, phiZ, s);
  if (d <= 16) return pws_basis_launch<T, 16>(L, K, M, d, n, b, Z, ls, var, omega_out, phase_out, phiZ, s);
  return pws_basis_launch<T, 32>(L, K, M, d, n, b, Z, ls, var, omega_out, phase_out, phiZ, s);
}

extern "C" int mm_pathwise_basis(int L, int K, int M, int d, int dtype, const double* n, const double* b, const double* Z,
                                 const double* ls, const double* var, void* omega_out, void* phase_out, double* phiZ_out,
                                 void* stream) {
  if (L <= 0 || K <= 0 || M <= 0 || d <= 0 || d > MM_DMAX) return MM_E_DIM;
  if (L > 65535 || (M + PWS_MROWS - 1) / PWS_MROWS > 65535) return MM_E_DIM;      // grid y, z
  if (dtype != MM_F32 && dtype != MM_F64) return MM_E_DTYPE;
  if (!n || !b || !Z || !ls || !var || !omega_out || !phase_out || !phiZ_out) return MM_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_F64) return pws_basis<double>(L, K, M, d, n, b, Z, ls, var, omega_out, phase_out, phiZ_out, s);
  return pws_basis<float>(L, K, M, d, n, b, Z, ls, var, omega_out, phase_out, phiZ_out, s);
}

template <typename T>
static int pws_pack(int S, int L, int K, int M, const double* w, const double* v, void* wb, hipStream_t s) {
  const int BT = 64 * PwsVec<T>::W;
  const int nbK = mm_round_up_int(K, BT) / BT, nbM = mm_round_up_int(M, BT) / BT, NB = nbK + nbM, G = (S + 3) / 4;
  k_pw_pack_prior<T><<<dim3(G, L), PWS_THREADS, 0, s>>>(S, L, K, nbK, NB, w, (T*)wb);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  k_pw_pack_update<T><<<dim3((G + PWS_TS / 4 - 1) / (PWS_TS / 4), nbM, L), PWS_THREADS, 0, s>>>(S, L, M, G, nbK, NB, v, (T*)wb);
  return (int)hipGetLastError();
}

extern "C" int mm_pathwise_pack_stream(int S, int L, int K, int M, int dtype, const double* w, const double* v, void* wb_out,
                                       void* stream) {
  if (S <= 0 || L <= 0 || K <= 0 || M <= 0) return MM_E_DIM;
  if (L > 65535 || (M + 127) / 128 > 65535) return MM_E_DIM;                      // grid y, z
  if (dtype != MM_F32 && dtype != MM_F64) return MM_E_DTYPE;
  if (!w || !v || !wb_out) return MM_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MM_F64) return pws_pack<double>(S, L, K, M, w, v, wb_out, s);
  return pws_pack<float>(S, L, K, M, w, v, wb_out, s);
}
