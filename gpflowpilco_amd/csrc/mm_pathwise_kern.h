// The basis value of the pathwise update half, shared by the weight-stream pass (mm_pathwise.hip) and the shared-weight mean
// pass (mm_pathwise_mean.hip).  Both take the argument arg = zs . xs - hz - hx = -(log2 e / 2) r^2 of every kernel family.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#ifndef PW_EXP          // overridable for ablation builds (mm_pathwise.hip: PW_COS / PW_EXP)
#define PW_EXP(x_) pw_exp(x_)
#endif

// 2^x: the transcendental unit in f32, ocml in f64
__device__ __forceinline__ float pw_exp(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double pw_exp(double x) { return exp2(x); }

// The kernel family of the update half (KF): 0 SquaredExponential, 1 Matern-3/2, 2 Matern-5/2 (gpflow's parametrisation).
// The stream's argument is arg = zs . xs - hz - hx = -(log2 e / 2) r^2 for every family; pw_kern returns
//   e = k(r) / var  and  g = -k'(r) / (var r)   (SE: g = e; Matern-3/2: 3 e^-s, s = sqrt3 r; Matern-5/2: 5/3 (1 + s) e^-s, s = sqrt5 r)
// so that d e / d x_k = ln2 g (c_k - xscale_k^2 x_k) for all three.  With q = s log2 e = sqrt(4 nu log2 e (-arg)) the
// exponential is a bare 2^-q; -arg is clamped at 0 (expanded form: a sample on an inducing point gives a tiny negative r^2).
__device__ __forceinline__ float pw_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double pw_sqrt(double x) { return sqrt(x); }
template <int KF, typename T>
__device__ __forceinline__ void pw_kern(T arg, T& e, T& g) {
  if constexpr (KF == 0) {
    e = PW_EXP(arg); g = e;
  } else {
    // q = log2 e sqrt(2 nu) r, r^2 = -2 ln2 arg  =>  q^2 = 4 nu log2 e (-arg)
    constexpr double c2 = (KF == 1 ? 6.0 : 10.0) * 1.4426950408889634;
    const T q = pw_sqrt((T)c2 * (arg < (T)0 ? -arg : (T)0));
    const T p = PW_EXP(-q);
    const T sq = (T)0.6931471805599453 * q;                  // s = sqrt(2 nu) r
    if constexpr (KF == 1) {
      e = ((T)1 + sq) * p; g = (T)3 * p;
    } else {
      e = ((T)1 + sq + (T)(1.0 / 3.0) * sq * sq) * p; g = (T)(5.0 / 3.0) * ((T)1 + sq) * p;
    }
  }
}
