// The operands of a pathwise drift as ONE bundle, from the C ABI to the launches (mm_pathwise.hip, mm_pathwise_mean.hip,
// mm_pathwise_policy.hip).  Nearly all of them are const void* or const double*: between functions they travel by NAME, so
// that no call can swap two of them unnoticed.  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include "mm_common.h"

struct MMPwDrift {
  int S = 0, L = 0, M = 0, K = 0, d = 0, dtype = 0, kernel = 0;
  // element type dtype: omega_t [L,d,K], phase [L,K], zs_t [L,d,M], hz [L,M], wb the blocked weight stream
  const void *omega_t = nullptr, *phase = nullptr, *zs_t = nullptr, *hz = nullptr, *wb = nullptr;
  // x_scale [L,d], prior_scale [L], variance [L], mean_c [L] or NULL
  const double *x_scale = nullptr, *prior_scale = nullptr, *variance = nullptr, *mean_c = nullptr;
  // non-NULL: a mean-only drift -- one shared weight vector per latent [L,M] in place of the stream (mm_pathwise_mean.hip);
  // K, omega_t, phase, prior_scale and wb are then not read
  const double* beta = nullptr;
};

// what one evaluation writes: f [S,L], and at most one of jac [S,L,d] (d f / d x, d <= 16) and abs_out [S,L] (the sum of the
// absolute terms).  euler: f is x + dt f (d == L), also written to traj when that is set.  A mean-only drift takes f and jac.
struct MMPwOut {
  void *f = nullptr, *jac = nullptr, *abs_out = nullptr, *traj = nullptr;
  int euler = 0;
  double dt = 0.0;
};

// one evaluation of the drift at x [S,d]: pw_check / pwm_check, the dtype dispatch, and on D.beta the launcher
int mm_pw_drift_eval(const MMPwDrift& D, const void* x, const MMPwOut& o, hipStream_t s);

// mm_pathwise_mean.hip
int pwm_check(int S, int L, int M, int d, int dtype, int kern);
template <typename T>
int pwm_launch(const MMPwDrift& D, const T* x, T* out, T* jac, hipStream_t s);
