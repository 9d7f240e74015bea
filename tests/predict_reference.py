"""Reference of the predictive mean and variance for tests/test_predict_host.py and tests/test_gpu_predict.py: the sums

  mean[n][l] = sum_m K_l[m][n] beta_l[m] + c_l,      fvar[n][l] = var_l + sum_ij K_l[i][n] C_l[i][j] K_l[j][n]

in float64 torch on the CPU from ``precompute("cpu")`` with the difference-form Gram of tests/gram_reference.py, and -- the scale the
tolerances are stated in -- the sum of the ABSOLUTE values of each output's terms.  Designs: ``make_svgp(stable=True, mean_c=True)``
with points uniform in [-0.2, 1.2]^d.  Every design handed out satisfies the condition under which a tolerance of 1e-11 x the
absolute-term sum means something for the variance: that bound is at most 1e-6 var_l (asserted here, on the CPU, for every use)."""
import functools

import numpy as np
import torch

from gpflowpilco_amd.synthetic import make_svgp
from tests.gram_reference import gram

F64 = torch.float64


def sums(X, Z, ls, var, beta, C, mean_c):
  """-> dict(mean, fvar, smean, svar) [N, L] for CPU float64 operands (C None: fvar and svar None)."""
  K = gram(X, Z, ls, var)                                                   # [L,M,N]
  c = torch.zeros_like(var) if mean_c is None else mean_c
  out = dict(mean=torch.einsum("lmn,lm->nl", K, beta) + c, smean=torch.einsum("lmn,lm->nl", K, beta.abs()) + c.abs(),
             fvar=None, svar=None)
  if C is not None:
    out["fvar"] = var + torch.einsum("lin,lij,ljn->nl", K, C, K)
    out["svar"] = var + torch.einsum("lin,lij,ljn->nl", K, C.abs(), K)
  return out


@functools.lru_cache(maxsize=None)
def design(L, M, N, d, seed=0):
  """-> (syn, X [N,d], (Z, ls, var, beta, C, mean_c) of ``precompute("cpu")``)."""
  syn = make_svgp(L, M, d, seed=1000 * seed + 7 * L + 3 * M + d, stable=True, mean_c=True)
  rng = np.random.default_rng(5000 + 1000 * seed + 11 * N + d)
  X = torch.tensor(rng.uniform(-0.2, 1.2, size=(N, d)), dtype=F64)
  return syn, X, tuple(t.contiguous() for t in syn.to_model("cpu").precompute("cpu"))


@functools.lru_cache(maxsize=None)
def reference(L, M, N, d, seed=0):
  """The sums of ``design(L, M, N, d, seed)``; asserts the design's condition."""
  _, X, ops6 = design(L, M, N, d, seed)
  ref = sums(X, *ops6)
  worst = float((1e-11 * ref["svar"] / ops6[2]).max())
  assert worst <= 1e-6, f"design {(L, M, N, d, seed)}: 1e-11 x the variance's absolute-term sum is {worst:.2e} var: replace it"
  return ref


# ---- whole models: the oracle's parameters for SVGP.predict_f against oracle.pin_oracle.svgp_predict_f ---------------------------
@functools.lru_cache(maxsize=None)
def model_case(whiten, coreg, L=2, M=40, d=4, N=70, seed=0):
  """-> (oracle SVGPParams, X [N,d] numpy): the ``make_svgp(stable=True)`` posterior, handed over whitened or -- the same
  distribution, u = Lk v -- not whitened; ``coreg``: two latents mixed to P = 3 outputs by a row-normalised W; a Constant mean."""
  from oracle import mm_oracle as mo
  syn = make_svgp(L, M, d, seed=300 + seed + 7 * L + 3 * M + d, stable=True)
  rng = np.random.default_rng(900 + seed)
  q_mu, q_sqrt = syn.q_mu.copy(), syn.q_sqrt.copy()
  if not whiten:
    for a in range(L):
      Lk = np.linalg.cholesky(mo.se_kernel(syn.Z, None, syn.lengthscales[a], syn.variance[a]) + mo.DEFAULT_JITTER * np.eye(M))
      q_mu[:, a], q_sqrt[a] = Lk @ q_mu[:, a], Lk @ q_sqrt[a]
  W = None
  if coreg:
    W = rng.uniform(size=(3, L))
    W = W / np.linalg.norm(W, axis=-1, keepdims=True)
  p = mo.SVGPParams(Z=np.broadcast_to(syn.Z, (L, M, d)).copy(), lengthscales=syn.lengthscales, variance=syn.variance, q_mu=q_mu,
                    q_sqrt=q_sqrt, whiten=whiten, mean_c=0.1 * rng.standard_normal(3 if coreg else L), W=W)
  return p, rng.uniform(-0.2, 1.2, size=(N, d))


def model_reference(p, X, model):
  """For oracle parameters ``p``, points X (numpy) and the CPU model built from ``p``: the oracle's predict_f (mean [N,P],
  cov [N,P,P]), the same from the quadratic form on ``model.precompute("cpu")`` (the second CPU formulation: what the native route
  evaluates), the elementwise gap between the two, and the absolute-term sums of mean, var and cov after the mixing."""
  from oracle import pin_oracle
  mean_o, cov_o = (torch.from_numpy(a) for a in pin_oracle.svgp_predict_f(X, p))
  Z, ls, var, beta, C, _ = model.precompute("cpu")
  s = sums(torch.from_numpy(X), Z, ls, var, beta, C, None)
  L = Z.shape[0]
  W = torch.eye(L, dtype=F64) if p.W is None else torch.from_numpy(p.W)
  c = torch.from_numpy(np.asarray(p.mean_c))
  mix = lambda v: torch.einsum("pl,nl,ql->npq", W, v, W)
  mean_q, cov_q = s["mean"] @ W.T + c, mix(s["fvar"])
  worst = float((1e-11 * s["svar"] / var).max())
  assert worst <= 1e-6, f"1e-11 x the variance's absolute-term sum is {worst:.2e} var: replace the design"
  return dict(mean=mean_o, cov=cov_o, mean_q=mean_q, cov_q=cov_q, gap_mean=(mean_q - mean_o).abs(), gap_cov=(cov_q - cov_o).abs(),
              smean=s["smean"] @ W.abs().T + c.abs(), scov=torch.einsum("pl,nl,ql->npq", W.abs(), s["svar"], W.abs()))
