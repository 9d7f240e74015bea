"""numpy study behind the XCD map of the diagonal f64 sweeps: how unequal the latents of the flagship shape
(C3, BASELINE recipe) are, i.e. what a map that gives every XCD one whole latent costs against one that deals every latent's
tiles over all eight.

On the bench's own draws (every 32nd batch element of steps 0, 7 and 23; rows and columns recentred, points in norm order,
Mp = 2048) it prints, per latent, the mean degree of the e^b tier polynomial over the 32 x 32 wave tiles of the 64 x 64 tiles
it <= jt, and the modelled cost of the heaviest latent over the mean.  Cost of an entry: 32 MFMA cycles + 5 (degree + 2) VALU
cycles; a workgroup (four wave tiles) waits for its slowest wave.  A MODEL of the arithmetic alone: what the GPU said stands
beside it in DESIGN.md 4.5.

  python tools/diag_balance_study.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflowpilco_amd.synthetic import make_inputs, make_svgp
L, M, d, B, H, Mp = 8, 2000, 8, 256, 40, 2048
syn = make_svgp(L, M, d, seed=1002, ls_bounds=(0.3, 3.0), stable=False)
mu_all, S_all = make_inputs(B * H, d, seed=2000 + 1002, scale=0.1, lo=0.0, hi=1.0)
mu_all, S_all = mu_all.reshape(H, B, d), S_all.reshape(H, B, d, d)
Z = np.broadcast_to(syn.Z, (L, M, d)); ls = syn.lengthscales
def deg(t):   # POLYC FMAs per entry by the wave tile's max |b| (mm_f64.hip: the LOWP minimax tiers)
  return np.select([t < 1/64, t < 1/32, t < 1/16, t < 1/8, t < 1/4, t < 3/4], [5, 6, 7, 8, 9, 12], 15)
nt = Mp // 64
iu = np.triu_indices(nt)
Zs = []
for a in range(L):
  zb = Z[a].mean(0)
  o = np.argsort((((Z[a] - zb) / ls[a]) ** 2).sum(1))
  zc = np.zeros((Mp, d)); zc[:M] = Z[a][o] - zb          # (padded rows: zero operands, lowest tier)
  Zs.append(zc)
print("step | mean degree per latent (0 to %d) | all | max / mean of the modelled cost" % (L - 1))
for h in (0, 7, 23):
  dg, cost = np.zeros(L), np.zeros(L)
  nb = 0
  for b in range(0, B, 32):
    S = S_all[h, b]
    nb += 1
    for a in range(L):
      La = ls[a] ** 2; V = La / 2
      T = np.diag(V) @ np.linalg.solve(S + np.diag(V), S); T = 0.5 * (T + T.T)
      G = T / La[:, None] / La[None, :]
      bb = np.abs(Zs[a] @ G @ Zs[a].T)
      t = bb.reshape(nt, 2, 32, nt, 2, 32).max(axis=(2, 5))            # [it][rh][jt][cw]: wave tiles
      dw = deg(t).transpose(0, 2, 1, 3).reshape(nt, nt, 4)[iu]         # the four waves of every visited tile
      dg[a] += dw.mean()
      cost[a] += (32 + 5 * (dw.max(axis=1) + 2)).sum()
  dg /= nb
  print("%4d | %s | %.2f | %.3f" % (h, ", ".join("%.2f" % v for v in dg), dg.mean(), cost.max() / cost.mean()))
