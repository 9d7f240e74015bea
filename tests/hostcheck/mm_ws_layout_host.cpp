// Where the q stage leaves its per-item results in the workspace (csrc/mm_common.h: mm_workspace_layout), for tests that compare
// them to the bit (tests/test_gpu_spoly_loads.py).  Test infrastructure, host code only; nothing in the product loads it.
#include "../../gpflowpilco_amd/csrc/mm_common.h"

// out[0..5] = byte offsets of s12, s56, estS, ilist; the number of off-diagonal pairs Po; the workspace's size
extern "C" int mm_test_ws_offsets(int B, int L, int M, int d, int dtype, int flags, unsigned long long* out) {
  const MMWorkspaceLayout o = mm_workspace_layout(B, L, M, d, dtype, flags);
  out[0] = o.s12; out[1] = o.s56; out[2] = o.estS; out[3] = o.ilist; out[4] = (unsigned long long)o.Po; out[5] = o.total;
  return 0;
}
