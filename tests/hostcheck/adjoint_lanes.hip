// The Ctx-templated adjoint code of csrc/mm_adjoint.h, mm_adjoint_nd.h and mm_mix.h at the DEVICE's lane counts, on the CPU -- TEST
// INFRASTRUCTURE ONLY: a stand-alone program (tests/test_adjoint_lanes.py builds it three times -- plain, address + undefined-behaviour
// sanitizers, thread sanitizer -- and runs it; nothing is loaded into Python, nothing under gpflowpilco_amd/ links it).
//
// MMATeamCtx runs one host thread per lane: lane() / nl() come from the team, sync() is a pthread barrier.  Every function runs with the
// lane count(s) its kernels are launched with (64: the tail / mixing kernels; 256: the policy head and the GP item kernels; 256 and 512:
// k_pair_agg), on operands, outputs and scratch allocated on the heap at EXACTLY their documented sizes -- scratch exactly
// mma_*_scratch(..., nl) doubles -- with scratch and every ASSIGNED output filled with NaN, and again on MMAHostCtx (one lane).  A missing
// barrier is then a ThreadSanitizer report, a short size formula an AddressSanitizer report, scratch read before it is written a NaN.
//
// Agreement with the one-lane result:
//   BIT-EQUAL where every output entry is formed by one lane in a fixed order whatever the lane count: mma_mm, mma_spd_inverse,
//     mma_solve_pivot, mma_encode_bwd, mma_cost_bwd, mma_step_bwd(_nd), mma_head_bwd(_nd), mma_pair_poly, mma_pair_convert(_rows),
//     mma_mix_fwd / _bwd, the tail and pair-aggregate sequences -- and the functions below at shapes where every slice count is 1;
//   otherwise (sums over the centres split into nl / M sub-sweeps or nl / (1 + d + d^2) slices: mma_policy_small_bwd, mma_policy_pair_bwd,
//     mma_policy_nd_bwd, mma_raw_moments, mma_gp_item_moments, mma_gp_item_bwd, the policy-head sequences) within the tolerance and
//     scale the Python host test of the function asserts against autograd: 2e-10 of the largest entry per group for the policy
//     (tests/test_adjoint_host.py, tests/test_adjoint_nd_host.py), 1e-10 for the GP items (tests/test_adjoint_host.py).
//
// usage: adjoint_lanes [--only FN] [--no-sync FN] [--short-scratch FN]
//   --no-sync FN        FN's cases alone, with sync() a no-op            (the thread-sanitizer build must report a race)
//   --short-scratch FN  FN's cases alone, scratch one double too short   (the address-sanitizer build must report an overflow)
// Prints one line per (function, lane count, shape) case and "cases: N"; exit status 1 on any mismatch, non-finite output or ok == false.
#include <pthread.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "../../gpflowpilco_amd/csrc/mm_mix.h"
#include "../../gpflowpilco_amd/csrc/mm_adjoint_lds.h"

typedef std::vector<double> V;
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

// ---- the threaded execution context ------------------------------------------------------------------------------------------------
struct Team {
  int nl; bool nosync; pthread_barrier_t bar;
  Team(int n, bool ns) : nl(n), nosync(ns) { pthread_barrier_init(&bar, nullptr, (unsigned)n); }
  ~Team() { pthread_barrier_destroy(&bar); }
};
struct MMATeamCtx {
  Team* t; int ln;
  __host__ __device__ void stamp(int) const {}
  __host__ __device__ int lane() const { return ln; }
  __host__ __device__ int nl() const { return t->nl; }
  __host__ __device__ void sync() const {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!t->nosync) pthread_barrier_wait(&t->bar);
#endif
  }
  __host__ __device__ int group() const { return 0; }
  __host__ __device__ int ngroups() const { return 1; }
};

// nl threads that live for the whole program (starting 256 threads per case costs more than the cases): a job starts and ends at
// a barrier with the caller, which orders it against the caller's accesses exactly as starting and joining the threads would
struct Pool {
  int nl; bool quit = false; pthread_barrier_t go, done; std::function<void(int)> job; std::vector<std::thread> th;
  explicit Pool(int n) : nl(n) {
    pthread_barrier_init(&go, nullptr, (unsigned)n + 1); pthread_barrier_init(&done, nullptr, (unsigned)n + 1);
    for (int l = 0; l < n; ++l)
      th.emplace_back([this, l] {
        for (;;) { pthread_barrier_wait(&go); if (quit) return; job(l); pthread_barrier_wait(&done); }
      });
  }
  void run(std::function<void(int)> j) { job = std::move(j); pthread_barrier_wait(&go); pthread_barrier_wait(&done); }
  ~Pool() { quit = true; pthread_barrier_wait(&go); for (auto& x : th) x.join(); pthread_barrier_destroy(&go); pthread_barrier_destroy(&done); }
};
static std::vector<std::unique_ptr<Pool>> g_pools;
static Pool& pool(int nl) {
  for (auto& p : g_pools) if (p->nl == nl) return *p;
  g_pools.emplace_back(new Pool(nl));
  return *g_pools.back();
}

struct Run {
  int nl; bool nosync; int shorten;
  // f(ctx) on every lane of a team of nl threads; nl == 1: the one-lane reference on MMAHostCtx
  template <class F> void operator()(F f) const {
    if (nl == 1) { f(MMAHostCtx()); return; }
    Team t(nl, nosync);
    pool(nl).run([&t, &f](int l) { f(MMATeamCtx{&t, l}); });
  }
  V scratch(int n) const { return V((size_t)(n > shorten ? n - shorten : 0), kNaN); }
};

// ---- inputs ------------------------------------------------------------------------------------------------------------------------
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 12345u) { u(); u(); }
  double u() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
  V vec(size_t n, double lo = -1.0, double hi = 1.0) { V v(n); for (auto& x : v) x = lo + (hi - lo) * u(); return v; }
  V spd(int n, double diag = 0.5) {                    // R R^T / n + diag I
    V R = vec((size_t)n * n), S((size_t)n * n);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) {
      double a = i == j ? diag : 0.0;
      for (int k = 0; k < n; ++k) a += R[i * n + k] * R[j * n + k] / n;
      S[i * n + j] = a;
    }
    return S;
  }
};
static V nanv(size_t n) { return V(n, kNaN); }
static V minus(const V& v, double c) { V o(v); for (auto& x : o) x -= c; return o; }
static V slice(const V& v, size_t a, size_t b) { return V(v.begin() + (long)a, v.begin() + (long)b); }
static std::string fmt(const char* f, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int g = 0) {
  char buf[160]; snprintf(buf, sizeof buf, f, a, b, c, d, e, g); return buf;
}
static MMComposeDims make_dims(int nx, int na, int nu) {
  int32_t act[MMC_NA] = {0};
  for (int i = 0; i < na; ++i) act[i] = nx - 1 - i;            // distinct, not sorted
  MMComposeDims D;
  if (mm_compose_dims_nd(nx, na, nu, act, D) != 0) { fprintf(stderr, "bad dims %d %d %d\n", nx, na, nu); exit(2); }
  return D;
}

// ---- outputs and their comparison --------------------------------------------------------------------------------------------------
struct Out { std::string name; V v; double tol; bool unit; };   // tol 0: bit-equal; unit: |got - want| < tol max(1, |want|) per entry;
typedef std::vector<Out> Outs;                                 // else max |got - want| < tol max |want|
static Out bits(const char* n, const V& v) { return Out{n, v, 0.0, false}; }
static Out rel(const char* n, const V& v, double tol) { return Out{n, v, tol, false}; }

static const char *g_only = nullptr, *g_nosync = nullptr, *g_short = nullptr;
static int g_cases = 0, g_fail = 0;
static std::atomic<int> g_notok{0};

static void fail(const char* fn, int nl, const std::string& shape, const std::string& what) {
  ++g_fail;
  printf("FAIL %s nl=%d %s: %s\n", fn, nl, shape.c_str(), what.c_str());
}

static void check(const char* fn, int nl, const std::string& shape, const std::function<Outs(const Run&)>& body) {
  const char* pick = g_nosync ? g_nosync : g_short ? g_short : g_only;
  if (pick && strcmp(pick, fn) != 0) return;
  const Run team{nl, g_nosync != nullptr, g_short ? 1 : 0}, host{1, false, 0};
  g_notok = 0;
  const Outs got = body(team), want = body(host);
  const int before = g_fail;
  if (g_notok.load()) fail(fn, nl, shape, "ok == false on SPD inputs");
  if (got.size() != want.size()) fail(fn, nl, shape, "output count");
  for (size_t o = 0; o < got.size() && o < want.size(); ++o) {
    const Out &g = got[o], &w = want[o];
    if (g.v.size() != w.v.size()) { fail(fn, nl, shape, g.name + ": size"); continue; }
    double md = 0.0, mw = 0.0; bool finite = true, same = true, unit_ok = true;
    for (size_t i = 0; i < g.v.size(); ++i) {
      if (!std::isfinite(g.v[i]) || !std::isfinite(w.v[i])) finite = false;
      if (memcmp(&g.v[i], &w.v[i], sizeof(double)) != 0) same = false;
      const double dlt = fabs(g.v[i] - w.v[i]);
      md = fmax(md, dlt); mw = fmax(mw, fabs(w.v[i]));
      if (!(dlt < g.tol * fmax(1.0, fabs(w.v[i])))) unit_ok = false;
    }
    char buf[200];
    snprintf(buf, sizeof buf, "%s: max |diff| %.3e, max |want| %.3e, tol %.1e", g.name.c_str(), md, mw, g.tol);
    if (!finite) fail(fn, nl, shape, g.name + ": not finite");
    else if (g.tol == 0.0) { if (!same) fail(fn, nl, shape, std::string("not bit-equal, ") + buf); }
    else if (g.unit) { if (!unit_ok) fail(fn, nl, shape, buf); }
    else if (!same && !(md < g.tol * fmax(mw, 1e-300))) fail(fn, nl, shape, buf);
  }
  ++g_cases;
  printf("case %s nl=%d %s %s\n", fn, nl, shape.c_str(), g_fail == before ? "ok" : "FAILED");
  fflush(stdout);
}

// value returned in every lane: all lanes must agree bit for bit
static Out lanes_value(const char* n, const V& ret) {
  V v(1, ret[0]);
  for (double r : ret) if (memcmp(&r, &ret[0], sizeof(double)) != 0) v[0] = kNaN;
  return bits(n, v);
}

// ---- the dense helpers ---------------------------------------------------------------------------------------------------------------
static void cases_dense() {
  const int mm[][3] = {{1, 1, 1}, {3, 3, 3}, {8, 8, 8}, {16, 16, 16}, {17, 5, 16}};     // n m: below / at / above 256 entries
  for (auto& s : mm) {
    const int n = s[0], k = s[1], m = s[2];
    check("mma_mm", 256, fmt("n%d k%d m%d", n, k, m), [=](const Run& run) {
      Rng r(100 + n * 31 + m);
      const int lda = k + 1, ldb = m + 1, ldc = m + 1;
      const V A = r.vec((size_t)(n - 1) * lda + k), B = r.vec((size_t)(k - 1) * ldb + m);
      V C = nanv((size_t)(n - 1) * ldc + m), out;
      run([&](auto c) { mma_mm(c, n, k, m, A.data(), lda, B.data(), ldb, C.data(), ldc); });
      for (int i = 0; i < n; ++i) for (int j = 0; j < m; ++j) out.push_back(C[i * ldc + j]);
      return Outs{bits("C", out)};
    });
  }
  for (int d : {1, 3, 8, 16, 17}) {                                                     // d^2 below and above 256
    check("mma_spd_inverse", 256, fmt("d%d", d), [=](const Run& run) {
      Rng r(200 + d);
      const int dp = d + 1;
      const V S = r.spd(d);
      V A = nanv((size_t)d * dp), Y = nanv((size_t)d * dp), ret((size_t)run.nl, kNaN), out;
      for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) A[i * dp + j] = S[i * d + j];
      run([&](auto c) { bool ok = true; ret[c.lane()] = mma_spd_inverse(c, A.data(), Y.data(), d, dp, &ok); if (!ok) g_notok = 1; });
      for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) out.push_back(A[i * dp + j]);
      return Outs{bits("inverse", out), lanes_value("logdet", ret)};
    });
  }
  const int sp[][2] = {{1, 1}, {3, 3}, {5, 2}, {8, 8}, {9, 9}, {16, 16}, {24, 24}};     // (n - 1)(n + nr - 1) below and above 64
  for (auto& s : sp) {
    const int n = s[0], nr = s[1];
    check("mma_solve_pivot", 64, fmt("n%d nr%d", n, nr), [=](const Run& run) {
      Rng r(300 + n * 7 + nr);
      const int ld = n + nr;
      V Aug = r.vec((size_t)n * ld), ret((size_t)run.nl, kNaN);                         // no dominant diagonal: rows are exchanged
      run([&](auto c) { ret[c.lane()] = mma_solve_pivot(c, Aug.data(), n, nr, ld); });
      return Outs{bits("Aug", Aug), lanes_value("det", ret)};
    });
  }
}

// ---- the composed step: encode, cost, step ---------------------------------------------------------------------------------------------
static const int kEnc[][2] = {{1, 0}, {1, 1}, {5, 0}, {5, 1}, {5, 5}, {16, 0}, {16, 1}, {16, 8}};     // (nx, na)

static void cases_step() {
  for (auto& s : kEnc) {
    const int nx = s[0], na = s[1];
    check("mma_encode_bwd", 64, fmt("nx%d na%d", nx, na), [=](const Run& run) {
      Rng r(400 + nx * 9 + na);
      const MMComposeDims D = make_dims(nx, na, 1);
      const int ne = D.ne;
      const V m = r.vec(nx), S = r.spd(nx), gme = r.vec(ne), gSee = r.vec((size_t)ne * ne), gSxe = r.vec((size_t)nx * ne);
      V gm(nx, 0.25), gS((size_t)nx * nx, -0.5), sm = run.scratch(mma_encode_bwd_scratch(nx, na));
      run([&](auto c) { mma_encode_bwd(c, D, m.data(), S.data(), gme.data(), gSee.data(), gSxe.data(), gm.data(), gS.data(), sm.data()); });
      return Outs{bits("gm", gm), bits("gS", gS)};
    });
    check("mma_step_bwd", 64, fmt("nx%d na%d", nx, na), [=](const Run& run) {
      Rng r(500 + nx * 9 + na);
      const MMComposeDims D = make_dims(nx, na, 1);
      const int ne = D.ne, nd = D.nd;
      const V Sxe = r.vec((size_t)nx * ne), cp = r.vec(ne), Sdd = r.vec((size_t)nd * nd), dcross = r.vec((size_t)nd * nx),
              gm1 = r.vec(nx), gS1 = r.vec((size_t)nx * nx);
      V gSxe = nanv((size_t)nx * ne), gcp = nanv(ne), gSdd = nanv((size_t)nd * nd), gdf1 = nanv(nx), gdSff = nanv((size_t)nx * nx),
        gdcross = nanv((size_t)nd * nx), sm = run.scratch(mma_step_bwd_scratch(nx, nd));
      run([&](auto c) {
        mma_step_bwd(c, D, 0.1, Sxe.data(), cp.data(), Sdd.data(), dcross.data(), gm1.data(), gS1.data(), gSxe.data(), gcp.data(),
                     gSdd.data(), gdf1.data(), gdSff.data(), gdcross.data(), sm.data());
      });
      return Outs{bits("gSxe", gSxe), bits("gcp", gcp), bits("gSdd", gSdd), bits("gdf1", gdf1), bits("gdSff", gdSff), bits("gdcross", gdcross)};
    });
  }
  for (int n : {1, 5, 9, 16, 24}) {                                                     // n^2 below and above 64; 24 = the widest ne
    check("mma_cost_bwd", 64, fmt("n%d", n), [=](const Run& run) {
      Rng r(600 + n);
      const V mean = r.vec(n), cov = r.spd(n), target = r.vec(n), W = r.spd(n);
      V gmean(n, 0.25), gcov((size_t)n * n, -0.5), sm = run.scratch(mma_cost_bwd_scratch(n)), ret((size_t)run.nl, kNaN);
      run([&](auto c) {
        ret[c.lane()] = mma_cost_bwd(c, n, mean.data(), cov.data(), target.data(), W.data(), 0.7, gmean.data(), gcov.data(), sm.data());
      });
      return Outs{bits("gmean", gmean), bits("gcov", gcov), lanes_value("cost", ret)};
    });
  }
  const int nds[][3] = {{1, 0, 1}, {5, 1, 2}, {5, 5, 4}, {16, 0, 2}, {16, 1, 1}, {16, 8, 4}};  // (nx, na, nu)
  for (auto& s : nds) {
    const int nx = s[0], na = s[1], nu = s[2];
    check("mma_step_bwd_nd", 64, fmt("nx%d na%d nu%d", nx, na, nu), [=](const Run& run) {
      Rng r(700 + nx * 9 + na * 5 + nu);
      const MMComposeDims D = make_dims(nx, na, nu);
      const int ne = D.ne, nd = D.nd;
      const V Sxe = r.vec((size_t)nx * ne), cp = r.vec((size_t)ne * nu), Sdd = r.vec((size_t)nd * nd), dcross = r.vec((size_t)nd * nx),
              gm1 = r.vec(nx), gS1 = r.vec((size_t)nx * nx);
      V gSxe = nanv((size_t)nx * ne), gcp = nanv((size_t)ne * nu), gSdd = nanv((size_t)nd * nd), gdf1 = nanv(nx),
        gdSff = nanv((size_t)nx * nx), gdcross = nanv((size_t)nd * nx), sm = run.scratch(mma_step_bwd_scratch(nx, nd));
      run([&](auto c) {
        mma_step_bwd_nd(c, D, 0.1, Sxe.data(), cp.data(), Sdd.data(), dcross.data(), gm1.data(), gS1.data(), gSxe.data(), gcp.data(),
                        gSdd.data(), gdf1.data(), gdSff.data(), gdcross.data(), sm.data());
      });
      return Outs{bits("gSxe", gSxe), bits("gcp", gcp), bits("gSdd", gSdd), bits("gdf1", gdf1), bits("gdSff", gdSff), bits("gdcross", gdcross)};
    });
  }
}

// ---- the NormalCDF heads -------------------------------------------------------------------------------------------------------------
static void cases_head() {
  const int hs[][2] = {{1, 1}, {5, 1}, {5, -1}, {8, 1}};                                 // (ne, sign of pSff)
  for (auto& s : hs) {
    const int ne = s[0], sg = s[1];
    check("mma_head_bwd", 256, fmt("ne%d pSff%+d", ne, sg), [=](const Run& run) {
      Rng r(800 + ne * 3 + sg);
      const int nd = ne + 1;
      const V pcross = r.vec(ne), See = r.spd(ne), gmd = r.vec(nd), gSdd = r.vec((size_t)nd * nd), gcp = r.vec(ne);
      V gme = nanv(ne), gSee = nanv((size_t)ne * ne), gpc = nanv(ne), sm = run.scratch(ne + 4);
      run([&](auto c) {
        mma_head_bwd(c, ne, 2.0, -0.5, 0.3, 0.4 * sg, pcross.data(), See.data(), gmd.data(), gSdd.data(), gcp.data(), gme.data(),
                     gSee.data(), gpc.data(), sm.data());
      });
      return Outs{bits("gme", gme), bits("gSee", gSee), bits("gpcross", gpc), bits("gpf1 gpSff", slice(sm, ne, ne + 2))};
    });
  }
  const int hn[][2] = {{1, 1}, {5, 2}, {8, 4}, {16, 1}, {16, 4}};                        // (ne, nu): ne^2, ne nu below and above 256
  for (auto& s : hn) {
    const int ne = s[0], nu = s[1];
    check("mma_head_bwd_nd", 256, fmt("ne%d nu%d", ne, nu), [=](const Run& run) {
      Rng r(900 + ne * 5 + nu);
      const int nd = ne + nu;
      const V scale = r.vec(nu, 0.5, 2.0), shift = r.vec(nu), pf1 = r.vec(nu), pSff = r.spd(nu), pcross = r.vec((size_t)ne * nu),
              See = r.spd(ne), gmd = r.vec(nd), gSdd = r.vec((size_t)nd * nd), gcp = r.vec((size_t)ne * nu);
      V gme = nanv(ne), gSee = nanv((size_t)ne * ne), gpc = nanv((size_t)ne * nu), gpf1 = nanv(nu), gpS = nanv((size_t)nu * nu),
        sm = run.scratch(mma_head_bwd_nd_scratch(ne, nu));
      run([&](auto c) {
        mma_head_bwd_nd(c, ne, nu, scale.data(), shift.data(), pf1.data(), pSff.data(), pcross.data(), See.data(), gmd.data(), gSdd.data(),
                        gcp.data(), gme.data(), gSee.data(), gpc.data(), gpf1.data(), gpS.data(), sm.data());
      });
      return Outs{bits("gme", gme), bits("gSee", gSee), bits("gpcross", gpc), bits("gpf1", gpf1), bits("gpSff", gpS)};
    });
  }
}

// ---- the policy match ------------------------------------------------------------------------------------------------------------------
struct Policy { int nu, M, d; V Z, beta, ls2, var, mu, Sigma; };
static Policy make_policy(Rng& r, int nu, int M, int d) {
  Policy p{nu, M, d, r.vec((size_t)nu * M * d), r.vec((size_t)nu * M), r.vec((size_t)nu * d, 0.5, 1.5), r.vec(nu, 0.5, 1.5),
           r.vec(d, -0.5, 0.5), r.spd(d, 0.3)};
  return p;
}
static const double kPolTol = 2e-10;        // tests/test_adjoint_host.py, tests/test_adjoint_nd_host.py: tol of the policy match
static const double kParFill = 0.125;       // what the ACCUMULATED packed gradient starts from
static bool policy_one_slice(int M, int d, int nl) { return mma_policy_nsub(M, nl) == 1 && nl / (d * d + 2 * d + 2) <= 1; }

// the groups of one latent's packed gradient, as the Python tests compare them: dZ, dbeta, 2 ls dls2, dvar, dmean
static void par_groups(Outs& o, const char* tag, const V& gpar, size_t off, int M, int d, const double* ls2, double tol) {
  const size_t Md = (size_t)M * d;
  const V g = minus(slice(gpar, off, off + Md + M + d + 2), kParFill);
  V dls = slice(g, Md + M, Md + M + d);
  for (int k = 0; k < d; ++k) dls[k] *= 2.0 * sqrt(ls2[k]);
  const std::string t(tag);
  o.push_back(Out{t + ".dZ", slice(g, 0, Md), tol, false});
  o.push_back(Out{t + ".dbeta", slice(g, Md, Md + M), tol, false});
  o.push_back(Out{t + ".dls", dls, tol, false});
  o.push_back(Out{t + ".dvar dmean", slice(g, Md + M + d, Md + M + d + 2), tol, true});
}

static void cases_policy() {
  // M: nl / M > 1 (sub-sweeps), = 1, M > nl;  d: d^2 + 2 d + 2 below 256 (slices) and above (15: 257, 16: 290)
  const int sm_[][2] = {{1, 1}, {3, 3}, {64, 8}, {128, 4}, {256, 2}, {257, 3}, {13, 15}, {3, 16}};
  for (auto& s : sm_) {
    const int M = s[0], d = s[1];
    check("mma_policy_small_bwd", 256, fmt("M%d d%d", M, d), [=](const Run& run) {
      Rng r(1000 + M * 17 + d);
      const Policy p = make_policy(r, 1, M, d);
      const V gcross = r.vec(d);
      const double tol = policy_one_slice(M, d, run.nl) ? 0.0 : kPolTol;
      V gmu = nanv(d), gSig = nanv((size_t)d * d), gpar((size_t)M * d + M + d + 2, kParFill),
        sm = run.scratch(mma_policy_small_bwd_scratch(M, d, run.nl));
      run([&](auto c) {
        bool ok = true;
        mma_policy_small_bwd<decltype(c), 8>(c, M, d, p.Z.data(), p.beta.data(), p.ls2.data(), p.var[0], p.mu.data(), p.Sigma.data(), 0.6,
                                             -0.4, gcross.data(), gmu.data(), gSig.data(), gpar.data(), sm.data(), &ok);
        if (!ok) g_notok = 1;
      });
      Outs o{rel("gmu", gmu, tol), rel("gSig", gSig, tol)};
      par_groups(o, "gpar", gpar, 0, M, d, p.ls2.data(), tol);
      return o;
    });
  }
  const int pr[][2] = {{1, 1}, {3, 3}, {64, 8}, {257, 2}, {5, 16}};
  for (auto& s : pr) {
    const int M = s[0], d = s[1];
    check("mma_policy_pair_bwd", 256, fmt("M%d d%d", M, d), [=](const Run& run) {
      Rng r(1100 + M * 17 + d);
      const Policy p = make_policy(r, 2, M, d);
      const size_t Md = (size_t)M * d, glen = Md + M + d + 2;
      const double tol = mma_policy_nsub(M, run.nl) == 1 ? 0.0 : kPolTol;
      V gmu(d, 0.25), gSig((size_t)d * d, -0.5), gpa(glen, kParFill), gpb(glen, kParFill),
        sm = run.scratch(mma_policy_pair_bwd_scratch(M, d, run.nl));
      run([&](auto c) {
        bool ok = true;
        mma_policy_pair_bwd(c, M, d, p.Z.data(), p.beta.data(), p.ls2.data(), p.var[0], p.Z.data() + Md, p.beta.data() + M,
                            p.ls2.data() + d, p.var[1], p.mu.data(), p.Sigma.data(), 0.7, gmu.data(), gSig.data(), gpa.data(), gpb.data(),
                            sm.data(), &ok);
        if (!ok) g_notok = 1;
      });
      Outs o{rel("gmu", minus(gmu, 0.25), tol), rel("gSig", minus(gSig, -0.5), tol)};
      par_groups(o, "gpa", gpa, 0, M, d, p.ls2.data(), tol);
      par_groups(o, "gpb", gpb, 0, M, d, p.ls2.data() + d, tol);
      return o;
    });
  }
  const int nd_[][3] = {{1, 3, 3}, {2, 64, 5}, {4, 3, 8}, {3, 257, 2}, {2, 5, 16}};      // (nu, M, d)
  for (auto& s : nd_) {
    const int nu = s[0], M = s[1], d = s[2];
    check("mma_policy_nd_bwd", 256, fmt("nu%d M%d d%d", nu, M, d), [=](const Run& run) {
      Rng r(1200 + nu * 101 + M * 17 + d);
      const Policy p = make_policy(r, nu, M, d);
      const size_t glen = (size_t)M * d + M + d + 2;
      const V gf1 = r.vec(nu), gSff = r.vec((size_t)nu * nu), gcross = r.vec((size_t)d * nu);
      const double tol = policy_one_slice(M, d, run.nl) ? 0.0 : kPolTol;
      V gmu = nanv(d), gSig = nanv((size_t)d * d), gpar((size_t)nu * glen, kParFill), sm = run.scratch(mma_policy_nd_bwd_scratch(M, d, run.nl));
      run([&](auto c) {
        bool ok = true;
        mma_policy_nd_bwd<decltype(c), 8>(c, nu, M, d, p.Z.data(), p.beta.data(), p.ls2.data(), p.var.data(), p.mu.data(), p.Sigma.data(),
                                          gf1.data(), gSff.data(), gcross.data(), gmu.data(), gSig.data(), gpar.data(), sm.data(), &ok);
        if (!ok) g_notok = 1;
      });
      Outs o{rel("gmu", gmu, tol), rel("gSig", gSig, tol)};
      for (int a = 0; a < nu; ++a) par_groups(o, fmt("gpar[%d]", a).c_str(), gpar, a * glen, M, d, p.ls2.data() + (size_t)a * d, tol);
      return o;
    });
  }
}

// ---- the off-diagonal pair aggregates (k_pair_agg: 512 lanes on its own, 256 beside the diagonal sweep) ----------------------------------
static void cases_pair() {
  std::vector<short> rtab((8 * 8 * 8 * 8 * 8 - 8) / 7, 0);                               // MMModelLayout::rtab: ranks of DK = 8 index tuples
  for (int k = 1; k <= 4; ++k)
    for (int pos = 0; pos < (1 << (3 * k)); ++pos)
      rtab[(size_t)(((1 << (3 * k)) - 8) / 7 + pos)] =
          (short)mm_mono_rank_unsorted(pos & 7, (pos >> 3) & 7, (pos >> 6) & 7, (pos >> 9) & 7, k);
  for (int nl : {256, 512}) {
    const int pp[][2] = {{1, 0}, {3, 0}, {3, 1}, {8, 0}, {8, 1}};                        // (d, ranks from the table): d^4 below and above nl
    for (auto& s : pp) {
      const int d = s[0], tab = s[1];
      check("mma_pair_poly", nl, fmt("d%d rtab%d", d, tab), [=, &rtab](const Run& run) {
        Rng r(1300 + d * 3 + tab);
        const int nm = mm_mono_off(5, d);
        const V G = r.vec((size_t)d * d, -0.3, 0.3), dmu = r.vec(d), mR = r.vec(nm), mC = r.vec(nm);
        V T = nanv(mma_pair_agg_len(d)), sm = run.scratch(mma_pair_poly_scratch(d));
        run([&](auto c) { mma_pair_poly(c, d, G.data(), dmu.data(), mR.data(), mC.data(), T.data(), sm.data(), tab ? rtab.data() : nullptr); });
        return Outs{bits("T", T)};
      });
    }
    for (int d : {1, 3, 8}) {
      check("mma_pair_convert", nl, fmt("d%d", d), [=](const Run& run) {
        Rng r(1400 + d);
        const V dmu2 = r.vec(d);
        V T = r.vec(mma_pair_agg_len(d));
        run([&](auto c) { mma_pair_convert(c, d, dmu2.data(), T.data()); });
        return Outs{bits("T", T)};
      });
      check("mma_pair_convert_rows", nl, fmt("d%d", d), [=](const Run& run) {
        Rng r(1500 + d);
        const V dmu = r.vec(d);
        V T = r.vec(mma_pair_agg_len(d));
        run([&](auto c) { mma_pair_convert_rows(c, d, dmu.data(), T.data()); });
        return Outs{bits("T", T)};
      });
    }
  }
}

// ---- the drift's match: moments and items ------------------------------------------------------------------------------------------------
static const double kGpTol = 1e-10;         // tests/test_adjoint_host.py: the GP match's adjoint against autograd

struct GP {
  int L, M, Mp, d, full, unc, P, Po;
  V Z, ls2, mu, Sigma, latmat, w, q, col, colL, row, pagg, f1raw, g_f1, g_Sff, g_cross;
  std::unique_ptr<double[]> empty;           // a zero-length allocation: `row` where it is not read
};
static void pad_nan(V& v, int rows, int M, int Mp) { for (int r = 0; r < rows; ++r) for (int m = M; m < Mp; ++m) v[(size_t)r * Mp + m] = kNaN; }
static GP make_gp(Rng& r, int L, int M, int Mp, int d, int full, int unc) {
  GP g;
  g.L = L; g.M = M; g.Mp = Mp; g.d = d; g.full = full; g.unc = unc; g.P = full ? L * (L + 1) / 2 : L; g.Po = g.P - L;
  g.Z = r.vec((size_t)L * M * d); g.ls2 = r.vec((size_t)L * d, 0.5, 1.5); g.mu = r.vec(d, -0.5, 0.5); g.Sigma = r.spd(d, 0.3);
  const int lat = 2 * d * d + 2, dp = d + 1;
  g.latmat = nanv((size_t)L * lat);                                       // P_a = (Sigma + Lambda_a)^-1; the rest of the slab is not read
  for (int a = 0; a < L; ++a) {
    V A((size_t)d * dp, 0.0), Y((size_t)d * dp, 0.0);
    for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) A[i * dp + j] = g.Sigma[i * d + j] + (i == j ? g.ls2[(size_t)a * d + i] : 0.0);
    bool ok = true;
    mma_spd_inverse(MMAHostCtx(), A.data(), Y.data(), d, dp, &ok);
    for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) g.latmat[(size_t)a * lat + i * d + j] = A[i * dp + j];
  }
  g.w = r.vec((size_t)L * Mp); g.q = r.vec((size_t)L * Mp, 0.1, 1.0);
  g.col = r.vec((size_t)g.P * (3 + d) * Mp); g.row = r.vec((size_t)g.Po * 2 * Mp);
  pad_nan(g.w, L, M, Mp); pad_nan(g.q, L, M, Mp); pad_nan(g.col, g.P * (3 + d), M, Mp); pad_nan(g.row, g.Po * 2, M, Mp);
  g.colL = slice(g.col, 0, (size_t)L * (3 + d) * Mp);
  g.pagg = r.vec((size_t)g.Po * mma_pair_agg_len(d)); g.f1raw = r.vec(L);
  g.g_f1 = r.vec(L); g.g_Sff = r.vec(full ? (size_t)L * L : (size_t)L); g.g_cross = r.vec((size_t)d * L);
  g.empty.reset(new double[0]);
  return g;
}
static bool gp_needs_moments(const GP& g, int item, bool agg) { return item < g.L || !(agg && item - g.L >= g.L); }

// mma_gp_item_moments over chunks of `chunk` centres, for every item that needs moments: pre[item] = [nchunk][3 nc]
static std::vector<V> gp_moments(const Run& run, const GP& g, int chunk, bool agg) {
  const int nc = mma_gp_ncol(g.d), nchunk = (g.M + chunk - 1) / chunk;
  std::vector<V> pre((size_t)(g.L + g.P));
  for (int item = 0; item < g.L + g.P; ++item) {
    if (!gp_needs_moments(g, item, agg)) continue;
    pre[item] = nanv((size_t)nchunk * 3 * nc);
    for (int ch = 0; ch < nchunk; ++ch) {
      const int m0 = ch * chunk, m1 = std::min(g.M, m0 + chunk);
      V sm = run.scratch(mma_gp_moments_scratch(g.d, run.nl, m1 - m0));
      double* out = pre[item].data() + (size_t)ch * 3 * nc;
      run([&](auto c) {
        mma_gp_item_moments(c, item, m0, m1, g.L, g.M, g.Mp, g.d, g.P, g.unc != 0, g.Z.data(), g.mu.data(), g.latmat.data(), g.w.data(),
                            g.q.data(), agg ? g.colL.data() : g.col.data(), agg ? g.empty.get() : g.row.data(), g.g_f1.data(),
                            g.g_Sff.data(), g.full, g.g_cross.data(), agg, out, sm.data());
      });
    }
  }
  return pre;
}

// every item of the match (what k_gp_bwd_items does, one workgroup per item); chunk > 0: the moments first (k_gp_bwd_moments)
static Outs gp_items(const Run& run, const GP& g, int chunk, bool agg) {
  const int d = g.d, nc = mma_gp_ncol(d), nchunk = chunk ? (g.M + chunk - 1) / chunk : 0;
  const double tol = mma_gp_nslice(d, run.nl) == 1 ? 0.0 : kGpTol;
  std::vector<V> pre;
  if (chunk) pre = gp_moments(Run{run.nl, run.nosync, 0}, g, chunk, agg);
  Outs o;
  (void)nc;
  for (int item = 0; item < g.L + g.P; ++item) {
    V gSi = nanv((size_t)d * d), gmi = nanv(d), cbuf = nanv(g.M), sm = run.scratch(mma_gp_item_scratch(d, run.nl));
    const double* pr = (chunk && gp_needs_moments(g, item, agg)) ? pre[item].data() : nullptr;
    run([&](auto c) {
      bool ok = true;
      mma_gp_item_bwd(c, item, g.L, g.M, g.Mp, d, g.P, g.unc != 0, g.Z.data(), g.ls2.data(), g.mu.data(), g.Sigma.data(), g.latmat.data(),
                      g.w.data(), g.q.data(), agg ? g.colL.data() : g.col.data(), agg ? g.empty.get() : g.row.data(), g.g_f1.data(),
                      g.g_Sff.data(), g.full, g.g_cross.data(), gSi.data(), gmi.data(), cbuf.data(), sm.data(), &ok,
                      agg ? g.pagg.data() : nullptr, g.f1raw.data(), pr, pr ? nchunk : 0);
      if (!ok) g_notok = 1;
    });
    o.push_back(rel(fmt("gS item %d", item).c_str(), gSi, tol));
    o.push_back(rel(fmt("gmu item %d", item).c_str(), gmi, tol));
  }
  return o;
}

static void cases_gp() {
  // 1 + d + d^2 below 256 (slices: 85 at d = 1, 19 at 3, 3 at 8) and above (16: 273, 17: 307); M below and above 4 slices and nl
  const int rm[][2] = {{1, 1}, {3, 3}, {300, 3}, {64, 8}, {300, 15}, {5, 16}};
  for (auto& s : rm) {
    const int M = s[0], d = s[1];
    check("mma_raw_moments", 256, fmt("M%d d%d", M, d), [=](const Run& run) {
      Rng r(1600 + M * 13 + d);
      const int nc = mma_gp_ncol(d), ns = mma_gp_nslice(d, run.nl);
      const V Z = r.vec((size_t)M * d), coef = r.vec(M);
      V part = run.scratch(ns * nc), out = nanv(nc);
      run([&](auto c) { mma_raw_moments(c, M, d, Z.data(), coef.data(), part.data(), out.data()); });
      return Outs{rel("moments", out, ns == 1 ? 0.0 : kGpTol)};
    });
  }
  // (L, M, Mp, d, full_cov, with_unc, chunk): one case per mode -- plain / chunked partials / aggregates / aggregates + chunked
  const int gp[][7] = {{1, 1, 1, 1, 0, 0, 1}, {3, 5, 8, 3, 1, 1, 2}, {2, 300, 320, 3, 1, 0, 128}, {2, 7, 7, 8, 0, 1, 4},
                       {2, 6, 8, 8, 1, 1, 4}, {2, 6, 8, 16, 1, 1, 4}, {2, 3, 3, 17, 1, 0, 2}, {1, 4, 4, 32, 0, 1, 2}};
  for (auto& s : gp) {
    const int L = s[0], M = s[1], Mp = s[2], d = s[3], full = s[4], unc = s[5], chunk = s[6];
    const std::string shape = fmt("L%d M%d Mp%d d%d full%d unc%d", L, M, Mp, d, full, unc);
    const uint64_t seed = 1700 + L * 1009 + M * 13 + d * 7 + full * 3 + unc;
    const bool has_agg = full && L > 1 && d <= 8;                          // aggregates: f32 packs, d <= 8, off-diagonal pairs present
    for (int agg = 0; agg <= (has_agg ? 1 : 0); ++agg) {
      check("mma_gp_item_moments", 256, shape + fmt(" chunk%d pagg%d", chunk, agg), [=](const Run& run) {
        Rng r(seed);
        const GP g = make_gp(r, L, M, Mp, d, full, unc);
        const std::vector<V> pre = gp_moments(run, g, chunk, agg != 0);
        const double tol = mma_gp_nslice(d, run.nl) == 1 ? 0.0 : kGpTol;
        Outs o;
        for (size_t i = 0; i < pre.size(); ++i) if (!pre[i].empty()) o.push_back(rel(fmt("pre item %d", (int)i).c_str(), pre[i], tol));
        return o;
      });
      for (int chunked = 0; chunked <= 1; ++chunked) {
        check("mma_gp_item_bwd", 256, shape + fmt(" chunk%d pagg%d", chunked ? chunk : 0, agg), [=](const Run& run) {
          Rng r(seed);
          const GP g = make_gp(r, L, M, Mp, d, full, unc);
          return gp_items(run, g, chunked ? chunk : 0, agg != 0);
        });
      }
    }
  }
}

// ---- the mixing of a coregionalised drift (k_compose_mix_nd, k_compose_mix_bwd_nd: 64 lanes) -------------------------------------------
template <typename T>
static void mix_fwd_case(const char* fn, int nx, int Lg, int nd, int with_c) {
  check(fn, 64, fmt("nx%d Lg%d nd%d c%d", nx, Lg, nd, with_c), [=](const Run& run) {
    Rng r(1800 + nx * 11 + Lg * 5 + nd);
    auto cast = [](const V& v) { std::vector<T> o(v.size()); for (size_t i = 0; i < v.size(); ++i) o[i] = (T)v[i]; return o; };
    auto back = [](const std::vector<T>& v) { V o(v.size()); for (size_t i = 0; i < v.size(); ++i) o[i] = (double)v[i]; return o; };
    const V W = r.vec((size_t)nx * Lg), mc = r.vec(nx);
    const std::vector<T> g1 = cast(r.vec(Lg)), Sgg = cast(r.spd(Lg)), cg = cast(r.vec((size_t)nd * Lg));
    std::vector<T> f1 = cast(nanv(nx)), Sff = cast(nanv((size_t)nx * nx)), cross = cast(nanv((size_t)nd * nx));
    V sm = run.scratch(mma_mix_scratch(nx, Lg));
    run([&](auto c) {
      mma_mix_fwd<decltype(c), T>(c, nx, Lg, nd, W.data(), with_c ? mc.data() : nullptr, g1.data(), Sgg.data(), cg.data(), f1.data(),
                                  Sff.data(), cross.data(), sm.data());
    });
    return Outs{bits("f1", back(f1)), bits("Sff", back(Sff)), bits("cross", back(cross))};
  });
}

static void cases_mix() {
  const int mx[][4] = {{1, 1, 2, 1}, {5, 2, 8, 1}, {5, 5, 8, 0}, {16, 3, 32, 1}, {16, 16, 21, 1}};   // (nx, Lg <= nx, nd, with a mean)
  for (auto& s : mx) {
    const int nx = s[0], Lg = s[1], nd = s[2];
    mix_fwd_case<double>("mma_mix_fwd<double>", nx, Lg, nd, s[3]);
    mix_fwd_case<float>("mma_mix_fwd<float>", nx, Lg, nd, s[3]);
    check("mma_mix_bwd", 64, fmt("nx%d Lg%d nd%d", nx, Lg, nd), [=](const Run& run) {
      Rng r(1900 + nx * 11 + Lg * 5 + nd);
      const V W = r.vec((size_t)nx * Lg), gf1 = r.vec(nx), gSff = r.vec((size_t)nx * nx), gcross = r.vec((size_t)nd * nx);
      V gg1 = nanv(Lg), gSgg = nanv((size_t)Lg * Lg), gcg = nanv((size_t)nd * Lg), sm = run.scratch(mma_mix_scratch(nx, Lg));
      run([&](auto c) {
        mma_mix_bwd(c, nx, Lg, nd, W.data(), gf1.data(), gSff.data(), gcross.data(), gg1.data(), gSgg.data(), gcg.data(), sm.data());
      });
      return Outs{bits("gg1", gg1), bits("gSgg", gSgg), bits("gcg", gcg)};
    });
  }
}

// ---- sequences on one arena, laid out as the kernel carves it and sized by its *_lds() helper less the trailing + 8 --------------------------
// k_compose_tail_bwd / _nd: cost -> encode -> step on one work area (64 lanes)
static void seq_tail(int nx, int na, int nu, bool nd_kernel) {
  check(nd_kernel ? "seq_tail_bwd_nd" : "seq_tail_bwd", 64, fmt("nx%d na%d nu%d", nx, na, nu), [=](const Run& run) {
    Rng r(2000 + nx * 9 + na * 5 + nu);
    const MMComposeDims D = make_dims(nx, na, nu);
    const int ne = D.ne, nd = D.nd;
    const size_t total = (nd_kernel ? mm_tail_bwd_nd_lds(nx, ne, nd) : mm_tail_bwd_lds(nx, ne, nd)) / sizeof(double) - 8;
    const size_t carry = (size_t)ne + ne * ne + nx * ne + nx + nx * nx;
    V arena = nanv(total - (size_t)run.shorten);                            // the work area, after ...
    for (size_t i = 0; i < carry; ++i) arena[i] = 2.0 * r.u() - 1.0;        // ... the carried adjoints the kernel loads first
    double* gme = arena.data(); double* gSee = gme + ne; double* gSxe = gSee + ne * ne; double* gm1 = gSxe + nx * ne;
    double* gS1 = gm1 + nx; double* wk = gS1 + nx * nx;
    const V x1m = r.vec(nx), x1S = r.spd(nx), me1 = r.vec(ne), See1 = r.spd(ne), target = r.vec(ne), precis = r.spd(ne),
            Sxe = r.vec((size_t)nx * ne), cp = r.vec((size_t)ne * nu), Sdd = r.vec((size_t)nd * nd), dcross = r.vec((size_t)nd * nx);
    V cSxe = nanv((size_t)nx * ne), ccp = nanv((size_t)ne * nu), cSdd = nanv((size_t)nd * nd), cdf1 = nanv(nx), cdSff = nanv((size_t)nx * nx),
      cdcross = nanv((size_t)nd * nx);
    run([&](auto c) {
      mma_cost_bwd(c, ne, me1.data(), See1.data(), target.data(), precis.data(), 0.7, gme, gSee, wk);
      mma_encode_bwd(c, D, x1m.data(), x1S.data(), gme, gSee, gSxe, gm1, gS1, wk);
      if (nd_kernel)
        mma_step_bwd_nd(c, D, 0.1, Sxe.data(), cp.data(), Sdd.data(), dcross.data(), gm1, gS1, cSxe.data(), ccp.data(), cSdd.data(),
                        cdf1.data(), cdSff.data(), cdcross.data(), wk);
      else
        mma_step_bwd(c, D, 0.1, Sxe.data(), cp.data(), Sdd.data(), dcross.data(), gm1, gS1, cSxe.data(), ccp.data(), cSdd.data(), cdf1.data(),
                     cdSff.data(), cdcross.data(), wk);
    });
    return Outs{bits("carry", slice(arena, 0, carry)), bits("cSxe", cSxe), bits("ccp", ccp), bits("cSdd", cSdd), bits("cdf1", cdf1),
                bits("cdSff", cdSff), bits("cdcross", cdcross)};
  });
}

// k_policy_head_bwd_small: head -> policy (256 lanes)
static void seq_policy_head(int M, int ne) {
  check("seq_policy_head_bwd", 256, fmt("M%d ne%d", M, ne), [=](const Run& run) {
    Rng r(2100 + M * 17 + ne);
    const int nd = ne + 1;
    const Policy p = make_policy(r, 1, M, ne);
    const size_t total = mm_policy_bwd_lds(M, ne) / sizeof(double) - 8;
    V arena = nanv(total - (size_t)run.shorten);
    double* gme = arena.data(); double* gSee = gme + ne; double* gpc = gSee + ne * ne; double* gmu = gpc + ne; double* gSig = gmu + ne;
    double* hw = gSig + ne * ne; double* dmd = hw + ne + 4; double* dSd = dmd + nd; double* wk = dSd + nd * nd;
    for (int k = 0; k < nd; ++k) dmd[k] = 2.0 * r.u() - 1.0;               // the kernel fills these two before its first barrier
    for (int k = 0; k < nd * nd; ++k) dSd[k] = 2.0 * r.u() - 1.0;
    const V pcross = r.vec(ne), ccp = r.vec(ne);
    const double tol = policy_one_slice(M, ne, run.nl) ? 0.0 : kPolTol;
    V gpar((size_t)M * ne + M + ne + 2, kParFill), cme = nanv(ne), cSee = nanv((size_t)ne * ne);
    run([&](auto c) {
      mma_head_bwd(c, ne, 2.0, -0.5, 0.3, 0.4, pcross.data(), p.Sigma.data(), dmd, dSd, ccp.data(), gme, gSee, gpc, hw);
      const double gpf1 = hw[ne], gpSff = hw[ne + 1];
      bool ok = true;
      mma_policy_small_bwd<decltype(c), 8>(c, M, ne, p.Z.data(), p.beta.data(), p.ls2.data(), p.var[0], p.mu.data(), p.Sigma.data(), gpf1,
                                           gpSff, gpc, gmu, gSig, gpar.data(), wk, &ok);
      for (int k = c.lane(); k < ne; k += c.nl()) cme[k] = gme[k] + gmu[k];
      for (int idx = c.lane(); idx < ne * ne; idx += c.nl()) cSee[idx] = gSee[idx] + gSig[idx];
      if (!ok) g_notok = 1;
    });
    Outs o{rel("cme", cme, tol), rel("cSee", cSee, tol)};
    par_groups(o, "gpar", gpar, 0, M, ne, p.ls2.data(), tol);
    return o;
  });
}

// k_policy_head_bwd_nd (and its _wide entries: `wide` sizes the arena with mm_policy_bwd_wide_lds): head -> policy (256 lanes)
static void seq_policy_head_nd(int M, int ne, int nu, bool wide) {
  check(wide ? "seq_policy_head_bwd_wide" : "seq_policy_head_bwd_nd", 256, fmt("M%d ne%d nu%d", M, ne, nu), [=](const Run& run) {
    Rng r(2200 + M * 17 + ne * 5 + nu);
    const int nd = ne + nu;
    const Policy p = make_policy(r, nu, M, ne);
    const size_t glen = (size_t)M * ne + M + ne + 2;
    const size_t total = (wide ? mm_policy_bwd_wide_lds(M, ne, nu) : mm_policy_bwd_nd_lds(M, ne, nu)) / sizeof(double) - 8;
    V arena = nanv(total - (size_t)run.shorten);
    double* gme = arena.data(); double* gSee = gme + ne; double* gpc = gSee + ne * ne; double* gmu = gpc + ne * nu; double* gSig = gmu + ne;
    double* gpf1 = gSig + ne * ne; double* gpS = gpf1 + nu; double* hsc = gpS + nu * nu;
    double* hw = hsc + 2 * nu;
    double* dmd = hw + mma_head_bwd_nd_scratch(ne, nu);
    double* dSd = dmd + nd;
    double* wk = dSd + nd * nd;
    for (int k = 0; k < nd; ++k) dmd[k] = 2.0 * r.u() - 1.0;               // the kernel fills these three before its first barrier
    for (int k = 0; k < nd * nd; ++k) dSd[k] = 2.0 * r.u() - 1.0;
    for (int k = 0; k < nu; ++k) { hsc[k] = 0.5 + 1.5 * r.u(); hsc[nu + k] = 2.0 * r.u() - 1.0; }
    const V pf1 = r.vec(nu), pSff = r.spd(nu), pcross = r.vec((size_t)ne * nu), ccp = r.vec((size_t)ne * nu);
    const double tol = policy_one_slice(M, ne, run.nl) ? 0.0 : kPolTol;
    V gpar((size_t)nu * glen, kParFill), cme = nanv(ne), cSee = nanv((size_t)ne * ne);
    run([&](auto c) {
      mma_head_bwd_nd(c, ne, nu, hsc, hsc + nu, pf1.data(), pSff.data(), pcross.data(), p.Sigma.data(), dmd, dSd, ccp.data(), gme, gSee,
                      gpc, gpf1, gpS, hw);
      bool ok = true;
      mma_policy_nd_bwd<decltype(c), 8>(c, nu, M, ne, p.Z.data(), p.beta.data(), p.ls2.data(), p.var.data(), p.mu.data(), p.Sigma.data(),
                                        gpf1, gpS, gpc, gmu, gSig, gpar.data(), wk, &ok);
      c.sync();
      for (int k = c.lane(); k < ne; k += c.nl()) cme[k] = gme[k] + gmu[k];
      for (int idx = c.lane(); idx < ne * ne; idx += c.nl()) cSee[idx] = gSee[idx] + gSig[idx];
      if (!ok) g_notok = 1;
    });
    Outs o{rel("cme", cme, tol), rel("cSee", cSee, tol)};
    for (int a = 0; a < nu; ++a) par_groups(o, fmt("gpar[%d]", a).c_str(), gpar, a * glen, M, ne, p.ls2.data() + (size_t)a * ne, tol);
    return o;
  });
}

// k_pair_agg: polynomial part -> (rows re-centred) -> + the remainder slabs -> columns re-centred, on the kernel's arena: the two
// weight-moment tables (KMp columns each: the degree <= 4 monomials rounded up to 16), G, the three shifts, T, the polynomial's scratch
static void seq_pair_agg(int nl, int d, int rcen) {
  check("seq_pair_agg", nl, fmt("d%d rcen%d", d, rcen), [=](const Run& run) {
    Rng r(2300 + d * 3 + rcen);
    const int nT = mma_pair_agg_len(d), KMp = (mm_mono_off(5, d) + 15) / 16 * 16;
    const size_t total = (size_t)2 * KMp + d * d + 3 * d + nT + mma_pair_poly_scratch(d);
    V arena = nanv(total - (size_t)run.shorten);
    double* nh = arena.data(); double* qh = nh + KMp; double* G = qh + KMp; double* dmu = G + d * d; double* dmu2 = dmu + d;
    double* dmuP = dmu2 + d; double* T = dmuP + d; double* scr = T + nT;
    for (int k = 0; k < 2 * KMp; ++k) nh[k] = 2.0 * r.u() - 1.0;             // the kernel fills these before its first barrier
    for (int k = 0; k < d * d; ++k) G[k] = 0.6 * r.u() - 0.3;
    for (int k = 0; k < d; ++k) { dmu[k] = 2.0 * r.u() - 1.0; dmu2[k] = 2.0 * r.u() - 1.0; dmuP[k] = rcen ? 0.0 : dmu[k]; }
    const V slab = r.vec(nT);
    V out = nanv(nT);
    run([&](auto c) {
      mma_pair_poly(c, d, G, dmuP, nh, qh, T, scr);
      if (rcen) { c.sync(); mma_pair_convert_rows(c, d, dmu, T); c.sync(); }
      for (int idx = c.lane(); idx < nT; idx += c.nl()) T[idx] += slab[idx];
      c.sync();
      mma_pair_convert(c, d, dmu2, T);
      c.sync();
      for (int idx = c.lane(); idx < nT; idx += c.nl()) out[idx] = T[idx];
    });
    return Outs{bits("pagg", out)};
  });
}

static void cases_sequences() {
  for (int nl : {256, 512}) for (int d : {3, 8}) for (int rcen : {0, 1}) seq_pair_agg(nl, d, rcen);
  seq_tail(1, 0, 1, false); seq_tail(5, 1, 1, false); seq_tail(16, 0, 1, false); seq_tail(16, 8, 1, false);
  seq_tail(5, 1, 2, true); seq_tail(16, 0, 1, true); seq_tail(16, 8, 4, true);
  seq_policy_head(3, 1); seq_policy_head(64, 5); seq_policy_head(1, 8); seq_policy_head(256, 8);
  seq_policy_head_nd(3, 5, 2, false); seq_policy_head_nd(64, 8, 4, false);
  seq_policy_head_nd(5, 16, 1, true); seq_policy_head_nd(3, 12, 2, true);
  // (the item kernels' sequence, moments -> item, passes through global memory: the chunked cases of mma_gp_item_bwd)
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const bool has = i + 1 < argc;
    if (!strcmp(argv[i], "--only") && has) g_only = argv[++i];
    else if (!strcmp(argv[i], "--no-sync") && has) g_nosync = argv[++i];
    else if (!strcmp(argv[i], "--short-scratch") && has) g_short = argv[++i];
    else { fprintf(stderr, "usage: %s [--only FN] [--no-sync FN] [--short-scratch FN]\n", argv[0]); return 2; }
  }
  cases_dense();
  cases_step();
  cases_head();
  cases_policy();
  cases_pair();
  cases_gp();
  cases_mix();
  cases_sequences();
  g_pools.clear();
  printf("cases: %d\nfailures: %d\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
