// The device overloads of mma_spd_inverse and mma_solve_pivot (csrc/mm_adjoint.h) on the GPU, one matrix per workgroup, for
// tests/test_gpu_dense_small.py.  Test infrastructure: a program of its own, nothing of the product library is linked.
//
//   dense_small in.bin out.bin
//
// in.bin (little endian):  int64 magic, int64 groups;  per group  int64 func (0 inverse, 1 solve), ctx (0 MMADevCtx, 1 MMAWideCtx<true>,
// 2 MMAWideCtx<false>), lanes (64 or 256), cases, blk;  then int64 dims[cases][3] = (n, nr, ld)  and  double block[cases][blk]: the
// LDS image of each case as the callers carve it -- inverse: A [n][ld] then Y [n][ld] (nr unused), solve: Aug [n][ld] -- with whatever
// the writer put into the padding and behind the end (the guard band).
// out.bin:  per group  double block[cases][blk] (the whole LDS image after the call),  double ret[cases][lanes] (the return value of
// every lane),  int32 ok[cases][lanes] (every lane's ok; 1 for the solve).
// One launch per group.  Every HIP call is checked: the first failure prints the error and exits 1, nothing is launched after it.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mm_adjoint.h"

#define CHECK(call)                                                                                        \
  do {                                                                                                     \
    const hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) {                                                                                \
      std::fprintf(stderr, "dense_small: %s: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      std::exit(1);                                                                                        \
    }                                                                                                      \
  } while (0)

static const int64_t kMagic = 0x444e53454431LL;
static const int kMaxN = 32, kMaxBlk = 4096;      // 32 KiB of LDS per workgroup at the most

template <class Ctx, int FUNC>
__global__ void k_case(const double* __restrict__ in, const long long* __restrict__ dims, int blk, double* __restrict__ out,
                       double* __restrict__ ret, int* __restrict__ okout) {
  extern __shared__ double sm[];
  const int cs = (int)blockIdx.x, t = (int)threadIdx.x, nl = (int)blockDim.x;
  const int n = (int)dims[3 * cs], nr = (int)dims[3 * cs + 1], ld = (int)dims[3 * cs + 2];
  for (int k = t; k < blk; k += nl) sm[k] = in[(size_t)cs * blk + k];
  __syncthreads();
  Ctx c{};
  bool ok = true;
  double r;
  if (FUNC == 0) r = mma_spd_inverse(c, sm, sm + n * ld, n, ld, &ok);
  else r = mma_solve_pivot(c, sm, n, nr, ld);
  __syncthreads();
  for (int k = t; k < blk; k += nl) out[(size_t)cs * blk + k] = sm[k];
  ret[(size_t)cs * nl + t] = r;
  okout[(size_t)cs * nl + t] = ok ? 1 : 0;
}

typedef void (*Kern)(const double*, const long long*, int, double*, double*, int*);
static Kern kernel(int func, int ctx) {
  if (func == 0) return ctx == 0 ? k_case<MMADevCtx, 0> : (ctx == 1 ? k_case<MMAWideCtx<true>, 0> : k_case<MMAWideCtx<false>, 0>);
  return ctx == 0 ? k_case<MMADevCtx, 1> : (ctx == 1 ? k_case<MMAWideCtx<true>, 1> : k_case<MMAWideCtx<false>, 1>);
}

static void fail(const char* what) { std::fprintf(stderr, "dense_small: %s\n", what); std::exit(2); }
static void rd(std::FILE* f, void* p, size_t bytes) { if (bytes && std::fread(p, 1, bytes, f) != bytes) fail("short read"); }
static void wr(std::FILE* f, const void* p, size_t bytes) { if (bytes && std::fwrite(p, 1, bytes, f) != bytes) fail("short write"); }

int main(int argc, char** argv) {
  if (argc != 3) fail("usage: dense_small in.bin out.bin");
  std::FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) fail("cannot open the input");
  int64_t head[2];
  rd(fi, head, sizeof head);
  if (head[0] != kMagic || head[1] < 0 || head[1] > 64) fail("not a case file");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) fail("cannot open the output");
  for (int64_t g = 0; g < head[1]; ++g) {
    int64_t gh[5];
    rd(fi, gh, sizeof gh);
    const int func = (int)gh[0], ctx = (int)gh[1], lanes = (int)gh[2], cases = (int)gh[3], blk = (int)gh[4];
    if (func < 0 || func > 1 || ctx < 0 || ctx > 2 || (lanes != 64 && lanes != 256) || cases < 1 || cases > 4096 || blk < 2 || blk > kMaxBlk)
      fail("bad group header");
    std::vector<long long> dims((size_t)cases * 3);
    std::vector<double> block((size_t)cases * blk), ret((size_t)cases * lanes);
    std::vector<int> ok((size_t)cases * lanes);
    rd(fi, dims.data(), dims.size() * sizeof(long long));
    rd(fi, block.data(), block.size() * sizeof(double));
    // every access of the code under test stays inside the block: checked here, before anything runs
    for (int cs = 0; cs < cases; ++cs) {
      const long long n = dims[3 * cs], nr = dims[3 * cs + 1], ld = dims[3 * cs + 2];
      if (n < 1 || n > kMaxN || ld < n + (func == 0 ? 1 : 0) || ld > 4 * kMaxN) fail("bad case dims");   // (Y[0..1] needs n ld >= 2)
      if (func == 0 ? (2 * n * ld > blk) : (nr < 1 || nr > kMaxN || n + nr > ld || n * ld > blk)) fail("case does not fit its block");
    }
    double *d_in, *d_out, *d_ret;
    long long* d_dims;
    int* d_ok;
    CHECK(hipMalloc(&d_in, block.size() * sizeof(double)));
    CHECK(hipMalloc(&d_out, block.size() * sizeof(double)));
    CHECK(hipMalloc(&d_ret, ret.size() * sizeof(double)));
    CHECK(hipMalloc(&d_dims, dims.size() * sizeof(long long)));
    CHECK(hipMalloc(&d_ok, ok.size() * sizeof(int)));
    CHECK(hipMemcpy(d_in, block.data(), block.size() * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_dims, dims.data(), dims.size() * sizeof(long long), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, block.size() * sizeof(double)));
    CHECK(hipMemset(d_ret, 0, ret.size() * sizeof(double)));
    CHECK(hipMemset(d_ok, 0xff, ok.size() * sizeof(int)));
    kernel(func, ctx)<<<dim3((unsigned)cases), dim3((unsigned)lanes), (size_t)blk * sizeof(double), 0>>>(d_in, d_dims, blk, d_out, d_ret, d_ok);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(block.data(), d_out, block.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ret.data(), d_ret, ret.size() * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(ok.data(), d_ok, ok.size() * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out)); CHECK(hipFree(d_ret)); CHECK(hipFree(d_dims)); CHECK(hipFree(d_ok));
    wr(fo, block.data(), block.size() * sizeof(double));
    wr(fo, ret.data(), ret.size() * sizeof(double));
    wr(fo, ok.data(), ok.size() * sizeof(int));
    std::printf("group %d: func %d ctx %d lanes %d cases %d blk %d ok\n", (int)g, func, ctx, lanes, cases, blk);
  }
  if (std::fgetc(fi) != EOF) fail("trailing bytes in the input");
  std::fclose(fi);
  if (std::fclose(fo) != 0) fail("cannot close the output");
  return 0;
}
