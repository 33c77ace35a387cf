// Fused gather-multiply-sum for MI355X (gfx950, CDNA4): the
// continuous-filter message of SchNet's CFConv and of both DimeNet++
// aggregations, and the edge-wise product that closes it under
// differentiation.
//
//   gms: out[i, f] = sum_{e in row i} x[gidx[e], f] * w[e, f]
//   gm : out[e, f] = a[ia[e], f] * b[ib[e], f]
//
// gms maps one thread to one (row, feature pack), gm one thread to one
// (edge, feature pack); both grid-stride.  Consecutive lanes hold
// consecutive packs, so every step of a row walk reads contiguous
// pieces of one row of x and one row of w.  No atomics, no zero fill,
// no LDS: every output element has exactly one writer.
//
// Rows are positions rowptr[i] .. rowptr[i+1] of the edge list, or of
// perm (a stable argsort of an unsorted index) when one is given.  The
// sum runs in ascending position from 0 in the accumulator type (fp32
// for bf16/f16).  Each product is rounded to the accumulator type and
// then added (__fmul_rn / __dmul_rn: never contracted into an fma), so
// for fp32/fp64 the result equals, bit for bit, the composition
// segment_sum_csr(gather(x) * w); for the half types the product is
// exact in fp32.  The result is rounded once.
//
// A pack is 16 bytes (VEC = 16 / sizeof(T)) when the row size in bytes
// is a multiple of 16 and every base pointer is 16-byte aligned, and
// one element otherwise.  A null index means the identity (e itself).
//
// A row is walked by one thread: the run time follows the longest row.

#include <torch/extension.h>
#include <ATen/OpMathType.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "check_launch.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGridCap = 8192;
constexpr int kUnroll = 4;      // positions of a row loaded ahead of the adds

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

// __fmul_rn / __dmul_rn are a plain product in the HIP headers, which
// the compiler's default (contract = fast) still fuses with the add
// that follows; this turns contraction off for the rest of the file.
#pragma clang fp contract(off)

__device__ inline float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ inline double mul_rn(double a, double b) { return __dmul_rn(a, b); }

template <typename T, typename ACC, int VEC>
__global__ void gms_kernel(const T* __restrict__ x, const T* __restrict__ w,
                           const long* __restrict__ rowptr,
                           const long* __restrict__ perm,
                           const long* __restrict__ gidx,
                           T* __restrict__ out, long N, long Fp) {
  using P = Pack<T, VEC>;
  const P* __restrict__ xp = reinterpret_cast<const P*>(x);
  const P* __restrict__ wp = reinterpret_cast<const P*>(w);
  P* __restrict__ op = reinterpret_cast<P*>(out);
  const long total = N * Fp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / Fp;
    const long f = i - r * Fp;
    const long lo = rowptr[r], hi = rowptr[r + 1];
    ACC acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = (ACC)0;
    long p = lo;
    // kUnroll positions at a time: the dependent loads perm -> gidx ->
    // x of several positions are in flight together; the adds keep
    // their order
    for (; p + kUnroll <= hi; p += kUnroll) {
      P xv[kUnroll], wv[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const long e = perm ? perm[p + u] : p + u;
        const long c = gidx ? gidx[e] : e;
        xv[u] = xp[c * Fp + f];
        wv[u] = wp[e * Fp + f];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          acc[k] += mul_rn((ACC)xv[u].v[k], (ACC)wv[u].v[k]);
    }
    for (; p < hi; ++p) {
      const long e = perm ? perm[p] : p;
      const long c = gidx ? gidx[e] : e;
      const P xv = xp[c * Fp + f];
      const P wv = wp[e * Fp + f];
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        acc[k] += mul_rn((ACC)xv.v[k], (ACC)wv.v[k]);
    }
    P o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = (T)acc[k];
    op[i] = o;
  }
}

template <typename T, int VEC>
__global__ void gm_kernel(const T* __restrict__ a, const T* __restrict__ b,
                          const long* __restrict__ ia,
                          const long* __restrict__ ib, T* __restrict__ out,
                          long E, long Fp) {
  using P = Pack<T, VEC>;
  using ACC = at::opmath_type<T>;
  const P* __restrict__ ap = reinterpret_cast<const P*>(a);
  const P* __restrict__ bp = reinterpret_cast<const P*>(b);
  P* __restrict__ op = reinterpret_cast<P*>(out);
  const long total = E * Fp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long e = i / Fp;
    const long f = i - e * Fp;
    const long ca = ia ? ia[e] : e;
    const long cb = ib ? ib[e] : e;
    const P av = ap[ca * Fp + f];
    const P bv = bp[cb * Fp + f];
    P o;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      o.v[k] = (T)mul_rn((ACC)av.v[k], (ACC)bv.v[k]);
    op[i] = o;
  }
}

inline int n_blocks(long total) {
  long b = (total + kBlock - 1) / kBlock;
  return (int)std::min<long>(b, kGridCap);
}

inline bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

void check_rows(const torch::Tensor& t, const torch::Tensor& like,
                const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2, what,
              " must be a contiguous [rows, F] GPU tensor");
  TORCH_CHECK(t.scalar_type() == like.scalar_type() &&
                  t.size(1) == like.size(1),
              what, ": both operands must have the same dtype and F");
}

// a null pointer for an absent (identity) index
const long* index_ptr(const c10::optional<torch::Tensor>& idx, long n,
                      torch::Tensor& keep, const char* what) {
  if (!idx.has_value()) return nullptr;
  TORCH_CHECK(idx->is_cuda() && idx->dtype() == torch::kLong &&
                  idx->dim() == 1 && idx->numel() == n,
              what, " must be int64 [E] on the device");
  keep = idx->contiguous();
  return keep.data_ptr<long>();
}

}  // namespace

// out[N, F] = sum over the rows of (rowptr, perm) of x[gidx[e]] * w[e];
// gidx absent: x[e]; rowptr[N] must equal E = w.size(0)
torch::Tensor gather_mul_sum(torch::Tensor x, torch::Tensor w,
                             c10::optional<torch::Tensor> gidx,
                             torch::Tensor rowptr,
                             c10::optional<torch::Tensor> perm) {
  check_rows(x, x, "x");
  check_rows(w, x, "w");
  TORCH_CHECK(rowptr.is_cuda() && rowptr.dtype() == torch::kLong &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "rowptr must be int64 [N + 1] on the device");
  const long E = w.size(0), N = rowptr.numel() - 1, F = x.size(1);
  TORCH_CHECK(E < (1L << 31), "gather_mul_sum: E must be below 2^31");
  TORCH_CHECK(gidx.has_value() || x.size(0) == E,
              "without a gather index x needs one row per edge");
  torch::Tensor gk, pk;
  const long* gp = index_ptr(gidx, E, gk, "the gather index");
  const long* pp = index_ptr(perm, E, pk, "perm");
  if (N * F == 0 || E == 0) return torch::zeros({N, F}, x.options());
  auto out = torch::empty({N, F}, x.options());
  auto rp = rowptr.contiguous();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(),
      "gather_mul_sum", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        constexpr int kVec = 16 / sizeof(scalar_t);
        const scalar_t* xp = x.data_ptr<scalar_t>();
        const scalar_t* wp = w.data_ptr<scalar_t>();
        scalar_t* op = out.data_ptr<scalar_t>();
        if (F % kVec == 0 && aligned16(xp) && aligned16(wp) &&
            aligned16(op)) {
          const long Fp = F / kVec;
          hipLaunchKernelGGL((gms_kernel<scalar_t, acc_t, kVec>),
                             dim3(n_blocks(N * Fp)), dim3(kBlock), 0,
                             at::hip::getCurrentHIPStream().stream(), xp, wp,
                             rp.data_ptr<long>(), pp, gp, op, N, Fp);
        } else {
          hipLaunchKernelGGL((gms_kernel<scalar_t, acc_t, 1>),
                             dim3(n_blocks(N * F)), dim3(kBlock), 0,
                             at::hip::getCurrentHIPStream().stream(), xp, wp,
                             rp.data_ptr<long>(), pp, gp, op, N, F);
        }
        check_launch("gms_kernel");
      });
  return out;
}

// out[E, F] = a[ia[e]] * b[ib[e]]; an absent index is the identity
torch::Tensor gather_mul(torch::Tensor a, torch::Tensor b,
                         c10::optional<torch::Tensor> ia,
                         c10::optional<torch::Tensor> ib, long E) {
  check_rows(a, a, "a");
  check_rows(b, a, "b");
  TORCH_CHECK(E >= 0 && E < (1L << 31), "gather_mul: E must be below 2^31");
  TORCH_CHECK(ia.has_value() || a.size(0) == E,
              "without an index a needs one row per edge");
  TORCH_CHECK(ib.has_value() || b.size(0) == E,
              "without an index b needs one row per edge");
  const long F = a.size(1);
  torch::Tensor ak, bk;
  const long* iap = index_ptr(ia, E, ak, "the index of a");
  const long* ibp = index_ptr(ib, E, bk, "the index of b");
  auto out = torch::empty({E, F}, a.options());
  if (E * F == 0) return out;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, a.scalar_type(),
      "gather_mul", [&] {
        constexpr int kVec = 16 / sizeof(scalar_t);
        const scalar_t* ap = a.data_ptr<scalar_t>();
        const scalar_t* bp = b.data_ptr<scalar_t>();
        scalar_t* op = out.data_ptr<scalar_t>();
        if (F % kVec == 0 && aligned16(ap) && aligned16(bp) &&
            aligned16(op)) {
          const long Fp = F / kVec;
          hipLaunchKernelGGL((gm_kernel<scalar_t, kVec>),
                             dim3(n_blocks(E * Fp)), dim3(kBlock), 0,
                             at::hip::getCurrentHIPStream().stream(), ap, bp,
                             iap, ibp, op, E, Fp);
        } else {
          hipLaunchKernelGGL((gm_kernel<scalar_t, 1>),
                             dim3(n_blocks(E * F)), dim3(kBlock), 0,
                             at::hip::getCurrentHIPStream().stream(), ap, bp,
                             iap, ibp, op, E, F);
        }
        check_launch("gm_kernel");
      });
  return out;
}
