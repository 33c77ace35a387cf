// hydragnn_amd HIP kernels for MI355X (gfx950, CDNA4).
//
// Segment reductions (gather / scatter) are THE hot aggregation of every
// message-passing stack. Design notes:
//  - wave = 64 lanes; block sizes are multiples of 64.
//  - memory-bound ops: grid-stride loops, coalesced along the feature
//    dim, vectorized where dtype/shape allow.
//  - bf16/f16 sums accumulate in fp32 on every route (atomicAdd on
//    packed halves is both slow and lossy), cast once at the end; a
//    mean is divided in the accumulator type before that one cast.
//  - a launch of zero elements is skipped; every launch is checked.
//  - grid capped at ~2048 blocks with grid-stride (guide G11).
//
// Reference behavior being reimplemented (not copied):
//   torch_scatter.scatter / index_add_ call sites listed in SURVEY.md §2c.

#include <torch/extension.h>
#include <ATen/OpMathType.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define CHECK_CUDA(x) TORCH_CHECK(x.is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

namespace {

constexpr int kBlock = 256;

inline int n_blocks(long total, int block, int cap = 2048) {
  long b = (total + block - 1) / block;
  return (int)std::min<long>(b, cap);
}

// elements of one row: the product of the trailing dims (defined for a
// tensor of zero rows too)
inline long row_elems(const torch::Tensor& t) {
  long f = 1;
  for (int64_t d = 1; d < t.dim(); ++d) f *= t.size(d);
  return f;
}

inline bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

// -------------------------------------------------------------------------
// gather: out[e, f] = src[index[e], f]
// -------------------------------------------------------------------------
template <typename T>
__global__ void gather_kernel(const T* __restrict__ src,
                              const long* __restrict__ index,
                              T* __restrict__ out, long E, long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    out[i] = src[index[e] * F + f];
  }
}

// float4-vectorized variant for rows that are a multiple of 16 bytes
// on 16-byte-aligned bases (16B/lane coalescing).
template <typename V>
__global__ void gather_kernel_vec(const V* __restrict__ src,
                                  const long* __restrict__ index,
                                  V* __restrict__ out, long E, long Fv) {
  long total = E * Fv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / Fv;
    long f = i - e * Fv;
    out[i] = src[index[e] * Fv + f];
  }
}

// -------------------------------------------------------------------------
// scatter-add (atomic path; CSR segment path below is used when rowptr
// is available).  fp32/fp64 only — half types go through an fp32 buffer.
// -------------------------------------------------------------------------
template <typename T>
__global__ void scatter_add_kernel(const T* __restrict__ src,
                                   const long* __restrict__ index,
                                   T* __restrict__ out, long E, long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    atomicAdd(&out[index[e] * F + f], src[i]);
  }
}

__global__ void scatter_add_bf16_kernel(const __hip_bfloat16* __restrict__ src,
                                        const long* __restrict__ index,
                                        float* __restrict__ out, long E,
                                        long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    atomicAdd(&out[index[e] * F + f], __bfloat162float(src[i]));
  }
}

__global__ void scatter_add_f16_kernel(const __half* __restrict__ src,
                                       const long* __restrict__ index,
                                       float* __restrict__ out, long E,
                                       long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    atomicAdd(&out[index[e] * F + f], __half2float(src[i]));
  }
}

// CSR segment sum over dst-sorted edges: deterministic and
// contention-free (vs the atomic path).  Thread per (row, feature);
// consecutive edges of a row are contiguous src rows -> coalesced
// within each step of the edge loop.  ACC is fp32 for bf16/f16.  MEAN
// divides the accumulator by the row length before the one store.
template <typename T, typename ACC, bool MEAN>
__global__ void segment_sum_csr_kernel(const T* __restrict__ src,
                                       const long* __restrict__ rowptr,
                                       T* __restrict__ out, long N,
                                       long F) {
  long total = N * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long n = i / F;
    long f = i - n * F;
    ACC acc = (ACC)0;
    long lo = rowptr[n], hi = rowptr[n + 1];
    for (long e = lo; e < hi; ++e) acc += (ACC)src[e * F + f];
    if (MEAN && hi > lo) acc = acc / (ACC)(hi - lo);
    out[i] = (T)acc;
  }
}

// Indexed CSR segment sum: out[r] = sum_{e in row r} src[perm[e]].
// Used as gather's backward when the caller precomputed an index-sort
// (scatter-by-unsorted-index without atomics: deterministic, no L2
// contention on hot rows).
template <typename T, typename ACC>
__global__ void segment_sum_csr_idx_kernel(
    const T* __restrict__ src, const long* __restrict__ rowptr,
    const long* __restrict__ perm, T* __restrict__ out, long N,
    long F) {
  long total = N * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long n = i / F;
    long f = i - n * F;
    ACC acc = (ACC)0;
    long lo = rowptr[n], hi = rowptr[n + 1];
    for (long e = lo; e < hi; ++e) acc += (ACC)src[perm[e] * F + f];
    out[i] = (T)acc;
  }
}

__global__ void count_kernel(const long* __restrict__ index,
                             float* __restrict__ count, long E) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < E;
       i += (long)gridDim.x * blockDim.x) {
    atomicAdd(&count[index[i]], 1.0f);
  }
}

// in place on the accumulator (fp32 or fp64), before any cast
template <typename T>
__global__ void divide_rows_kernel(T* __restrict__ out,
                                   const float* __restrict__ count, long N,
                                   long F) {
  long total = N * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long n = i / F;
    float c = count[n];
    if (c > 0.5f) out[i] = out[i] / (T)c;
  }
}

// -------------------------------------------------------------------------
// scatter min/max with argext — two-pass:
//   pass 1: atomic extreme on float-ordered bits
//   pass 2: first (lowest e) matching edge wins the arg slot (atomicMin)
//   finalize: a slot no edge claimed (arg still kNoArg) is an empty
//   segment -> 0 / -1; the value cannot tell, a segment of all -inf
//   under max leaves the bits at their fill
// -------------------------------------------------------------------------
constexpr unsigned long long kNoArg = 0x7fffffffffffffffull;

__device__ inline unsigned int float_flip(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving
}
__device__ inline float float_unflip(unsigned int u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__global__ void scatter_max_pass1(const float* __restrict__ src,
                                  const long* __restrict__ index,
                                  unsigned int* __restrict__ out_bits, long E,
                                  long F, bool is_max) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    unsigned int bits = float_flip(src[i]);
    unsigned int* slot = &out_bits[index[e] * F + f];
    if (is_max)
      atomicMax(slot, bits);
    else
      atomicMin(slot, bits);
  }
}

__global__ void scatter_max_pass2(const float* __restrict__ src,
                                  const long* __restrict__ index,
                                  const unsigned int* __restrict__ out_bits,
                                  unsigned long long* __restrict__ arg, long E,
                                  long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    long slot = index[e] * F + f;
    if (float_flip(src[i]) == out_bits[slot]) {
      atomicMin(&arg[slot], (unsigned long long)e);
    }
  }
}

// ---- fp64 variants (order-preserving flip on 64-bit patterns) ----
__device__ inline unsigned long long double_flip(double f) {
  unsigned long long u = __double_as_longlong(f);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double double_unflip(unsigned long long u) {
  return __longlong_as_double(
      (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u);
}

__global__ void scatter_max_pass1_f64(const double* __restrict__ src,
                                      const long* __restrict__ index,
                                      unsigned long long* __restrict__ out_bits,
                                      long E, long F, bool is_max) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    unsigned long long bits = double_flip(src[i]);
    unsigned long long* slot = &out_bits[index[e] * F + f];
    if (is_max)
      atomicMax(slot, bits);
    else
      atomicMin(slot, bits);
  }
}

__global__ void scatter_max_pass2_f64(const double* __restrict__ src,
                                      const long* __restrict__ index,
                                      const unsigned long long* __restrict__ out_bits,
                                      unsigned long long* __restrict__ arg,
                                      long E, long F) {
  long total = E * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    long e = i / F;
    long f = i - e * F;
    long slot = index[e] * F + f;
    if (double_flip(src[i]) == out_bits[slot]) {
      atomicMin(&arg[slot], (unsigned long long)e);
    }
  }
}

__global__ void scatter_max_finalize_f64(
    const unsigned long long* __restrict__ bits,
    const unsigned long long* __restrict__ arg, double* __restrict__ out,
    long* __restrict__ arg_out, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    bool present = arg[i] != kNoArg;
    out[i] = present ? double_unflip(bits[i]) : 0.0;
    arg_out[i] = present ? (long)arg[i] : -1;
  }
}

__global__ void scatter_max_finalize(const unsigned int* __restrict__ bits,
                                     const unsigned long long* __restrict__ arg,
                                     float* __restrict__ out,
                                     long* __restrict__ arg_out, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    bool present = arg[i] != kNoArg;
    out[i] = present ? float_unflip(bits[i]) : 0.0f;
    arg_out[i] = present ? (long)arg[i] : -1;
  }
}

// -------------------------------------------------------------------------
// radius graph (brute force within graph, count+fill; capping by
// distance order is finished in Python with device torch ops)
// -------------------------------------------------------------------------
__global__ void radius_count_kernel(const float* __restrict__ pos,
                                    const long* __restrict__ graph_of,
                                    const long* __restrict__ gptr, long N,
                                    float r2, bool loop,
                                    int* __restrict__ count) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N;
       i += (long)gridDim.x * blockDim.x) {
    long g = graph_of[i];
    long lo = gptr[g], hi = gptr[g + 1];
    float xi = pos[i * 3], yi = pos[i * 3 + 1], zi = pos[i * 3 + 2];
    int c = 0;
    for (long j = lo; j < hi; ++j) {
      if (!loop && j == i) continue;
      float dx = pos[j * 3] - xi, dy = pos[j * 3 + 1] - yi,
            dz = pos[j * 3 + 2] - zi;
      if (dx * dx + dy * dy + dz * dz <= r2) ++c;
    }
    count[i] = c;
  }
}

__global__ void radius_fill_kernel(const float* __restrict__ pos,
                                   const long* __restrict__ graph_of,
                                   const long* __restrict__ gptr,
                                   const long* __restrict__ offs, long N,
                                   float r2, bool loop,
                                   long* __restrict__ src_out,
                                   long* __restrict__ dst_out,
                                   float* __restrict__ dist_out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N;
       i += (long)gridDim.x * blockDim.x) {
    long g = graph_of[i];
    long lo = gptr[g], hi = gptr[g + 1];
    float xi = pos[i * 3], yi = pos[i * 3 + 1], zi = pos[i * 3 + 2];
    long w = offs[i];
    for (long j = lo; j < hi; ++j) {
      if (!loop && j == i) continue;
      float dx = pos[j * 3] - xi, dy = pos[j * 3 + 1] - yi,
            dz = pos[j * 3 + 2] - zi;
      float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 <= r2) {
        src_out[w] = j;   // src = neighbor
        dst_out[w] = i;   // dst = center
        dist_out[w] = sqrtf(d2);
        ++w;
      }
    }
  }
}

}  // namespace

// ===========================================================================
// C++ entry points
// ===========================================================================

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

#define LAUNCH(kernel, total, cap, ...)                                   \
  do {                                                                    \
    hipLaunchKernelGGL(kernel, dim3(n_blocks((total), kBlock, (cap))),    \
                       dim3(kBlock), 0, cur_stream(), __VA_ARGS__);       \
    C10_HIP_KERNEL_LAUNCH_CHECK();                                        \
  } while (0)

torch::Tensor gather_fwd(torch::Tensor src, torch::Tensor index) {
  CHECK_CUDA(src); CHECK_CONTIG(src); CHECK_CUDA(index);
  TORCH_CHECK(index.dtype() == torch::kLong);
  TORCH_CHECK(src.dim() >= 1, "src needs a row dim");
  long E = index.numel();
  long F = row_elems(src);
  auto sizes = src.sizes().vec();
  sizes[0] = E;
  auto out = torch::empty(sizes, src.options());
  if (E * F == 0) return out;
  auto idx = index.contiguous();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, src.scalar_type(),
      "gather_fwd", [&] {
        long bytes = F * sizeof(scalar_t);
        const scalar_t* sp = src.data_ptr<scalar_t>();
        scalar_t* op = out.data_ptr<scalar_t>();
        // a contiguous view into a flat buffer need not start on 16 B
        if (bytes % 16 == 0 && aligned16(sp) && aligned16(op)) {
          long Fv = bytes / 16;
          LAUNCH(gather_kernel_vec<float4>, E * Fv, 2048,
                 reinterpret_cast<const float4*>(sp), idx.data_ptr<long>(),
                 reinterpret_cast<float4*>(op), E, Fv);
        } else {
          LAUNCH(gather_kernel<scalar_t>, E * F, 2048, sp,
                 idx.data_ptr<long>(), op, E, F);
        }
      });
  return out;
}

// Atomic segment sum into a zeroed accumulator: fp32 for bf16/f16
// sources, the source dtype otherwise.
static torch::Tensor scatter_sum_acc(const torch::Tensor& src,
                                     const torch::Tensor& index,
                                     long dim_size) {
  CHECK_CUDA(src); CHECK_CONTIG(src); CHECK_CUDA(index);
  TORCH_CHECK(index.dtype() == torch::kLong);
  TORCH_CHECK(src.dim() >= 1 && index.numel() == src.size(0),
              "index must hold one entry per src row");
  long E = index.numel();
  long F = row_elems(src);
  auto sizes = src.sizes().vec();
  sizes[0] = dim_size;
  auto st = src.scalar_type();
  bool half = st == at::ScalarType::BFloat16 || st == at::ScalarType::Half;
  auto acc = torch::zeros(
      sizes, half ? src.options().dtype(torch::kFloat) : src.options());
  if (E * F == 0 || dim_size == 0) return acc;
  auto idx = index.contiguous();
  if (st == at::ScalarType::BFloat16) {
    LAUNCH(scatter_add_bf16_kernel, E * F, 2048,
           reinterpret_cast<const __hip_bfloat16*>(src.data_ptr()),
           idx.data_ptr<long>(), acc.data_ptr<float>(), E, F);
  } else if (st == at::ScalarType::Half) {
    LAUNCH(scatter_add_f16_kernel, E * F, 2048,
           reinterpret_cast<const __half*>(src.data_ptr()),
           idx.data_ptr<long>(), acc.data_ptr<float>(), E, F);
  } else {
    AT_DISPATCH_FLOATING_TYPES(st, "scatter_sum_fwd", [&] {
      LAUNCH(scatter_add_kernel<scalar_t>, E * F, 2048,
             src.data_ptr<scalar_t>(), idx.data_ptr<long>(),
             acc.data_ptr<scalar_t>(), E, F);
    });
  }
  return acc;
}

torch::Tensor scatter_sum_fwd(torch::Tensor src, torch::Tensor index,
                              long dim_size) {
  return scatter_sum_acc(src, index, dim_size).to(src.scalar_type());
}

// mean = true (sorted route only): each row's sum is divided by its
// length in the accumulator type before the store.
torch::Tensor segment_sum_csr(torch::Tensor src, torch::Tensor rowptr,
                              c10::optional<torch::Tensor> perm,
                              bool mean) {
  CHECK_CUDA(src); CHECK_CONTIG(src); CHECK_CUDA(rowptr);
  TORCH_CHECK(rowptr.dtype() == torch::kLong && rowptr.numel() >= 1,
              "rowptr must be int64 [N + 1]");
  TORCH_CHECK(src.dim() >= 1, "src needs a row dim");
  TORCH_CHECK(!(mean && perm.has_value()),
              "the mean variant takes sorted rows, not a perm");
  long N = rowptr.numel() - 1;
  long F = row_elems(src);
  auto sizes = src.sizes().vec();
  sizes[0] = N;
  // nothing to sum: every row is empty
  if (N * F == 0 || src.size(0) == 0) return torch::zeros(sizes, src.options());
  auto out = torch::empty(sizes, src.options());
  auto rp = rowptr.contiguous();
  torch::Tensor pc;
  const long* perm_ptr = nullptr;
  if (perm.has_value()) {
    CHECK_CUDA((*perm));
    TORCH_CHECK(perm->dtype() == torch::kLong);
    pc = perm->contiguous();
    perm_ptr = pc.data_ptr<long>();
  }
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, src.scalar_type(),
      "segment_sum_csr", [&] {
        using acc_t = at::opmath_type<scalar_t>;  // fp32 for bf16/f16
        const scalar_t* sp = src.data_ptr<scalar_t>();
        scalar_t* op = out.data_ptr<scalar_t>();
        if (perm_ptr) {
          LAUNCH((segment_sum_csr_idx_kernel<scalar_t, acc_t>), N * F, 8192,
                 sp, rp.data_ptr<long>(), perm_ptr, op, N, F);
        } else if (mean) {
          LAUNCH((segment_sum_csr_kernel<scalar_t, acc_t, true>), N * F,
                 8192, sp, rp.data_ptr<long>(), op, N, F);
        } else {
          LAUNCH((segment_sum_csr_kernel<scalar_t, acc_t, false>), N * F,
                 8192, sp, rp.data_ptr<long>(), op, N, F);
        }
      });
  return out;
}

std::vector<torch::Tensor> scatter_mean_fwd(torch::Tensor src,
                                            torch::Tensor index,
                                            long dim_size) {
  auto acc = scatter_sum_acc(src, index, dim_size);
  long E = index.numel();
  long F = row_elems(src);
  auto count = torch::zeros({dim_size}, src.options().dtype(torch::kFloat));
  if (E > 0 && dim_size > 0) {
    auto idx = index.contiguous();
    LAUNCH(count_kernel, E, 2048, idx.data_ptr<long>(),
           count.data_ptr<float>(), E);
    if (F > 0) {
      // divide the accumulator; a half type is rounded once, after
      AT_DISPATCH_FLOATING_TYPES(acc.scalar_type(), "divide_rows", [&] {
        LAUNCH(divide_rows_kernel<scalar_t>, dim_size * F, 2048,
               acc.data_ptr<scalar_t>(), count.data_ptr<float>(), dim_size,
               F);
      });
    }
  }
  return {acc.to(src.scalar_type()), count};
}

std::vector<torch::Tensor> scatter_minmax_fwd_f64(torch::Tensor src,
                                                  torch::Tensor index,
                                                  long dim_size,
                                                  bool is_max) {
  auto srcd = src.contiguous();
  long E = index.numel();
  long F = row_elems(srcd);
  auto sizes = src.sizes().vec();
  sizes[0] = dim_size;
  long total = dim_size * F;
  auto idx = index.contiguous();
  auto bits = torch::empty(sizes, src.options().dtype(torch::kLong));
  {
    double fill = is_max ? -INFINITY : INFINITY;
    unsigned long long raw;
    memcpy(&raw, &fill, 8);
    unsigned long long u = (raw & 0x8000000000000000ull) ? ~raw
                           : (raw | 0x8000000000000000ull);
    bits.fill_((long)u);
  }
  auto arg64 = torch::full(sizes, (long)kNoArg,
                           src.options().dtype(torch::kLong));
  auto out = torch::empty(sizes, src.options());
  auto arg = torch::empty(sizes, src.options().dtype(torch::kLong));
  auto bits_p = reinterpret_cast<unsigned long long*>(bits.data_ptr<long>());
  auto arg_p = reinterpret_cast<unsigned long long*>(arg64.data_ptr<long>());
  if (E * F > 0 && dim_size > 0) {
    LAUNCH(scatter_max_pass1_f64, E * F, 2048, srcd.data_ptr<double>(),
           idx.data_ptr<long>(), bits_p, E, F, is_max);
    LAUNCH(scatter_max_pass2_f64, E * F, 2048, srcd.data_ptr<double>(),
           idx.data_ptr<long>(), bits_p, arg_p, E, F);
  }
  if (total > 0) {
    LAUNCH(scatter_max_finalize_f64, total, 2048, bits_p, arg_p,
           out.data_ptr<double>(), arg.data_ptr<long>(), total);
  }
  return {out, arg};
}

std::vector<torch::Tensor> scatter_minmax_fwd(torch::Tensor src,
                                              torch::Tensor index,
                                              long dim_size, bool is_max) {
  CHECK_CUDA(src); CHECK_CUDA(index);
  TORCH_CHECK(index.dtype() == torch::kLong);
  TORCH_CHECK(src.dim() >= 1 && index.numel() == src.size(0),
              "index must hold one entry per src row");
  if (src.scalar_type() == at::ScalarType::Double) {
    return scatter_minmax_fwd_f64(src, index, dim_size, is_max);
  }
  auto srcf = src.contiguous().to(torch::kFloat);
  long E = index.numel();
  long F = row_elems(srcf);
  auto sizes = src.sizes().vec();
  sizes[0] = dim_size;
  long total = dim_size * F;
  auto idx = index.contiguous();
  auto bits = torch::empty(sizes, src.options().dtype(torch::kInt));
  {
    float fill = is_max ? -INFINITY : INFINITY;
    unsigned int u;
    // host-side flip of the fill value
    unsigned int raw;
    memcpy(&raw, &fill, 4);
    u = (raw & 0x80000000u) ? ~raw : (raw | 0x80000000u);
    bits.fill_((int)u);
  }
  auto arg64 = torch::full(sizes, (long)kNoArg,
                           src.options().dtype(torch::kLong));
  auto out = torch::empty(sizes, src.options().dtype(torch::kFloat));
  auto arg = torch::empty(sizes, src.options().dtype(torch::kLong));
  auto bits_p = reinterpret_cast<unsigned int*>(bits.data_ptr<int>());
  auto arg_p = reinterpret_cast<unsigned long long*>(arg64.data_ptr<long>());
  if (E * F > 0 && dim_size > 0) {
    LAUNCH(scatter_max_pass1, E * F, 2048, srcf.data_ptr<float>(),
           idx.data_ptr<long>(), bits_p, E, F, is_max);
    LAUNCH(scatter_max_pass2, E * F, 2048, srcf.data_ptr<float>(),
           idx.data_ptr<long>(), bits_p, arg_p, E, F);
  }
  if (total > 0) {
    LAUNCH(scatter_max_finalize, total, 2048, bits_p, arg_p,
           out.data_ptr<float>(), arg.data_ptr<long>(), total);
  }
  return {out.to(src.scalar_type()), arg};
}

std::vector<torch::Tensor> radius_pairs(torch::Tensor pos, torch::Tensor batch,
                                        torch::Tensor gptr, double r,
                                        bool loop) {
  CHECK_CUDA(pos); CHECK_CONTIG(pos);
  long N = pos.size(0);
  float r2 = (float)(r * r);
  auto count = torch::zeros({N}, pos.options().dtype(torch::kInt));
  auto b = batch.contiguous();
  auto gp = gptr.contiguous();
  if (N > 0) {
    LAUNCH(radius_count_kernel, N, 2048, pos.data_ptr<float>(),
           b.data_ptr<long>(), gp.data_ptr<long>(), N, r2, loop,
           count.data_ptr<int>());
  }
  auto offs = torch::zeros({N}, pos.options().dtype(torch::kLong));
  auto csum = count.to(torch::kLong).cumsum(0);
  offs.slice(0, 1, N).copy_(csum.slice(0, 0, N - 1));
  long E = N > 0 ? csum[-1].item<long>() : 0;
  auto src = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dst = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dist = torch::empty({E}, pos.options().dtype(torch::kFloat));
  if (E > 0) {
    LAUNCH(radius_fill_kernel, N, 2048, pos.data_ptr<float>(),
           b.data_ptr<long>(), gp.data_ptr<long>(), offs.data_ptr<long>(), N,
           r2, loop, src.data_ptr<long>(), dst.data_ptr<long>(),
           dist.data_ptr<float>());
  }
  return {src, dst, dist};
}

// defined in mfma_linear.hip
torch::Tensor mfma_linear(torch::Tensor A, torch::Tensor B,
                          c10::optional<torch::Tensor> bias, bool trans_b);

// defined in etp.hip
torch::Tensor etp_general(torch::Tensor A, torch::Tensor B, torch::Tensor C,
                          torch::Tensor entries, torch::Tensor coefs,
                          long do_,
                          c10::optional<torch::Tensor> ai,
                          c10::optional<torch::Tensor> bi,
                          c10::optional<torch::Tensor> ci, long n_rows,
                          long static_id);
torch::Tensor etp_nodesum(torch::Tensor A, torch::Tensor B,
                          torch::Tensor C, torch::Tensor entries,
                          torch::Tensor coefs, long do_,
                          torch::Tensor rowptr,
                          c10::optional<torch::Tensor> ai,
                          c10::optional<torch::Tensor> bi,
                          c10::optional<torch::Tensor> ci);
torch::Tensor etp_reduce(torch::Tensor A, torch::Tensor C, torch::Tensor D,
                         torch::Tensor entries, torch::Tensor coefs,
                         long db,
                         c10::optional<torch::Tensor> ai,
                         c10::optional<torch::Tensor> ci,
                         c10::optional<torch::Tensor> di, long n_rows);
std::vector<torch::Tensor> etp_sweep(
    torch::Tensor A, torch::Tensor B, torch::Tensor G, torch::Tensor O,
    c10::optional<torch::Tensor> tA, c10::optional<torch::Tensor> tB,
    c10::optional<torch::Tensor> tG, c10::optional<torch::Tensor> tO,
    torch::Tensor entries, torch::Tensor coefs, long omask, long order,
    long static_id);
long etp_sweep_lds_bytes(long da, long db, long dg, long do_, long n_ent,
                         long tmask, long omask, long acc_bytes);
long etp_form_lds_bytes(long da, long db, long dg, long do_, long n_ent,
                        long acc_bytes, bool b_out, bool staged);
// defined in etp_static.hip
bool etp_static_supported(long table_id, long order, long omask,
                          long tmask);
std::vector<long> etp_path_counts();

// defined in varlen_attn.hip
torch::Tensor varlen_attention(torch::Tensor Q, torch::Tensor K,
                               torch::Tensor V, torch::Tensor ptr);
std::vector<torch::Tensor> varlen_attention_fwd(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V,
    torch::Tensor ptr);
std::vector<torch::Tensor> varlen_attention_bwd(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V, torch::Tensor O,
    torch::Tensor LSE, torch::Tensor dO, torch::Tensor ptr);
long varlen_attention_lds_bytes(long dh, long pass);
std::vector<long> varlen_attention_tiling(long dh);
std::vector<torch::Tensor> varlen_attention_bwd2(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V, torch::Tensor O,
    torch::Tensor LSE, torch::Tensor dO, torch::Tensor cQ,
    torch::Tensor cK, torch::Tensor cV, torch::Tensor ptr);
std::vector<long> varlen_attention_tiling2(long dh);

// defined in irreps_linear.hip
torch::Tensor irreps_linear(torch::Tensor X, torch::Tensor W,
                            torch::Tensor lmap,
                            c10::optional<torch::Tensor> bias,
                            bool trans_w,
                            c10::optional<torch::Tensor> add);
torch::Tensor irreps_linear_gw(torch::Tensor X, torch::Tensor G,
                               torch::Tensor lmap, long L,
                               long nblocks);
// defined in gemv.hip
torch::Tensor gemv_small_n(torch::Tensor A, torch::Tensor W,
                           c10::optional<torch::Tensor> bias);
// defined in fused_adamw.hip
void fused_adamw(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                 torch::Tensor v, torch::Tensor step, torch::Tensor bc,
                 double lr, double beta1, double beta2, double eps,
                 double wd);
void fused_adamw_bf16(torch::Tensor p, torch::Tensor g,
                      torch::Tensor master, torch::Tensor m,
                      torch::Tensor v, torch::Tensor step,
                      torch::Tensor bc, double lr, double beta1,
                      double beta2, double eps, double wd);
// defined in radius.hip
std::vector<torch::Tensor> radius_pairs_t(torch::Tensor pos,
                                          torch::Tensor batch,
                                          torch::Tensor gptr, double r,
                                          bool loop,
                                          c10::optional<torch::Tensor> shifts);
std::vector<torch::Tensor> radius_pairs_cells(
    torch::Tensor pos, torch::Tensor order, torch::Tensor cell_of,
    torch::Tensor cell_start, long ncx, long ncy, long ncz, double r,
    bool loop);
// defined in symcon.hip
torch::Tensor symcon_forward(torch::Tensor x, torch::Tensor elem,
                             torch::Tensor W, torch::Tensor ent,
                             torch::Tensor coef, long Do);
std::vector<torch::Tensor> symcon_grad(
    torch::Tensor x, torch::Tensor g, c10::optional<torch::Tensor> t,
    torch::Tensor W, torch::Tensor perm, torch::Tensor rowptr,
    torch::Tensor ent, torch::Tensor coef, long mask);
long symcon_lds_bytes(long D, long Do, long P, long K, long order,
                      long acc_bytes);
std::vector<long> symcon_grad_geometry(long N, long C, long D, long Do,
                                       long P, long K, long order,
                                       long nel, bool dbl);

// defined in segment_linear.hip
torch::Tensor segment_outer_sum(torch::Tensor A, torch::Tensor B,
                                torch::Tensor ptr, long z);
torch::Tensor segment_matvec(torch::Tensor A, torch::Tensor K,
                             torch::Tensor ptr, bool trans);
long segment_linear_lds_bytes(long a, long b, at::ScalarType dtype,
                              long pass);
std::vector<long> segment_linear_tiling(long a, long b,
                                        at::ScalarType dtype);

// defined in pna_aggr.hip
std::vector<torch::Tensor> pna_fwd(torch::Tensor x, torch::Tensor rowptr,
                                   c10::optional<torch::Tensor> perm,
                                   torch::Tensor scale,
                                   std::vector<long> aggs);
torch::Tensor pna_bwd(torch::Tensor x, torch::Tensor rowptr,
                      c10::optional<torch::Tensor> perm,
                      torch::Tensor scale, std::vector<long> aggs,
                      torch::Tensor stats, torch::Tensor arg,
                      torch::Tensor G);
std::vector<torch::Tensor> pna_bwd2(torch::Tensor x, torch::Tensor rowptr,
                                    c10::optional<torch::Tensor> perm,
                                    torch::Tensor scale,
                                    std::vector<long> aggs,
                                    torch::Tensor stats, torch::Tensor arg,
                                    torch::Tensor G, torch::Tensor c,
                                    bool need_G, bool need_x);
long pna_grid_blocks(long n_threads);

// defined in gather_mul.hip
torch::Tensor gather_mul_sum(torch::Tensor x, torch::Tensor w,
                             c10::optional<torch::Tensor> gidx,
                             torch::Tensor rowptr,
                             c10::optional<torch::Tensor> perm);
torch::Tensor gather_mul(torch::Tensor a, torch::Tensor b,
                         c10::optional<torch::Tensor> ia,
                         c10::optional<torch::Tensor> ib, long E);

// defined in act_linear.hip
torch::Tensor act_linear_fwd(torch::Tensor h, torch::Tensor W,
                             c10::optional<torch::Tensor> bias);
torch::Tensor act_linear_dgrad(torch::Tensor g, torch::Tensor W,
                               torch::Tensor h);
torch::Tensor act_linear_dgrad_dg(torch::Tensor u, torch::Tensor W,
                                  torch::Tensor h);
torch::Tensor act_linear_dgrad_dh(torch::Tensor u, torch::Tensor g,
                                  torch::Tensor W, torch::Tensor h);
std::vector<torch::Tensor> act_linear_wgrad(
    torch::Tensor g, torch::Tensor x, c10::optional<torch::Tensor> u,
    bool act, bool want_bias);
long act_linear_wgrad_chunks(long E);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("act_linear_fwd", &act_linear_fwd,
        "y = bf16(silu(h)) W^T + b (HIP)",
        pybind11::arg("h"), pybind11::arg("W"),
        pybind11::arg("bias") = pybind11::none());
  m.def("act_linear_dgrad", &act_linear_dgrad,
        "gh = (g W) silu'(h) (HIP)",
        pybind11::arg("g"), pybind11::arg("W"), pybind11::arg("h"));
  m.def("act_linear_dgrad_dg", &act_linear_dgrad_dg,
        "dg = bf16(u silu'(h)) W^T (HIP)",
        pybind11::arg("u"), pybind11::arg("W"), pybind11::arg("h"));
  m.def("act_linear_dgrad_dh", &act_linear_dgrad_dh,
        "dh = u (g W) silu''(h) (HIP)",
        pybind11::arg("u"), pybind11::arg("g"), pybind11::arg("W"),
        pybind11::arg("h"));
  m.def("act_linear_wgrad", &act_linear_wgrad,
        "(gW, gb) = (g^T p, column sum of g), p = x, bf16(silu(x)) or "
        "bf16(u silu'(x)) (HIP)",
        pybind11::arg("g"), pybind11::arg("x"),
        pybind11::arg("u") = pybind11::none(),
        pybind11::arg("act") = true, pybind11::arg("want_bias") = false);
  m.def("act_linear_wgrad_chunks", &act_linear_wgrad_chunks,
        "E-chunks of an act_linear_wgrad launch: a function of E alone");
  m.def("gather_mul_sum", &gather_mul_sum,
        "out[i] = sum over CSR row i of x[gidx[e]] * w[e] (HIP); an "
        "absent gidx is the identity",
        pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("gidx"),
        pybind11::arg("rowptr"), pybind11::arg("perm"));
  m.def("gather_mul", &gather_mul,
        "out[e] = a[ia[e]] * b[ib[e]] (HIP); an absent index is the "
        "identity",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("ia"),
        pybind11::arg("ib"), pybind11::arg("E"));
  m.def("pna_fwd", &pna_fwd,
        "fused PNA aggregation -> (out, stats, arg) (HIP); aggregator "
        "ids: 0 sum, 1 mean, 2 min, 3 max, 4 std, 5 var",
        pybind11::arg("x"), pybind11::arg("rowptr"), pybind11::arg("perm"),
        pybind11::arg("scale"), pybind11::arg("aggs"));
  m.def("pna_bwd", &pna_bwd, "fused PNA aggregation backward -> dx (HIP)",
        pybind11::arg("x"), pybind11::arg("rowptr"), pybind11::arg("perm"),
        pybind11::arg("scale"), pybind11::arg("aggs"),
        pybind11::arg("stats"), pybind11::arg("arg"), pybind11::arg("G"));
  m.def("pna_bwd2", &pna_bwd2,
        "fused PNA aggregation second order -> (hG, gx) (HIP)",
        pybind11::arg("x"), pybind11::arg("rowptr"), pybind11::arg("perm"),
        pybind11::arg("scale"), pybind11::arg("aggs"),
        pybind11::arg("stats"), pybind11::arg("arg"), pybind11::arg("G"),
        pybind11::arg("c"), pybind11::arg("need_G"),
        pybind11::arg("need_x"));
  m.def("pna_grid_blocks", &pna_grid_blocks,
        "blocks of a PNA launch over n (row, feature) threads");
  m.def("segment_outer_sum", &segment_outer_sum,
        "per-segment outer-product sum -> K[G, H, a, b] in the "
        "accumulator type (HIP); z <= 0 picks the row split",
        pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("ptr"),
        pybind11::arg("z") = 0);
  m.def("segment_matvec", &segment_matvec,
        "per-row product with the row's segment matrix (HIP)",
        pybind11::arg("A"), pybind11::arg("K"), pybind11::arg("ptr"),
        pybind11::arg("trans") = false);
  m.def("segment_linear_lds_bytes", &segment_linear_lds_bytes,
        "dynamic-LDS bytes of a segment-linear launch "
        "(pass 0 outer sum, 1 matvec, 2 matvec trans)",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("dtype"),
        pybind11::arg("pass"));
  m.def("segment_linear_tiling", &segment_linear_tiling,
        "(outer-sum row tile R, matvec rows per workgroup pass)",
        pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("dtype"));
  m.def("symcon_forward", &symcon_forward,
        "fused symmetric contraction, whole output tower (HIP)");
  m.def("symcon_grad", &symcon_grad,
        "symmetric contraction first order (t None) or second order "
        "(HIP); mask bits: 1 x, 2 W, 4 g",
        pybind11::arg("x"), pybind11::arg("g"), pybind11::arg("t"),
        pybind11::arg("W"), pybind11::arg("perm"),
        pybind11::arg("rowptr"), pybind11::arg("ent"),
        pybind11::arg("coef"), pybind11::arg("mask"));
  m.def("symcon_lds_bytes", &symcon_lds_bytes,
        "dynamic-LDS bytes of a symcon launch (order 0 = forward)");
  m.def("symcon_grad_geometry", &symcon_grad_geometry,
        "(block, channel tile, row lanes, Z, channel tiles) of a "
        "symcon_grad launch");
  m.def("etp_general", &etp_general, "fused ETP contraction (HIP)",
        pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("C"),
        pybind11::arg("entries"), pybind11::arg("coefs"),
        pybind11::arg("do_"),
        pybind11::arg("ai") = pybind11::none(),
        pybind11::arg("bi") = pybind11::none(),
        pybind11::arg("ci") = pybind11::none(),
        pybind11::arg("n_rows") = 0, pybind11::arg("static_id") = -1);
  m.def("etp_nodesum", &etp_nodesum, "fused gather+TP+segment sum (HIP)",
        pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("C"),
        pybind11::arg("entries"), pybind11::arg("coefs"),
        pybind11::arg("do_"), pybind11::arg("rowptr"),
        pybind11::arg("ai") = pybind11::none(),
        pybind11::arg("bi") = pybind11::none(),
        pybind11::arg("ci") = pybind11::none());
  m.def("mfma_linear", &mfma_linear, "bf16 MFMA linear (HIP)",
        pybind11::arg("A"), pybind11::arg("B"),
        pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("trans_b") = true);
  m.def("etp_reduce", &etp_reduce, "fused ETP channel-reduce (HIP)",
        pybind11::arg("A"), pybind11::arg("C"), pybind11::arg("D"),
        pybind11::arg("entries"), pybind11::arg("coefs"),
        pybind11::arg("db"),
        pybind11::arg("ai") = pybind11::none(),
        pybind11::arg("ci") = pybind11::none(),
        pybind11::arg("di") = pybind11::none(),
        pybind11::arg("n_rows") = 0);
  m.def("etp_sweep", &etp_sweep,
        "several derivatives of the ETP form in one launch (HIP)",
        pybind11::arg("A"), pybind11::arg("B"), pybind11::arg("G"),
        pybind11::arg("O"), pybind11::arg("tA") = pybind11::none(),
        pybind11::arg("tB") = pybind11::none(),
        pybind11::arg("tG") = pybind11::none(),
        pybind11::arg("tO") = pybind11::none(),
        pybind11::arg("entries"), pybind11::arg("coefs"),
        pybind11::arg("omask"), pybind11::arg("order") = 1,
        pybind11::arg("static_id") = -1);
  m.def("etp_sweep_lds_bytes", &etp_sweep_lds_bytes,
        "dynamic-LDS bytes of one etp_sweep block");
  m.def("etp_form_lds_bytes", &etp_form_lds_bytes,
        "dynamic-LDS bytes of one block of the single-output ETP form "
        "(o-type or b-type output, rows staged or read through L1)",
        pybind11::arg("da"), pybind11::arg("db"), pybind11::arg("dg"),
        pybind11::arg("do_"), pybind11::arg("n_ent"),
        pybind11::arg("acc_bytes"), pybind11::arg("b_out"),
        pybind11::arg("staged"));
  m.def("etp_static_supported", &etp_static_supported,
        "whether (static table id, order, omask, tmask) has a "
        "compile-time-table ETP kernel");
  m.def("etp_path_counts", &etp_path_counts,
        "(static-table, run-time-table) ETP launches so far");
  m.def("gather_fwd", &gather_fwd, "gather rows (HIP)");
  m.def("scatter_sum_fwd", &scatter_sum_fwd, "scatter-add (HIP)");
  m.def("segment_sum_csr", &segment_sum_csr, "CSR segment sum (HIP)",
        pybind11::arg("src"), pybind11::arg("rowptr"),
        pybind11::arg("perm") = pybind11::none(),
        pybind11::arg("mean") = false);
  m.def("scatter_mean_fwd", &scatter_mean_fwd, "scatter-mean (HIP)");
  m.def("scatter_minmax_fwd", &scatter_minmax_fwd, "scatter-min/max (HIP)");
  m.def("radius_pairs", &radius_pairs, "radius pair enumeration (HIP)");
  m.def("fused_adamw", &fused_adamw,
        "single-kernel flat AdamW (HIP)");
  m.def("fused_adamw_bf16", &fused_adamw_bf16,
        "single-kernel flat AdamW, bf16 params + fp32 master (HIP)");
  m.def("radius_pairs_cells", &radius_pairs_cells,
        "cell-list radius pairs for large graphs (HIP)");
  m.def("radius_pairs_t", &radius_pairs_t,
        "tiled fp32/fp64 radius pairs, open or periodic (HIP)",
        pybind11::arg("pos"), pybind11::arg("batch"),
        pybind11::arg("gptr"), pybind11::arg("r"),
        pybind11::arg("loop") = false,
        pybind11::arg("shifts") = pybind11::none());
  m.def("varlen_attention", &varlen_attention,
        "segment-varlen attention (HIP)");
  m.def("varlen_attention_fwd", &varlen_attention_fwd,
        "segment-varlen attention forward -> (O, LSE) (HIP)");
  m.def("varlen_attention_bwd", &varlen_attention_bwd,
        "segment-varlen attention backward -> (dQ, dK, dV) (HIP)");
  m.def("varlen_attention_lds_bytes", &varlen_attention_lds_bytes,
        "LDS bytes of a varlen-attention instance "
        "(pass 0 fwd, 1 dQ, 2 dK/dV, 3 and 4 second order)",
        pybind11::arg("dh"), pybind11::arg("pass"));
  m.def("varlen_attention_tiling", &varlen_attention_tiling,
        "(tile rows, rows per workgroup pass) of the instance for dh");
  m.def("varlen_attention_bwd2", &varlen_attention_bwd2,
        "segment-varlen attention second order -> (gQ, gK, gV, gdO) "
        "(HIP)");
  m.def("varlen_attention_tiling2", &varlen_attention_tiling2,
        "(tile rows, rows per workgroup pass) of the second-order "
        "instance for dh");
  m.def("irreps_linear", &irreps_linear,
        "per-l channel-mixing MFMA linear (HIP)",
        pybind11::arg("X"), pybind11::arg("W"), pybind11::arg("lmap"),
        pybind11::arg("bias") = pybind11::none(),
        pybind11::arg("trans_w") = false,
        pybind11::arg("add") = pybind11::none());
  m.def("gemv_small_n", &gemv_small_n,
        "narrow-output bf16 linear (HIP)",
        pybind11::arg("A"), pybind11::arg("W"),
        pybind11::arg("bias") = pybind11::none());
  m.def("irreps_linear_gw", &irreps_linear_gw,
        "irreps-linear weight-grad partials (HIP)",
        pybind11::arg("X"), pybind11::arg("G"), pybind11::arg("lmap"),
        pybind11::arg("L"), pybind11::arg("nblocks") = 512);
}
