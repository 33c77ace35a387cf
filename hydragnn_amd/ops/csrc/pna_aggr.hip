// Fused PNA aggregation for MI355X (gfx950, CDNA4): every aggregator
// (sum, mean, min, max, std, var) times every degree scaler of
// DegreeScalerAggregation in one pass over the CSR rows, with its
// first- and second-order backward closed on the device.
//
// Mapping, shared by the three kernels: one thread per (row, feature),
// grid-stride.  Consecutive lanes hold consecutive features, so each
// step of a row walk reads one contiguous piece of an edge's feature
// row.  No atomics and no zero-fill: every output element has exactly
// one writer.  Every sum runs in ascending position within the row,
// from 0, in the accumulator type (fp32 for bf16/f16), so results are
// bitwise reproducible and the sorted route equals the perm route.
//
// Rows are positions rowptr[i] .. rowptr[i+1] of the edge list, or of
// perm (a stable argsort of an unsorted index) when one is given.
//
//   mu = sum x / n,  v = sum (x - mu)^2 / n (second walk of the row),
//   var = v,  std = sqrt(v + 1e-5);  an empty row gives mu = v = 0.
//   min/max: the lowest position attaining the extreme wins; presence
//   is decided by the arg (-1 = empty row, value 0), so +-inf count.
//
// The aggregator values are named scalars picked through a select
// chain, never a runtime-indexed array: no scratch.

#include <torch/extension.h>
#include <ATen/OpMathType.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include <hip/hip_runtime.h>

#include <limits>

namespace {

constexpr int kBlock = 256;
constexpr int kGridCap = 8192;
constexpr int kMaxAgg = 6;      // sum mean min max std var, each once
constexpr int kMaxScale = 8;

enum : int { A_SUM = 0, A_MEAN, A_MIN, A_MAX, A_STD, A_VAR };

struct PnaCfg {
  int A;                 // aggregators in the output, in order
  int S;                 // scalers
  int mask;              // bit a set: aggregator a present
  int agg[kMaxAgg];      // ids, output order
  int pos[kMaxAgg];      // column of each id in the output, -1: absent
};

__device__ inline bool has(int mask, int a) { return (mask >> a) & 1; }

template <typename ACC>
__device__ inline ACC pna_sqrt(ACC x);
template <>
__device__ inline float pna_sqrt<float>(float x) { return sqrtf(x); }
template <>
__device__ inline double pna_sqrt<double>(double x) { return sqrt(x); }

// position -> edge
__device__ inline long edge_of(const long* __restrict__ perm, long p) {
  return perm ? perm[p] : p;
}

// ---------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------
template <typename T, typename ACC>
__global__ void pna_fwd_kernel(const T* __restrict__ x,
                               const long* __restrict__ rowptr,
                               const long* __restrict__ perm,
                               const ACC* __restrict__ scale,
                               T* __restrict__ out,
                               ACC* __restrict__ stats,   // [N, F, 2]
                               int* __restrict__ arg,     // [N, F, 2]
                               long N, long F, PnaCfg cfg) {
  const long total = N * F;
  const bool want_var = has(cfg.mask, A_STD) || has(cfg.mask, A_VAR);
  const bool want_ext = has(cfg.mask, A_MIN) || has(cfg.mask, A_MAX);
  const long width = (long)cfg.S * cfg.A * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / F;
    const long f = i - r * F;
    const long lo = rowptr[r], hi = rowptr[r + 1];
    ACC sum = (ACC)0, mn = (ACC)0, mx = (ACC)0;
    int amn = -1, amx = -1;
    for (long p = lo; p < hi; ++p) {
      const ACC v = (ACC)x[edge_of(perm, p) * F + f];
      sum += v;
      if (amn < 0 || v < mn) { mn = v; amn = (int)p; }
      if (amx < 0 || v > mx) { mx = v; amx = (int)p; }
    }
    const ACC mean = hi > lo ? sum / (ACC)(hi - lo) : (ACC)0;
    ACC var = (ACC)0;
    if (want_var && hi > lo) {
      ACC ss = (ACC)0;
      for (long p = lo; p < hi; ++p) {
        const ACC d = (ACC)x[edge_of(perm, p) * F + f] - mean;
        ss += d * d;
      }
      var = ss / (ACC)(hi - lo);
    }
    const ACC sd = pna_sqrt<ACC>(var + (ACC)1e-5);
    if (want_var) {
      stats[i * 2] = mean;
      stats[i * 2 + 1] = var;
    }
    if (want_ext) {
      arg[i * 2] = amn;
      arg[i * 2 + 1] = amx;
    }
    T* o = out + r * width + f;
    for (int s = 0; s < cfg.S; ++s) {
      const ACC sc = scale[r * cfg.S + s];
      for (int a = 0; a < cfg.A; ++a) {
        const int id = cfg.agg[a];
        const ACC val = id == A_SUM ? sum : id == A_MEAN ? mean
                      : id == A_MIN ? mn : id == A_MAX ? mx
                      : id == A_STD ? sd : var;
        o[(long)(s * cfg.A + a) * F] = (T)(val * sc);
      }
    }
  }
}

// g_a = sum_s scale[r, s] G[r, s, a, f], each aggregator in a named
// scalar.  The column of aggregator id k is cfg.pos[k], a constant
// index into the kernel argument: the six sums stay in registers (a
// chain of `if (id == ...) g_... += v` is turned into an indexed array
// in scratch by the compiler).
template <typename T, typename ACC>
__device__ inline ACC fold_one(const T* __restrict__ g,
                               const ACC* __restrict__ sc, int S, int A,
                               int pos, long F) {
  ACC acc = (ACC)0;
  if (pos >= 0)
    for (int s = 0; s < S; ++s)
      acc += sc[s] * (ACC)g[(long)(s * A + pos) * F];
  return acc;
}

template <typename T, typename ACC>
__device__ inline void fold_scalers(const T* __restrict__ G,
                                    const ACC* __restrict__ scale, long r,
                                    long f, long F, const PnaCfg& cfg,
                                    ACC& g_sum, ACC& g_mean, ACC& g_min,
                                    ACC& g_max, ACC& g_std, ACC& g_var) {
  const T* g = G + r * ((long)cfg.S * cfg.A * F) + f;
  const ACC* sc = scale + r * cfg.S;
  g_sum = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_SUM], F);
  g_mean = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_MEAN], F);
  g_min = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_MIN], F);
  g_max = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_MAX], F);
  g_std = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_STD], F);
  g_var = fold_one<T, ACC>(g, sc, cfg.S, cfg.A, cfg.pos[A_VAR], F);
}

// ---------------------------------------------------------------------
// first-order backward: one store per element of dx
// ---------------------------------------------------------------------
template <typename T, typename ACC>
__global__ void pna_bwd_kernel(const T* __restrict__ x,
                               const long* __restrict__ rowptr,
                               const long* __restrict__ perm,
                               const ACC* __restrict__ scale,
                               const ACC* __restrict__ stats,
                               const int* __restrict__ arg,
                               const T* __restrict__ G,
                               T* __restrict__ dx, long N, long F,
                               PnaCfg cfg) {
  const long total = N * F;
  const bool want_var = has(cfg.mask, A_STD) || has(cfg.mask, A_VAR);
  const bool want_ext = has(cfg.mask, A_MIN) || has(cfg.mask, A_MAX);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / F;
    const long f = i - r * F;
    const long lo = rowptr[r], hi = rowptr[r + 1];
    if (hi <= lo) continue;
    ACC g_sum, g_mean, g_min, g_max, g_std, g_var;
    fold_scalers<T, ACC>(G, scale, r, f, F, cfg, g_sum, g_mean, g_min,
                         g_max, g_std, g_var);
    const ACC n = (ACC)(hi - lo);
    const ACC base = g_sum + g_mean / n;
    ACC mean = (ACC)0, k = (ACC)0;
    if (want_var) {
      mean = stats[i * 2];
      const ACC sd = pna_sqrt<ACC>(stats[i * 2 + 1] + (ACC)1e-5);
      k = g_std / (n * sd) + (ACC)2 * g_var / n;
    }
    int amn = -1, amx = -1;
    if (want_ext) {
      amn = arg[i * 2];
      amx = arg[i * 2 + 1];
    }
    for (long p = lo; p < hi; ++p) {
      const long e = edge_of(perm, p) * F + f;
      ACC d = base;
      if ((int)p == amx) d += g_max;
      if ((int)p == amn) d += g_min;
      // x - mu may be inf/nan where only min/max are asked for
      if (want_var) d += k * ((ACC)x[e] - mean);
      dx[e] = (T)d;
    }
  }
}

// ---------------------------------------------------------------------
// second order: the backward of pna_bwd_kernel.  With c the cotangent
// of dx, R = <c, dx>, y = x - mu, Cbar = sum c / n, Sc = sum c y:
//   dR/dG[r, s, a, f] = scale[r, s] h_a,
//     h_sum = sum c, h_mean = Cbar, h_max = c[argmax],
//     h_min = c[argmin], h_std = Sc / (n sd), h_var = 2 Sc / n;
//   dR/dx_k = g_std / (n sd) [(c_k - Cbar) - Sc y_k / (n sd^2)]
//             + g_var (2 / n) (c_k - Cbar).
// Null hG / gx: that gradient is not needed.
// ---------------------------------------------------------------------
template <typename T, typename ACC>
__global__ void pna_bwd2_kernel(const T* __restrict__ x,
                                const long* __restrict__ rowptr,
                                const long* __restrict__ perm,
                                const ACC* __restrict__ scale,
                                const ACC* __restrict__ stats,
                                const int* __restrict__ arg,
                                const T* __restrict__ G,
                                const T* __restrict__ c,
                                T* __restrict__ hG, T* __restrict__ gx,
                                long N, long F, PnaCfg cfg) {
  const long total = N * F;
  const bool want_var = has(cfg.mask, A_STD) || has(cfg.mask, A_VAR);
  const bool want_ext = has(cfg.mask, A_MIN) || has(cfg.mask, A_MAX);
  const long width = (long)cfg.S * cfg.A * F;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / F;
    const long f = i - r * F;
    const long lo = rowptr[r], hi = rowptr[r + 1];
    ACC mean = (ACC)0, sd = (ACC)1;
    if (want_var) {
      mean = stats[i * 2];
      sd = pna_sqrt<ACC>(stats[i * 2 + 1] + (ACC)1e-5);
    }
    ACC sum_c = (ACC)0, sc_y = (ACC)0;
    for (long p = lo; p < hi; ++p) {
      const long e = edge_of(perm, p) * F + f;
      const ACC ce = (ACC)c[e];
      sum_c += ce;
      if (want_var) sc_y += ce * ((ACC)x[e] - mean);
    }
    const ACC n = (ACC)(hi - lo);
    const ACC cbar = hi > lo ? sum_c / n : (ACC)0;
    if (hG) {
      ACC h_min = (ACC)0, h_max = (ACC)0;
      if (want_ext && hi > lo) {
        h_min = (ACC)c[edge_of(perm, arg[i * 2]) * F + f];
        h_max = (ACC)c[edge_of(perm, arg[i * 2 + 1]) * F + f];
      }
      const ACC h_std = hi > lo ? sc_y / (n * sd) : (ACC)0;
      const ACC h_var = hi > lo ? (ACC)2 * sc_y / n : (ACC)0;
      T* o = hG + r * width + f;
      for (int s = 0; s < cfg.S; ++s) {
        const ACC sc = scale[r * cfg.S + s];
        for (int a = 0; a < cfg.A; ++a) {
          const int id = cfg.agg[a];
          const ACC h = id == A_SUM ? sum_c : id == A_MEAN ? cbar
                      : id == A_MIN ? h_min : id == A_MAX ? h_max
                      : id == A_STD ? h_std : h_var;
          o[(long)(s * cfg.A + a) * F] = (T)(sc * h);
        }
      }
    }
    if (gx && hi > lo) {
      ACC g_sum, g_mean, g_min, g_max, g_std, g_var;
      fold_scalers<T, ACC>(G, scale, r, f, F, cfg, g_sum, g_mean, g_min,
                           g_max, g_std, g_var);
      const ACC ks = g_std / (n * sd);
      const ACC kv = (ACC)2 * g_var / n;
      const ACC q = sc_y / (n * sd * sd);
      for (long p = lo; p < hi; ++p) {
        const long e = edge_of(perm, p) * F + f;
        const ACC dc = (ACC)c[e] - cbar;
        const ACC y = (ACC)x[e] - mean;
        gx[e] = (T)(ks * (dc - q * y) + kv * dc);
      }
    }
  }
}

inline int n_blocks(long total) {
  long b = (total + kBlock - 1) / kBlock;
  return (int)std::min<long>(b, kGridCap);
}

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

inline long row_elems(const torch::Tensor& t) {
  long f = 1;
  for (int64_t d = 1; d < t.dim(); ++d) f *= t.size(d);
  return f;
}

struct Operands {
  long E, N, F;
  PnaCfg cfg;
  torch::Tensor rp, pc;
  const long* perm;
};

Operands check_operands(const torch::Tensor& x, const torch::Tensor& rowptr,
                        const c10::optional<torch::Tensor>& perm,
                        const torch::Tensor& scale,
                        const std::vector<long>& aggs) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
              "msg must be a contiguous GPU tensor");
  TORCH_CHECK(x.dim() >= 2, "msg needs a row and a feature dim");
  TORCH_CHECK(rowptr.is_cuda() && rowptr.dtype() == torch::kLong &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "rowptr must be int64 [N + 1] on the device");
  Operands o;
  o.E = x.size(0);
  o.N = rowptr.numel() - 1;
  o.F = row_elems(x);
  TORCH_CHECK(o.E < (1L << 31), "pna_aggregate stores args as int32: "
              "E must be below 2^31");
  TORCH_CHECK(!aggs.empty() && (long)aggs.size() <= kMaxAgg,
              "1 to 6 aggregators");
  o.cfg.A = (int)aggs.size();
  o.cfg.mask = 0;
  for (int a = 0; a < kMaxAgg; ++a) {
    o.cfg.agg[a] = 0;
    o.cfg.pos[a] = -1;
  }
  for (int a = 0; a < o.cfg.A; ++a) {
    TORCH_CHECK(aggs[a] >= 0 && aggs[a] < kMaxAgg, "unknown aggregator id");
    TORCH_CHECK(!((o.cfg.mask >> aggs[a]) & 1), "aggregator given twice");
    o.cfg.agg[a] = (int)aggs[a];
    o.cfg.pos[aggs[a]] = a;
    o.cfg.mask |= 1 << aggs[a];
  }
  TORCH_CHECK(scale.is_cuda() && scale.is_contiguous() && scale.dim() == 2 &&
                  scale.size(0) == o.N && scale.size(1) >= 1 &&
                  scale.size(1) <= kMaxScale,
              "scale must be contiguous [N, S], 1 <= S <= 8");
  auto acc_type = x.scalar_type() == at::ScalarType::Double
                      ? at::ScalarType::Double : at::ScalarType::Float;
  TORCH_CHECK(scale.scalar_type() == acc_type,
              "scale must be in the accumulator type");
  o.cfg.S = (int)scale.size(1);
  o.rp = rowptr.contiguous();
  o.perm = nullptr;
  if (perm.has_value()) {
    TORCH_CHECK(perm->is_cuda() && perm->dtype() == torch::kLong &&
                    perm->numel() == o.E,
                "perm must be int64 [E] on the device");
    o.pc = perm->contiguous();
    o.perm = o.pc.data_ptr<long>();
  }
  return o;
}

void check_saved(const Operands& o, const torch::Tensor& x,
                 const torch::Tensor& stats, const torch::Tensor& arg,
                 const torch::Tensor& G) {
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() &&
                  stats.numel() == o.N * o.F * 2,
              "stats must be contiguous [N, F, 2]");
  TORCH_CHECK(arg.is_cuda() && arg.is_contiguous() &&
                  arg.dtype() == torch::kInt && arg.numel() == o.N * o.F * 2,
              "arg must be contiguous int32 [N, F, 2]");
  TORCH_CHECK(G.is_cuda() && G.is_contiguous() &&
                  G.scalar_type() == x.scalar_type() &&
                  G.numel() == o.N * (long)o.cfg.S * o.cfg.A * o.F,
              "grad_out must be contiguous [N, S*A*F] in msg's dtype");
}

}  // namespace

// (out [N, S*A*F], stats [N, F, 2] accumulator type, arg [N, F, 2] int32)
std::vector<torch::Tensor> pna_fwd(torch::Tensor x, torch::Tensor rowptr,
                                   c10::optional<torch::Tensor> perm,
                                   torch::Tensor scale,
                                   std::vector<long> aggs) {
  Operands o = check_operands(x, rowptr, perm, scale, aggs);
  auto out = torch::empty({o.N, (long)o.cfg.S * o.cfg.A * o.F}, x.options());
  auto stats = torch::empty({o.N, o.F, 2}, scale.options());
  auto arg = torch::empty({o.N, o.F, 2}, x.options().dtype(torch::kInt));
  if (o.N * o.F == 0) return {out, stats, arg};
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(),
      "pna_fwd", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        hipLaunchKernelGGL((pna_fwd_kernel<scalar_t, acc_t>),
                           dim3(n_blocks(o.N * o.F)), dim3(kBlock), 0,
                           cur_stream(), x.data_ptr<scalar_t>(),
                           o.rp.data_ptr<long>(), o.perm,
                           scale.data_ptr<acc_t>(),
                           out.data_ptr<scalar_t>(),
                           stats.data_ptr<acc_t>(), arg.data_ptr<int>(),
                           o.N, o.F, o.cfg);
        C10_HIP_KERNEL_LAUNCH_CHECK();
      });
  return {out, stats, arg};
}

// dx [E, ...] for the cotangent G of out; rowptr[N] must equal E
torch::Tensor pna_bwd(torch::Tensor x, torch::Tensor rowptr,
                      c10::optional<torch::Tensor> perm,
                      torch::Tensor scale, std::vector<long> aggs,
                      torch::Tensor stats, torch::Tensor arg,
                      torch::Tensor G) {
  Operands o = check_operands(x, rowptr, perm, scale, aggs);
  check_saved(o, x, stats, arg, G);
  auto dx = torch::empty_like(x);
  if (o.N * o.F == 0 || o.E == 0) return dx;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(),
      "pna_bwd", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        hipLaunchKernelGGL((pna_bwd_kernel<scalar_t, acc_t>),
                           dim3(n_blocks(o.N * o.F)), dim3(kBlock), 0,
                           cur_stream(), x.data_ptr<scalar_t>(),
                           o.rp.data_ptr<long>(), o.perm,
                           scale.data_ptr<acc_t>(),
                           stats.data_ptr<acc_t>(), arg.data_ptr<int>(),
                           G.data_ptr<scalar_t>(),
                           dx.data_ptr<scalar_t>(), o.N, o.F, o.cfg);
        C10_HIP_KERNEL_LAUNCH_CHECK();
      });
  return dx;
}

// (hG like G, gx like x); an output that is not needed, or is
// identically zero (gx without std/var), comes back undefined
std::vector<torch::Tensor> pna_bwd2(torch::Tensor x, torch::Tensor rowptr,
                                    c10::optional<torch::Tensor> perm,
                                    torch::Tensor scale,
                                    std::vector<long> aggs,
                                    torch::Tensor stats, torch::Tensor arg,
                                    torch::Tensor G, torch::Tensor c,
                                    bool need_G, bool need_x) {
  Operands o = check_operands(x, rowptr, perm, scale, aggs);
  check_saved(o, x, stats, arg, G);
  TORCH_CHECK(c.is_cuda() && c.is_contiguous() &&
                  c.scalar_type() == x.scalar_type() &&
                  c.numel() == x.numel(),
              "the cotangent of dx must be contiguous, like msg");
  const bool var_terms = (o.cfg.mask >> A_STD) & 1 || (o.cfg.mask >> A_VAR) & 1;
  need_x = need_x && var_terms;
  torch::Tensor hG, gx;
  if (need_G) hG = torch::empty_like(G);
  if (need_x) gx = torch::empty_like(x);
  if (o.N * o.F == 0 || !(need_G || need_x)) return {hG, gx};
  if (o.E == 0) {
    if (need_G) hG.zero_();
    return {hG, gx};
  }
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, x.scalar_type(),
      "pna_bwd2", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        hipLaunchKernelGGL((pna_bwd2_kernel<scalar_t, acc_t>),
                           dim3(n_blocks(o.N * o.F)), dim3(kBlock), 0,
                           cur_stream(), x.data_ptr<scalar_t>(),
                           o.rp.data_ptr<long>(), o.perm,
                           scale.data_ptr<acc_t>(),
                           stats.data_ptr<acc_t>(), arg.data_ptr<int>(),
                           G.data_ptr<scalar_t>(), c.data_ptr<scalar_t>(),
                           need_G ? hG.data_ptr<scalar_t>() : nullptr,
                           need_x ? gx.data_ptr<scalar_t>() : nullptr,
                           o.N, o.F, o.cfg);
        C10_HIP_KERNEL_LAUNCH_CHECK();
      });
  return {hG, gx};
}

// blocks a launch over n_threads (row, feature) pairs gets: the grid cap
long pna_grid_blocks(long n_threads) { return n_blocks(n_threads); }
