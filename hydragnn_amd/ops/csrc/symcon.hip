// Fused MACE symmetric contraction (CDNA4/gfx950).
//
// The product block is a small polynomial in the node's features with
// per-element weights.  With x~ = (x_0 .. x_{D-1}, 1) and W[e, p, c] the
// block's weights concatenated over (lout, nu):
//
//   out[n,c,o] = sum_k coef_k W[elem[n], p_k, c] x~[i_k] x~[j_k] x~[l_k]
//
// one entry per non-zero of each U^(nu); index D (the constant 1) fills
// the slots a lower order leaves unused.  The composition this replaces
// materialised U.w[elem[n]] for every node and folded it with x order by
// order.  Here one thread per (node, channel) reads its D features and P
// weights, walks the table and writes the whole output tower:
//
//   symcon_fwd_kernel     out
//   symcon_first_kernel   Q = <g, out>:  dQ/dx and per-workgroup dQ/dW
//   symcon_second_kernel  R = <t, dQ/dx>:  dR/dg, dR/dx and dR/dW
//   symcon_wsum_kernel    second stage of the weight-gradient sum
//
// Per-thread state that is indexed by table entries lives in LDS slices
// laid out [slot][thread] (conflict-free, and no runtime-indexed register
// arrays, the family's route to scratch).  Entry words are staged in LDS
// once per workgroup and read as wave-uniform broadcasts.
//
// Weight gradients sum over all nodes of an element without atomics and
// in a fixed order.  Nodes are sorted by element on the host side (perm,
// rowptr); workgroup (z, e) takes the row chunks z, z+Z, .. of element e,
// each thread accumulates its (row lane, channel) over those chunks, the
// row lanes are summed in order and the workgroup writes one fp32 partial
// [e, z, P, C].  symcon_wsum_kernel adds the partials of an element in a
// fixed order and rounds once.  Z depends on the host-known shapes only.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "check_launch.h"

namespace {

template <typename T> struct sc_acc { using type = float; };
template <> struct sc_acc<double> { using type = double; };

constexpr int SC_MAX_D = 9;      // D, Do
constexpr int SC_MAX_P = 32;
constexpr int SC_MAX_ENT = 1024;
constexpr size_t SC_LDS_BUDGET = 150 * 1024;
constexpr long SC_PARTIAL_BYTES = 64L << 20;

// entry word: o | p << 4 | i << 10 | j << 14 | l << 18
struct Ent { int o, p, i, j, l; };
__device__ __forceinline__ Ent unpack(int w) {
  Ent e;
  e.o = w & 15;
  e.p = (w >> 4) & 63;
  e.i = (w >> 10) & 15;
  e.j = (w >> 14) & 15;
  e.l = (w >> 18) & 15;
  return e;
}

// Forward: flat thread per (n, c).  Entries arrive sorted by o, so an
// output accumulates in a register and lands in its slice once.
template <typename T>
__global__ void symcon_fwd_kernel(
    const T* __restrict__ x, const long* __restrict__ elem,
    const T* __restrict__ W, T* __restrict__ out,
    const int* __restrict__ ent, const float* __restrict__ coef, int K,
    long N, int C, int D, int Do, int P, int nel) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename sc_acc<T>::type;
  const int B = blockDim.x, tid = threadIdx.x;
  ACC* xs = reinterpret_cast<ACC*>(smem);       // [D+1][B]
  ACC* ws = xs + (size_t)(D + 1) * B;           // [P][B]
  ACC* os = ws + (size_t)P * B;                 // [Do][B]
  int* ent_l = reinterpret_cast<int*>(os + (size_t)Do * B);
  float* coef_l = reinterpret_cast<float*>(ent_l + K);
  for (int k = tid; k < K; k += B) {
    ent_l[k] = ent[k];
    coef_l[k] = coef[k];
  }
  __syncthreads();
  const long idx = (long)blockIdx.x * B + tid;
  if (idx >= N * C) return;
  const long n = idx / C;
  const int c = (int)(idx - n * C);
  long e = elem[n];
  e = e < 0 ? 0 : (e >= nel ? nel - 1 : e);
  const T* xp = x + idx * D;
  for (int d = 0; d < D; ++d) xs[d * B + tid] = (ACC)xp[d];
  xs[D * B + tid] = (ACC)1;
  const T* wp = W + e * (long)P * C + c;
  for (int p = 0; p < P; ++p) ws[p * B + tid] = (ACC)wp[(long)p * C];
  for (int o = 0; o < Do; ++o) os[o * B + tid] = (ACC)0;
  int cur = 0;
  ACC acc = 0;
  for (int k = 0; k < K; ++k) {
    const Ent q = unpack(ent_l[k]);
    if (q.o != cur) {  // wave-uniform
      os[cur * B + tid] = acc;
      acc = 0;
      cur = q.o;
    }
    acc += (ACC)coef_l[k] * ws[q.p * B + tid] * xs[q.i * B + tid] *
           xs[q.j * B + tid] * xs[q.l * B + tid];
  }
  if (K > 0) os[cur * B + tid] = acc;
  T* op = out + idx * Do;
  for (int o = 0; o < Do; ++o) op[o] = (T)os[o * B + tid];
}

// First and second order share the sorted walk.  Grid (Z, nel, channel
// tiles); the block is CT channels x R row lanes.
//   ORDER 1: inputs x, g.      outputs ox = dQ/dx, partial = dQ/dW
//   ORDER 2: inputs x, g, t.   outputs og = dR/dg, ox = dR/dx,
//                              partial = dR/dW
// A null output pointer masks that output.
template <typename T, int ORDER>
__global__ void symcon_grad_kernel(
    const T* __restrict__ x, const T* __restrict__ g,
    const T* __restrict__ t, const T* __restrict__ W,
    const long* __restrict__ perm, const long* __restrict__ rowptr,
    T* __restrict__ ox, T* __restrict__ og,
    typename sc_acc<T>::type* __restrict__ partial,
    const int* __restrict__ ent, const float* __restrict__ coef, int K,
    long N, int C, int D, int Do, int P, int ct_log2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename sc_acc<T>::type;
  const int B = blockDim.x, tid = threadIdx.x;
  const int CT = 1 << ct_log2, R = B >> ct_log2;
  const int Z = gridDim.x, z = blockIdx.x, e = blockIdx.y;
  const int cl = tid & (CT - 1), r = tid >> ct_log2;
  const int c = blockIdx.z * CT + cl;

  long start = rowptr[e], cnt = rowptr[e + 1] - start;
  if (start < 0 || cnt < 0 || start + cnt > N) cnt = 0;
  const long nchunks = (cnt + R - 1) / R;
  if (z >= nchunks) return;  // whole workgroup, before any barrier

  ACC* xs = reinterpret_cast<ACC*>(smem);            // [D+1][B]
  ACC* gs = xs + (size_t)(D + 1) * B;                // [Do][B]
  ACC* ws = gs + (size_t)Do * B;                     // [P][B]
  ACC* rx = ws + (size_t)P * B;                      // [D+1][B]
  ACC* rw = rx + (size_t)(D + 1) * B;                // [P][B]
  ACC* ts = rw + (size_t)P * B;                      // ORDER 2: [D+1][B]
  ACC* rg = ts + (ORDER == 2 ? (size_t)(D + 1) * B : 0);  // [Do][B]
  int* ent_l = reinterpret_cast<int*>(
      rg + (ORDER == 2 ? (size_t)Do * B : 0));
  float* coef_l = reinterpret_cast<float*>(ent_l + K);
  for (int k = tid; k < K; k += B) {
    ent_l[k] = ent[k];
    coef_l[k] = coef[k];
  }
  const bool chan = c < C;
  for (int p = 0; p < P; ++p) {
    ws[p * B + tid] =
        chan ? (ACC)W[((long)e * P + p) * C + c] : (ACC)0;
    rw[p * B + tid] = (ACC)0;
  }
  __syncthreads();

  for (long chunk = z; chunk < nchunks; chunk += Z) {
    const long row = chunk * R + r;
    if (!chan || row >= cnt) continue;
    const long n = perm[start + row];
    if (n < 0 || n >= N) continue;
    const long base = n * C + c;
    const T* xp = x + base * D;
    for (int d = 0; d < D; ++d) {
      xs[d * B + tid] = (ACC)xp[d];
      rx[d * B + tid] = (ACC)0;
    }
    xs[D * B + tid] = (ACC)1;
    rx[D * B + tid] = (ACC)0;
    const T* gp = g + base * Do;
    for (int o = 0; o < Do; ++o) gs[o * B + tid] = (ACC)gp[o];
    if (ORDER == 2) {
      const T* tp = t + base * D;
      for (int d = 0; d < D; ++d) ts[d * B + tid] = (ACC)tp[d];
      ts[D * B + tid] = (ACC)0;
      for (int o = 0; o < Do; ++o) rg[o * B + tid] = (ACC)0;
    }
    for (int k = 0; k < K; ++k) {
      const Ent q = unpack(ent_l[k]);
      const ACC cf = (ACC)coef_l[k];
      const ACC xi = xs[q.i * B + tid], xj = xs[q.j * B + tid],
                xl = xs[q.l * B + tid];
      const ACC w = ws[q.p * B + tid];
      const ACC cg = cf * gs[q.o * B + tid];
      const ACC cgw = cg * w;
      if (ORDER == 1) {
        rx[q.i * B + tid] += cgw * xj * xl;
        rx[q.j * B + tid] += cgw * xi * xl;
        rx[q.l * B + tid] += cgw * xi * xj;
        rw[q.p * B + tid] += cg * xi * xj * xl;
      } else {
        const ACC ti = ts[q.i * B + tid], tj = ts[q.j * B + tid],
                  tl = ts[q.l * B + tid];
        const ACC t1 = ti * xj * xl + xi * tj * xl + xi * xj * tl;
        rg[q.o * B + tid] += cf * w * t1;
        rw[q.p * B + tid] += cg * t1;
        rx[q.i * B + tid] += cgw * (tj * xl + xj * tl);
        rx[q.j * B + tid] += cgw * (ti * xl + xi * tl);
        rx[q.l * B + tid] += cgw * (ti * xj + xi * tj);
      }
    }
    if (ox) {
      T* p = ox + base * D;
      for (int d = 0; d < D; ++d) p[d] = (T)rx[d * B + tid];
    }
    if (ORDER == 2 && og) {
      T* p = og + base * Do;
      for (int o = 0; o < Do; ++o) p[o] = (T)rg[o * B + tid];
    }
  }

  if (partial) {
    __syncthreads();
    if (r == 0 && chan) {
      ACC* pp = partial + (((long)e * Z + z) * P) * C + c;
      for (int p = 0; p < P; ++p) {
        ACC s = 0;
        for (int rr = 0; rr < R; ++rr) s += rw[p * B + rr * CT + cl];
        pp[(long)p * C] = s;
      }
    }
  }
}

// gW[e, p, c] = sum over the partials that exist for e.  Grid (tiles of
// WS_PC weights, nel); a block is WS_PC weights x WS_Z lanes.  Lane zl
// adds the partials zl, zl + WS_Z, .. in order, then the lanes are
// added in order: a fixed association, but WS_Z loads in flight per
// weight where one thread walking all Z partials has a single one.
constexpr int WS_PC = 16, WS_Z = 16;
template <typename T>
__global__ __launch_bounds__(WS_PC * WS_Z) void symcon_wsum_kernel(
    const typename sc_acc<T>::type* __restrict__ partial,
    const long* __restrict__ rowptr, T* __restrict__ gW, long N, int PC,
    int Z, int R) {
  using ACC = typename sc_acc<T>::type;
  __shared__ ACC lanes[WS_PC * WS_Z];
  const int pl = threadIdx.x % WS_PC, zl = threadIdx.x / WS_PC;
  const long e = blockIdx.y;
  const int pc = blockIdx.x * WS_PC + pl;
  long start = rowptr[e], cnt = rowptr[e + 1] - start;
  if (start < 0 || cnt < 0 || start + cnt > N) cnt = 0;
  long nz = (cnt + R - 1) / R;
  if (nz > Z) nz = Z;
  ACC s = 0;
  if (pc < PC)
    for (long zz = zl; zz < nz; zz += WS_Z)
      s += partial[(e * Z + zz) * PC + pc];
  lanes[threadIdx.x] = s;
  __syncthreads();
  if (zl == 0 && pc < PC) {
    ACC t = 0;
    for (int k = 0; k < WS_Z; ++k) t += lanes[k * WS_PC + pl];
    gW[e * PC + pc] = (T)t;
  }
}

struct GradGeom {
  int block, ct_log2, R, Z, ctiles;
  size_t lds;
};

size_t grad_lds(int D, int Do, int P, int K, int order, int block,
                size_t acc) {
  size_t words = 2 * (size_t)(D + 1) + Do + 2 * (size_t)P;
  if (order == 2) words += (size_t)(D + 1) + Do;
  return words * block * acc + (size_t)K * 8;
}

GradGeom grad_geom(long N, int C, int D, int Do, int P, int K, int order,
                   int nel, bool dbl) {
  GradGeom G;
  G.block = dbl ? 128 : 256;
  G.ct_log2 = 3;
  while ((1 << G.ct_log2) < C && G.ct_log2 < 6) ++G.ct_log2;
  G.R = G.block >> G.ct_log2;
  G.ctiles = (C + (1 << G.ct_log2) - 1) >> G.ct_log2;
  // enough workgroups per element to fill the device when one element
  // holds every row; bounded by the size of the partial buffer
  long z = (N + (long)G.R * 8 - 1) / ((long)G.R * 8);
  long cap = SC_PARTIAL_BYTES /
             ((long)nel * P * C * (dbl ? 8 : 4) > 0
                  ? (long)nel * P * C * (dbl ? 8 : 4) : 1);
  if (z > cap) z = cap;
  if (z > 512) z = 512;
  if (z < 1) z = 1;
  G.Z = (int)z;
  G.lds = grad_lds(D, Do, P, K, order, G.block, dbl ? 8 : 4);
  return G;
}

void check_common(const torch::Tensor& x, const torch::Tensor& W,
                  const torch::Tensor& ent, const torch::Tensor& coef,
                  long Do) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous(),
              "symcon: x must be a contiguous [N, C, D] device tensor");
  TORCH_CHECK(W.is_cuda() && W.dim() == 3 && W.is_contiguous() &&
                  W.scalar_type() == x.scalar_type() &&
                  W.size(2) == x.size(1),
              "symcon: W must be contiguous [nel, P, C] of x's dtype");
  TORCH_CHECK(x.size(2) >= 1 && x.size(2) <= SC_MAX_D && Do >= 1 &&
                  Do <= SC_MAX_D && W.size(1) >= 1 &&
                  W.size(1) <= SC_MAX_P && W.size(0) >= 1,
              "symcon: outside the kernel envelope");
  TORCH_CHECK(ent.is_cuda() && coef.is_cuda() && ent.is_contiguous() &&
                  coef.is_contiguous() &&
                  ent.scalar_type() == at::ScalarType::Int &&
                  coef.scalar_type() == at::ScalarType::Float &&
                  ent.dim() == 1 && ent.sizes() == coef.sizes() &&
                  ent.size(0) <= SC_MAX_ENT,
              "symcon: bad entry table");
  TORCH_CHECK(x.scalar_type() == at::ScalarType::Float ||
                  x.scalar_type() == at::ScalarType::Double ||
                  x.scalar_type() == at::ScalarType::BFloat16,
              "symcon: fp32, bf16 or fp64");
}

void check_index(const torch::Tensor& t, long len, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 1 &&
                  t.scalar_type() == at::ScalarType::Long &&
                  t.size(0) == len,
              "symcon: ", what, " must be a contiguous int64 vector of ",
              len);
}

hipStream_t sc_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

}  // namespace

// Dynamic-LDS bytes of a launch; ops/symcon.py asks before it chooses
// the kernels.  order 0 is the forward.
long symcon_lds_bytes(long D, long Do, long P, long K, long order,
                      long acc_bytes) {
  if (order == 0)
    return (long)(((size_t)(D + 1) + P + Do) * 256 * acc_bytes +
                  (size_t)K * 8);
  return (long)grad_lds((int)D, (int)Do, (int)P, (int)K, (int)order,
                        acc_bytes == 8 ? 128 : 256, (size_t)acc_bytes);
}

// The packed entry words come from ops/symcon.py, which checks every
// index against its dimension when it builds the table.
torch::Tensor symcon_forward(torch::Tensor x, torch::Tensor elem,
                             torch::Tensor W, torch::Tensor ent,
                             torch::Tensor coef, long Do) {
  check_common(x, W, ent, coef, Do);
  const long N = x.size(0);
  const int C = x.size(1), D = x.size(2), P = W.size(1),
            nel = W.size(0), K = ent.size(0);
  check_index(elem, N, "elem");
  auto out = torch::empty({N, (long)C, Do}, x.options());
  const long NC = N * C;
  if (NC == 0) return out;
  const bool dbl = x.scalar_type() == at::ScalarType::Double;
  const int block = 256;
  const size_t lds =
      (size_t)symcon_lds_bytes(D, Do, P, K, 0, dbl ? 8 : 4);
  TORCH_CHECK(lds <= SC_LDS_BUDGET, "symcon_forward: LDS budget");
  const long blocks = (NC + block - 1) / block;
  AT_DISPATCH_FLOATING_TYPES_AND(
      at::ScalarType::BFloat16, x.scalar_type(), "symcon_forward", [&] {
        hipLaunchKernelGGL(
            symcon_fwd_kernel<scalar_t>, dim3(blocks), dim3(block), lds,
            sc_stream(), x.data_ptr<scalar_t>(), elem.data_ptr<long>(),
            W.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
            ent.data_ptr<int>(), coef.data_ptr<float>(), K, N, C, D,
            (int)Do, P, nel);
      });
  check_launch("symcon_forward");
  return out;
}

// order 1: t absent.  Returns {ox, oW}           (dQ/dx, dQ/dW)
// order 2: t given.   Returns {ox, oW, og}       (dR/dx, dR/dW, dR/dg)
// Outputs outside the mask (bit 0 x, bit 1 W, bit 2 g) come back
// undefined (None in Python).
std::vector<torch::Tensor> symcon_grad(
    torch::Tensor x, torch::Tensor g, c10::optional<torch::Tensor> t,
    torch::Tensor W, torch::Tensor perm, torch::Tensor rowptr,
    torch::Tensor ent, torch::Tensor coef, long mask) {
  const long Do = g.dim() == 3 ? g.size(2) : 0;
  check_common(x, W, ent, coef, Do);
  const int order = t.has_value() ? 2 : 1;
  TORCH_CHECK(mask > 0 && mask < (order == 2 ? 8 : 4),
              "symcon_grad: bad output mask");
  const long N = x.size(0);
  const int C = x.size(1), D = x.size(2), P = W.size(1),
            nel = W.size(0), K = ent.size(0);
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() &&
                  g.scalar_type() == x.scalar_type() && g.size(0) == N &&
                  g.size(1) == C,
              "symcon_grad: g must be contiguous [N, C, Do]");
  if (order == 2)
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == x.scalar_type() &&
                    t->sizes() == x.sizes(),
                "symcon_grad: t must match x");
  check_index(perm, N, "perm");
  check_index(rowptr, nel + 1, "rowptr");
  TORCH_CHECK(nel <= 65535, "symcon_grad: too many elements");
  const bool dbl = x.scalar_type() == at::ScalarType::Double;
  const GradGeom G = grad_geom(N, C, D, (int)Do, P, K, order, nel, dbl);
  TORCH_CHECK(G.lds <= SC_LDS_BUDGET, "symcon_grad: LDS budget");

  std::vector<torch::Tensor> outs(order == 2 ? 3 : 2);
  if (mask & 1) outs[0] = torch::empty_like(x);
  if (mask & 2) outs[1] = torch::empty_like(W);
  if (order == 2 && (mask & 4)) outs[2] = torch::empty_like(g);
  torch::Tensor partial;
  if (mask & 2)
    partial = torch::empty(
        {(long)nel, (long)G.Z, (long)P, (long)C},
        x.options().dtype(dbl ? torch::kDouble : torch::kFloat));
  AT_DISPATCH_FLOATING_TYPES_AND(
      at::ScalarType::BFloat16, x.scalar_type(), "symcon_grad", [&] {
        using ACC = typename sc_acc<scalar_t>::type;
        auto ptr = [](torch::Tensor& o) -> scalar_t* {
          return o.defined() ? o.data_ptr<scalar_t>() : nullptr;
        };
        if (N * C > 0) {
          auto kern = order == 1 ? symcon_grad_kernel<scalar_t, 1>
                                 : symcon_grad_kernel<scalar_t, 2>;
          hipLaunchKernelGGL(
              kern, dim3(G.Z, nel, G.ctiles), dim3(G.block), G.lds,
              sc_stream(), x.data_ptr<scalar_t>(),
              g.data_ptr<scalar_t>(),
              order == 2 ? t->data_ptr<scalar_t>() : nullptr,
              W.data_ptr<scalar_t>(), perm.data_ptr<long>(),
              rowptr.data_ptr<long>(), ptr(outs[0]),
              order == 2 ? ptr(outs[2]) : nullptr,
              partial.defined() ? partial.data_ptr<ACC>() : nullptr,
              ent.data_ptr<int>(), coef.data_ptr<float>(), K, N, C, D,
              (int)Do, P, G.ct_log2);
          check_launch("symcon_grad");
        }
        if (mask & 2) {
          // with no rows every element has zero partials to add
          const int PC = P * C;
          if (PC > 0) hipLaunchKernelGGL(
              symcon_wsum_kernel<scalar_t>,
              dim3((PC + WS_PC - 1) / WS_PC, nel), dim3(WS_PC * WS_Z), 0,
              sc_stream(), partial.data_ptr<ACC>(),
              rowptr.data_ptr<long>(), outs[1].data_ptr<scalar_t>(), N,
              PC, G.Z, G.R);
          check_launch("symcon_wsum");
        }
      });
  return outs;
}

// {block, channel tile, row lanes, Z, channel tiles}: how symcon_grad
// would lay out a launch (tests use it to build multi-chunk cases).
std::vector<long> symcon_grad_geometry(long N, long C, long D, long Do,
                                       long P, long K, long order,
                                       long nel, bool dbl) {
  const GradGeom G = grad_geom(N, (int)C, (int)D, (int)Do, (int)P, (int)K,
                               (int)order, (int)nel, dbl);
  return {G.block, 1L << G.ct_log2, G.R, G.Z, G.ctiles};
}
