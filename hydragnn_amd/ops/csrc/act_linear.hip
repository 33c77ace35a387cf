// Fused SiLU -> Linear family for the per-edge radial MLP (gfx950), closed
// under the two differentiations of force training.
//
// The unit is activation first: y = silu(h) W^T + b with h [E, K] the
// pre-activation, W [N, K], b [N].  With phi(x) = x s(x), s the logistic
// function, phi' = s (1 + x (1 - s)) and phi'' = s (1 - s)(2 + x (1 - 2 s)),
// all evaluated in fp32 from the bf16 value of h:
//
//   act_linear_fwd      y[e,n]  = sum_k bf16(phi(h[e,k])) W[n,k] + b[n]
//   act_linear_dgrad    gh[e,k] = (sum_n g[e,n] W[n,k]) phi'(h[e,k])
//   act_linear_dgrad_dg dg[e,n] = sum_k bf16(u[e,k] phi'(h[e,k])) W[n,k]
//   act_linear_dgrad_dh dh[e,k] = u[e,k] (sum_n g[e,n] W[n,k]) phi''(h[e,k])
//   act_linear_wgrad    gW[n,k] = sum_e g[e,n] p[e,k],  gb[n] = sum_e g[e,n]
//                       p = x | bf16(phi(x)) | bf16(u phi'(x))
//
// Sums run in fp32 and every result is rounded to bf16 once.  The four
// [E, .] GEMMs are one template derived from mfma_linear_kernel (128 x 64
// tile, v_mfma_f32_16x16x32_bf16): a prologue on the A tile as it is staged
// into LDS and an epilogue on the fp32 accumulators.  The activated tensor
// is never written to memory.  The MFMA runs transposed (W fragment as the
// A operand), so a lane ends up with four consecutive output columns and
// the epilogue reads h and u and writes the result 8 bytes at a time.
//
// The weight gradient contracts over E straight from the row-major [E, .]
// operands: E is cut into a number of chunks that depends on E alone, one
// block per (chunk, 64-wide k tile) transposes its 64-row stages into LDS,
// accumulates the [N, 64] tile on MFMA and writes one fp32 partial; a
// second kernel adds the partials in a fixed two-level order (ascending
// chunks within eight consecutive ranges, then the ranges in order) and
// rounds once.  No atomics, no padded copies: the E tail is masked at staging.
// The bias gradient is the row sum of the transposed g tile in LDS.
//
// Envelope: N % 64 == 0, K % 64 == 0, 64 <= K <= 256, 64 <= N <= 320 (the
// flagship's second interaction has five tensor-product paths of 64
// channels), E >= 256 (E == 0 returns zeros / an empty result).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "check_launch.h"

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BM = 128;   // rows of E per GEMM block
constexpr int BN = 64;    // output columns per GEMM block
constexpr int BK = 64;    // contraction depth per stage
// LDS rows of 64 bf16 = 128 B + 16 B pad: 16-byte aligned, and the 16
// rows of a fragment read land on 16 distinct 4-bank groups
constexpr int LP = 72;

constexpr int PRO_NONE = 0, PRO_PHI = 1, PRO_UDPHI = 2;
constexpr int EPI_BIAS = 0, EPI_DPHI = 1, EPI_UD2PHI = 2;

__device__ __forceinline__ float sigm(float x) {
  return 1.f / (1.f + expf(-x));
}
__device__ __forceinline__ float phi(float x) { return x * sigm(x); }
__device__ __forceinline__ float dphi(float x) {
  float s = sigm(x);
  return s * (1.f + x * (1.f - s));
}
__device__ __forceinline__ float d2phi(float x) {
  float s = sigm(x);
  return s * (1.f - s) * (2.f + x * (1.f - 2.f * s));
}

// p = x | bf16(phi(x)) | bf16(u phi'(x)), eight elements
template <int PRO>
__device__ __forceinline__ bf16x8 prologue(bf16x8 a, bf16x8 h) {
  if (PRO == PRO_NONE) return a;
  bf16x8 r;
  for (int t = 0; t < 8; ++t) {
    if (PRO == PRO_PHI)
      r[t] = (__bf16)phi((float)a[t]);
    else
      r[t] = (__bf16)((float)a[t] * dphi((float)h[t]));
  }
  return r;
}

// C[M, N] = epi(pro(A)[M, K] @ B), B = W[N, K] (TRANS_B) or W[K, N]
template <int PRO, int EPI, bool TRANS_B>
__global__ __launch_bounds__(256) void act_gemm_kernel(
    const __bf16* __restrict__ A,     // [M, K]
    const __bf16* __restrict__ AH,    // [M, K] h of the PRO_UDPHI prologue
    const __bf16* __restrict__ B,     // [N, K] or [K, N]
    const __bf16* __restrict__ bias,  // [N] or nullptr (EPI_BIAS)
    const __bf16* __restrict__ EH,    // [M, N] h of the dgrad epilogues
    const __bf16* __restrict__ EU,    // [M, N] u of EPI_UD2PHI
    __bf16* __restrict__ C,           // [M, N]
    long M, int N, int K) {
  __shared__ __attribute__((aligned(16))) __bf16 lA[BM * LP];  // [row][k]
  __shared__ __attribute__((aligned(16))) __bf16 lB[BN * LP];  // [col][k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;
  // the n tiles of one row block are neighbours in the grid, so the A
  // tile they share is read from memory once
  const int ntiles = N / BN;
  const long m0 = (long)(blockIdx.x / ntiles) * BM;
  const int n0 = (int)(blockIdx.x % ntiles) * BN;

  f32x4 acc[4][2];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 2; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += BK) {
    // A tile [BM, BK]: 1024 chunks of 8, four per thread
    for (int p = 0; p < 4; ++p) {
      int idx = p * 256 + tid;
      int row = idx >> 3;
      int col8 = (idx & 7) * 8;
      long gm = m0 + row;
      bf16x8 v;
      for (int t = 0; t < 8; ++t) v[t] = (__bf16)0.f;
      if (gm < M) {
        long off = gm * K + k0 + col8;
        bf16x8 a = *reinterpret_cast<const bf16x8*>(A + off);
        bf16x8 h = a;
        if (PRO == PRO_UDPHI)
          h = *reinterpret_cast<const bf16x8*>(AH + off);
        v = prologue<PRO>(a, h);
      }
      *reinterpret_cast<bf16x8*>(&lA[row * LP + col8]) = v;
    }
    // B tile as [col][k]
    if (TRANS_B) {
      for (int p = 0; p < 2; ++p) {
        int idx = p * 256 + tid;
        int col = idx >> 3;
        int k8 = (idx & 7) * 8;
        *reinterpret_cast<bf16x8*>(&lB[col * LP + k8]) =
            *reinterpret_cast<const bf16x8*>(
                B + (long)(n0 + col) * K + k0 + k8);
      }
    } else {
      // W[K, N]: lanes run along a row of W, each gathers 16 k
      int col = tid & 63;
      int kq = (tid >> 6) * 16;
      for (int half = 0; half < 2; ++half) {
        bf16x8 v;
        for (int t = 0; t < 8; ++t)
          v[t] = B[(long)(k0 + kq + half * 8 + t) * N + n0 + col];
        *reinterpret_cast<bf16x8*>(&lB[col * LP + kq + half * 8]) = v;
      }
    }
    __syncthreads();

    // fragment of either operand: lane l holds [row l&15][k 8(l>>4)+q].
    // W is the MFMA's A operand, so D[row = n][col = e].
    for (int s = 0; s < BK / 32; ++s) {
      const int kk = s * 32 + (lane >> 4) * 8;
      bf16x8 wf[2];
      for (int j = 0; j < 2; ++j)
        wf[j] = *reinterpret_cast<const bf16x8*>(
            &lB[(wc * 32 + j * 16 + (lane & 15)) * LP + kk]);
      for (int i = 0; i < 4; ++i) {
        bf16x8 af = *reinterpret_cast<const bf16x8*>(
            &lA[(wr * 64 + i * 16 + (lane & 15)) * LP + kk]);
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              wf[j], af, acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // D layout: col = lane&15 -> row of E, row = (lane>>4)*4 + reg -> four
  // consecutive output columns
  for (int i = 0; i < 4; ++i) {
    long e = m0 + wr * 64 + i * 16 + (lane & 15);
    if (e >= M) continue;
    for (int j = 0; j < 2; ++j) {
      int n = n0 + wc * 32 + j * 16 + (lane >> 4) * 4;
      long off = e * N + n;
      f32x4 a = acc[i][j];
      if (EPI == EPI_BIAS) {
        if (bias != nullptr) {
          bf16x4 bv = *reinterpret_cast<const bf16x4*>(bias + n);
          for (int r = 0; r < 4; ++r) a[r] += (float)bv[r];
        }
      } else {
        bf16x4 hv = *reinterpret_cast<const bf16x4*>(EH + off);
        if (EPI == EPI_DPHI) {
          for (int r = 0; r < 4; ++r) a[r] *= dphi((float)hv[r]);
        } else {
          bf16x4 uv = *reinterpret_cast<const bf16x4*>(EU + off);
          for (int r = 0; r < 4; ++r)
            a[r] *= (float)uv[r] * d2phi((float)hv[r]);
        }
      }
      bf16x4 o;
      for (int r = 0; r < 4; ++r) o[r] = (__bf16)a[r];
      *reinterpret_cast<bf16x4*>(C + off) = o;
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
constexpr int BE = 64;          // rows of E per stage
constexpr int WG_MIN_ROWS = 256;
constexpr int WG_MAX_CHUNKS = 512;

struct WgradSplit {
  long chunks, rows;
};

// the split of E into chunks: a function of E alone
WgradSplit wgrad_split(long E) {
  long c = (E + WG_MIN_ROWS - 1) / WG_MIN_ROWS;
  if (c > WG_MAX_CHUNKS) c = WG_MAX_CHUNKS;
  if (c < 1) c = 1;
  long rows = (E + c - 1) / c;
  rows = (rows + BE - 1) / BE * BE;
  if (rows < BE) rows = BE;
  c = (E + rows - 1) / rows;
  if (c < 1) c = 1;
  return {c, rows};
}

__device__ __forceinline__ unsigned pack2(__bf16 lo, __bf16 hi) {
  return (unsigned)__builtin_bit_cast(unsigned short, lo) |
         ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
}

// rows (2 ep, 2 ep + 1) x 8 columns -> transposed LDS image [col][e]
__device__ __forceinline__ void store_pair_t(__bf16* dst, int col0, int ep,
                                             bf16x8 v0, bf16x8 v1) {
  for (int t = 0; t < 8; ++t)
    *reinterpret_cast<unsigned*>(&dst[(col0 + t) * LP + 2 * ep]) =
        pack2(v0[t], v1[t]);
}

// partW[chunk, n, k] = sum over the chunk's rows of g[e, n] p[e, k];
// partB[chunk, n] = sum of g[e, n] (k tile 0 only).  N = NT * 64.
template <int NT, int PRO>
__global__ __launch_bounds__(256) void act_wgrad_kernel(
    const __bf16* __restrict__ G,   // [E, N]
    const __bf16* __restrict__ X,   // [E, K]
    const __bf16* __restrict__ U,   // [E, K] (PRO_UDPHI)
    float* __restrict__ partW,      // [chunks, N, K]
    float* __restrict__ partB,      // [chunks, N] or nullptr
    long E, int K, long rows) {
  constexpr int N = NT * 64;
  __shared__ __attribute__((aligned(16))) __bf16 lG[N * LP];    // [n][e]
  __shared__ __attribute__((aligned(16))) __bf16 lP[64 * LP];   // [k][e]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long chunk = blockIdx.x;
  const int k0 = blockIdx.y * 64;
  const long e_begin = chunk * rows;
  long e_end = e_begin + rows;
  if (e_end > E) e_end = E;

  f32x4 acc[NT][4];
  for (int i = 0; i < NT; ++i)
    for (int j = 0; j < 4; ++j)
      acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  float bsum[2] = {0.f, 0.f};   // rows tid and tid + 256 of g^T
  const bool do_bias = partB != nullptr && blockIdx.y == 0;

  // staging units: a pair of rows x 8 columns.  g has 32 x N/8 = NT*256
  // of them, the k tile of x has 256.
  bf16x8 gv[NT][2], xv[2], uv[2];
  auto load = [&](long e0) {
    bf16x8 z;
    for (int t = 0; t < 8; ++t) z[t] = (__bf16)0.f;
    for (int it = 0; it < NT; ++it) {
      int u = it * 256 + tid;
      int ep = u & 15 | ((u >> 4) / (N / 8)) << 4;   // 0..31
      int c8 = ((u >> 4) % (N / 8)) * 8;
      for (int r = 0; r < 2; ++r) {
        long e = e0 + 2 * ep + r;
        gv[it][r] = e < e_end
            ? *reinterpret_cast<const bf16x8*>(G + e * N + c8) : z;
      }
    }
    {
      int ep = tid & 15 | (tid >> 7) << 4;
      int c8 = ((tid >> 4) & 7) * 8;
      for (int r = 0; r < 2; ++r) {
        long e = e0 + 2 * ep + r;
        bool ok = e < e_end;
        xv[r] = ok ? *reinterpret_cast<const bf16x8*>(X + e * K + k0 + c8)
                   : z;
        if (PRO == PRO_UDPHI)
          uv[r] = ok ? *reinterpret_cast<const bf16x8*>(U + e * K + k0 + c8)
                     : z;
      }
    }
  };
  auto store = [&]() {
    for (int it = 0; it < NT; ++it) {
      int u = it * 256 + tid;
      int ep = u & 15 | ((u >> 4) / (N / 8)) << 4;
      int c8 = ((u >> 4) % (N / 8)) * 8;
      store_pair_t(lG, c8, ep, gv[it][0], gv[it][1]);
    }
    {
      int ep = tid & 15 | (tid >> 7) << 4;
      int c8 = ((tid >> 4) & 7) * 8;
      // masked rows hold x = u = 0: phi(0) = 0 and 0 * phi'(0) = 0
      bf16x8 p0 = PRO == PRO_UDPHI ? prologue<PRO>(uv[0], xv[0])
                                   : prologue<PRO>(xv[0], xv[0]);
      bf16x8 p1 = PRO == PRO_UDPHI ? prologue<PRO>(uv[1], xv[1])
                                   : prologue<PRO>(xv[1], xv[1]);
      store_pair_t(lP, c8, ep, p0, p1);
    }
  };

  if (e_begin < e_end) load(e_begin);
  for (long e0 = e_begin; e0 < e_end; e0 += BE) {
    __syncthreads();           // the previous stage's reads are done
    store();
    __syncthreads();
    if (e0 + BE < e_end) load(e0 + BE);   // in flight under the MFMAs

    // wave w owns rows n in [w*NT*16, (w+1)*NT*16) x the 64 k columns
    for (int s = 0; s < BE / 32; ++s) {
      const int ee = s * 32 + (lane >> 4) * 8;
      bf16x8 pf[4];
      for (int j = 0; j < 4; ++j)
        pf[j] = *reinterpret_cast<const bf16x8*>(
            &lP[(j * 16 + (lane & 15)) * LP + ee]);
      for (int i = 0; i < NT; ++i) {
        bf16x8 gf = *reinterpret_cast<const bf16x8*>(
            &lG[((wave * NT + i) * 16 + (lane & 15)) * LP + ee]);
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              gf, pf[j], acc[i][j], 0, 0, 0);
      }
    }
    if (do_bias) {
      for (int q = 0; q < 2; ++q) {
        int n = tid + q * 256;
        if (n >= N) break;
        for (int c = 0; c < BE / 8; ++c) {
          bf16x8 v = *reinterpret_cast<const bf16x8*>(&lG[n * LP + c * 8]);
          for (int t = 0; t < 8; ++t) bsum[q] += (float)v[t];
        }
      }
    }
  }

  // D layout: col = lane&15 -> k, row = (lane>>4)*4 + reg -> n
  for (int i = 0; i < NT; ++i)
    for (int j = 0; j < 4; ++j)
      for (int r = 0; r < 4; ++r) {
        int n = (wave * NT + i) * 16 + (lane >> 4) * 4 + r;
        int k = k0 + j * 16 + (lane & 15);
        partW[(chunk * N + n) * K + k] = acc[i][j][r];
      }
  if (do_bias)
    for (int q = 0; q < 2; ++q)
      if (tid + q * 256 < N) partB[chunk * N + tid + q * 256] = bsum[q];
}

// out = bf16(sum of the partials), in a fixed order of two levels: the
// chunks are cut into RG consecutive ranges (a function of the chunk count
// alone), a range is added in ascending chunk order, the RG range sums in
// ascending range order.  A block owns 32 consecutive outputs; thread
// (range, output) = (tid >> 5, tid & 31).  The first nk outputs are the
// weight gradient, the next n the bias gradient.
constexpr int RG = 8;

__global__ __launch_bounds__(32 * RG) void act_wgrad_reduce_kernel(
    const float* __restrict__ partW, const float* __restrict__ partB,
    __bf16* __restrict__ gW, __bf16* __restrict__ gb, long chunks, int nk,
    int n) {
  __shared__ float part[RG][32];
  const int o = threadIdx.x & 31;
  const int r = threadIdx.x >> 5;
  const int idx = blockIdx.x * 32 + o;
  const float* src = nullptr;
  __bf16* dst = nullptr;
  int stride = 0;
  if (idx < nk) {
    src = partW + idx; dst = gW + idx; stride = nk;
  } else if (partB != nullptr && idx < nk + n) {
    src = partB + (idx - nk); dst = gb + (idx - nk); stride = n;
  }
  const long per = (chunks + RG - 1) / RG;
  long c = r * per;
  long c_end = c + per < chunks ? c + per : chunks;
  float s = 0.f;
  if (src != nullptr) {
    for (; c + 4 <= c_end; c += 4) {
      float v[4];
      for (int t = 0; t < 4; ++t) v[t] = src[(c + t) * stride];
      for (int t = 0; t < 4; ++t) s += v[t];
    }
    for (; c < c_end; ++c) s += src[c * stride];
  }
  part[r][o] = s;
  __syncthreads();
  if (r == 0 && dst != nullptr) {
    float t = part[0][o];
    for (int q = 1; q < RG; ++q) t += part[q][o];
    *dst = (__bf16)t;
  }
}

const __bf16* bptr(const torch::Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr());
}

void check_operand(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::ScalarType::BFloat16,
              "act_linear: ", name, " must be a contiguous bf16 device tensor");
}

// the one statement of the envelope on this side (ops/act_linear.py has
// the other)
void check_envelope(long E, long N, long K) {
  TORCH_CHECK(N % 64 == 0 && K % 64 == 0 && N >= 64 && K >= 64 &&
              N <= 320 && K <= 256 && (E == 0 || E >= 256),
              "act_linear envelope: N in [64, 320] and K in [64, 256], "
              "multiples of 64, and E >= 256; got E=", E, " N=", N, " K=", K);
}

template <int PRO, int EPI, bool TRANS_B>
torch::Tensor launch_gemm(const torch::Tensor& A, const __bf16* AH,
                          const torch::Tensor& W, const __bf16* bias,
                          const __bf16* EH, const __bf16* EU, long n_out,
                          const char* what) {
  long M = A.size(0);
  int K = A.size(1);
  auto C = torch::empty({M, n_out}, A.options());
  if (M == 0) return C;
  long blocks = (M + BM - 1) / BM * (n_out / BN);
  TORCH_CHECK(blocks < (1L << 31), what, ": too many rows");
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL((act_gemm_kernel<PRO, EPI, TRANS_B>),
                     dim3((unsigned)blocks), dim3(256), 0, stream, bptr(A),
                     AH, bptr(W), bias, EH, EU,
                     reinterpret_cast<__bf16*>(C.data_ptr()), M, (int)n_out,
                     K);
  check_launch(what);
  return C;
}

}  // namespace

torch::Tensor act_linear_fwd(torch::Tensor h, torch::Tensor W,
                             c10::optional<torch::Tensor> bias) {
  check_operand(h, "h");
  check_operand(W, "W");
  TORCH_CHECK(h.dim() == 2 && W.dim() == 2 && h.size(1) == W.size(1),
              "act_linear: h [E, K] and W [N, K]");
  check_envelope(h.size(0), W.size(0), W.size(1));
  const __bf16* bp = nullptr;
  if (bias.has_value()) {
    check_operand(*bias, "bias");
    TORCH_CHECK(bias->dim() == 1 && bias->size(0) == W.size(0),
                "act_linear: bias [N]");
    bp = bptr(*bias);
  }
  return launch_gemm<PRO_PHI, EPI_BIAS, true>(
      h, nullptr, W, bp, nullptr, nullptr, W.size(0), "act_linear");
}

torch::Tensor act_linear_dgrad(torch::Tensor g, torch::Tensor W,
                               torch::Tensor h) {
  check_operand(g, "g");
  check_operand(W, "W");
  check_operand(h, "h");
  TORCH_CHECK(g.dim() == 2 && W.dim() == 2 && h.dim() == 2 &&
              g.size(1) == W.size(0) && h.size(1) == W.size(1) &&
              g.size(0) == h.size(0),
              "act_linear_dgrad: g [E, N], W [N, K], h [E, K]");
  check_envelope(h.size(0), W.size(0), W.size(1));
  return launch_gemm<PRO_NONE, EPI_DPHI, false>(
      g, nullptr, W, nullptr, bptr(h), nullptr, W.size(1),
      "act_linear_dgrad");
}

torch::Tensor act_linear_dgrad_dg(torch::Tensor u, torch::Tensor W,
                                  torch::Tensor h) {
  check_operand(u, "u");
  check_operand(W, "W");
  check_operand(h, "h");
  TORCH_CHECK(u.dim() == 2 && W.dim() == 2 && u.sizes() == h.sizes() &&
              h.size(1) == W.size(1),
              "act_linear_dgrad_dg: u, h [E, K] and W [N, K]");
  check_envelope(h.size(0), W.size(0), W.size(1));
  return launch_gemm<PRO_UDPHI, EPI_BIAS, true>(
      u, bptr(h), W, nullptr, nullptr, nullptr, W.size(0),
      "act_linear_dgrad_dg");
}

torch::Tensor act_linear_dgrad_dh(torch::Tensor u, torch::Tensor g,
                                  torch::Tensor W, torch::Tensor h) {
  check_operand(u, "u");
  check_operand(g, "g");
  check_operand(W, "W");
  check_operand(h, "h");
  TORCH_CHECK(g.dim() == 2 && W.dim() == 2 && u.sizes() == h.sizes() &&
              h.dim() == 2 && g.size(1) == W.size(0) &&
              h.size(1) == W.size(1) && g.size(0) == h.size(0),
              "act_linear_dgrad_dh: u, h [E, K], g [E, N], W [N, K]");
  check_envelope(h.size(0), W.size(0), W.size(1));
  return launch_gemm<PRO_NONE, EPI_UD2PHI, false>(
      g, nullptr, W, nullptr, bptr(h), bptr(u), W.size(1),
      "act_linear_dgrad_dh");
}

long act_linear_wgrad_chunks(long E) { return wgrad_split(E).chunks; }

// -> (gW [N, K], gb [N] or an empty tensor).  act: false p = x, true
// p = bf16(phi(x)), or p = bf16(u phi'(x)) when u is given.
std::vector<torch::Tensor> act_linear_wgrad(
    torch::Tensor g, torch::Tensor x, c10::optional<torch::Tensor> u,
    bool act, bool want_bias) {
  check_operand(g, "g");
  check_operand(x, "x");
  TORCH_CHECK(g.dim() == 2 && x.dim() == 2 && g.size(0) == x.size(0),
              "act_linear_wgrad: g [E, N] and x [E, K]");
  long E = g.size(0), N = g.size(1), K = x.size(1);
  check_envelope(E, N, K);
  const __bf16* up = nullptr;
  if (u.has_value()) {
    TORCH_CHECK(act, "act_linear_wgrad: u goes with act = true");
    check_operand(*u, "u");
    TORCH_CHECK(u->sizes() == x.sizes(), "act_linear_wgrad: u like x");
    up = bptr(*u);
  }
  auto gW = torch::empty({N, K}, g.options());
  auto gb = torch::empty({want_bias ? N : 0}, g.options());
  if (E == 0) return {gW.zero_(), gb.zero_()};
  WgradSplit sp = wgrad_split(E);
  auto fopt = g.options().dtype(torch::kFloat);
  auto partW = torch::empty({sp.chunks, N, K}, fopt);
  auto partB = torch::empty({want_bias ? sp.chunks : 0, N}, fopt);
  float* pb = want_bias ? partB.data_ptr<float>() : nullptr;
  auto stream = at::hip::getCurrentHIPStream().stream();
  dim3 grid((unsigned)sp.chunks, (unsigned)(K / 64));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, bptr(g), bptr(x), up,
                       partW.data_ptr<float>(), pb, E, (int)K, sp.rows);
  };
  auto pick = [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if (up != nullptr) launch(act_wgrad_kernel<NT, PRO_UDPHI>);
    else if (act) launch(act_wgrad_kernel<NT, PRO_PHI>);
    else launch(act_wgrad_kernel<NT, PRO_NONE>);
  };
  switch (N / 64) {
    case 1: pick(std::integral_constant<int, 1>{}); break;
    case 2: pick(std::integral_constant<int, 2>{}); break;
    case 3: pick(std::integral_constant<int, 3>{}); break;
    case 4: pick(std::integral_constant<int, 4>{}); break;
    case 5: pick(std::integral_constant<int, 5>{}); break;
    default: TORCH_CHECK(false, "act_linear_wgrad: N / 64 = ", N / 64);
  }
  check_launch("act_linear_wgrad");
  int nk = (int)(N * K), nb = want_bias ? (int)N : 0;
  hipLaunchKernelGGL(act_wgrad_reduce_kernel, dim3((nk + nb + 31) / 32),
                     dim3(32 * RG), 0, stream, partW.data_ptr<float>(),
                     (const float*)pb,
                     reinterpret_cast<__bf16*>(gW.data_ptr()),
                     reinterpret_cast<__bf16*>(gb.data_ptr()), sp.chunks, nk,
                     (int)N);
  check_launch("act_linear_wgrad_reduce");
  return {gW, gb};
}
