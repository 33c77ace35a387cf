// Pair-affine edge layer with wide edge attributes on the matrix cores
// (gfx950, CDNA4): the three primitives of ops/edge_affine.py that carry
// D, for T in {bf16, f16}, D % 32 == 0 in [32, 128] and H % 64 == 0 in
// [64, 256].  `node` does not depend on D and stays in edge_affine.hip.
//
//   fwd   : z[e, f]   = (P[i, f] + P[j, H + f]) + r2[e] w_r[f]
//                       + sum_k ea[e, k] W_e[f, k] + b[f]
//   edge  : dea[e, k] = sum_f g[e, f] W_e[f, k],  dr2[e] = sum_f g[e, f] w_r[f]
//   param : dW_e[f, k] = sum_e ea[e, k] g[e, f],  dw_r[f] = sum_e r2[e] g[e, f],
//           db[f] = sum_e g[e, f]
//
// All three run v_mfma_f32_16x16x32 with the per-edge operand as the N
// side, so the product [E, .] is never written: fwd adds the gathered
// rows of P, r2 w_r and b to the fp32 fragments and rounds once.  A lane
// of an operand fragment holds [row l & 15][k 8 (l >> 4) + 0..7], a lane
// of the result [row 4 (l >> 4) + reg][col l & 15] (act_linear.hip).
//
// fwd and edge: persistent 256-thread blocks keep the weight panel in
// LDS ([H][D + 8] for fwd, W_e^T as [D][H + 8] for edge; the 16-byte pad
// spreads the 16 rows of a fragment read over the banks) and grid-stride
// over tiles of 64 edges, whose rows are staged into LDS with 16-byte
// loads; wave w owns the tile's edges 16 w .. 16 w + 15.  The weights
// are the M operand, and the two M tiles of a group of 32 output columns
// take their rows interleaved (row i of tile h is column 8 (i >> 2) + 4 h
// + (i & 3)), so a lane ends up with eight consecutive columns of one
// edge: the gathers of P and the stores of z and dea are 16-byte packs.
//
// param: E is cut into the chunks of the narrow kernel (a function of E
// alone); a block owns a (chunk, tile of 64 features), stages 64 edges
// at a time transposed into LDS ([f][e] and [k][e]: e is the MFMA's k
// index), the next stage's loads in flight under the MFMAs, and wave w
// accumulates features 16 w .. 16 w + 15 against the D + 16 columns
// [ea | r2 | 1 | 0 ...]: the extra fragment column yields dw_r and db.
// Partials are fp32 [chunk, 2 + D, H]; pair_affine_param_reduce
// (edge_affine.hip) adds them in chunk order and rounds once.
//
// Products of two bf16 or two f16 values are exact in fp32, every sum is
// in fp32 and rounded once; the order of a sum is the matrix unit's and
// the tiling's, fixed per (shape, kernel).  No atomics, one writer per
// output element, no load or store at or beyond row E, nothing syncs
// with the host, E = 0 launches nothing.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "segment_common.h"

// defined in edge_affine.hip
void pair_affine_param_reduce(const torch::Tensor& partial,
                              torch::Tensor& dwr, torch::Tensor& dWe,
                              torch::Tensor& db, long H, long D,
                              long n_chunks);
long pair_affine_param_chunks(long E);

namespace {

using namespace segment;

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;   // 16 bytes
using u16 = unsigned short;

constexpr int kTile = 64;    // edges of a fwd / edge tile and of a param stage
constexpr int kPad = 8;      // halves added to an LDS row
constexpr int kStageLd = kTile + kPad;   // param: LDS row of 64 edges
constexpr int kMaxD = 128, kMaxH = 256;
constexpr int kMaxKT = kMaxD / 32;       // edge: groups of 32 columns of dea
constexpr int kMaxNT = kMaxD / 16 + 1;   // param: 16-wide column tiles
constexpr size_t kLdsBudget = 150 * 1024;

// Operand fragments are read from LDS as the MFMA's own vector type and
// staging copies move as u32x4: a zero-initialised Pack selected against
// a load went through scratch memory.
template <typename T> struct Mfma;
template <> struct Mfma<c10::BFloat16> {
  using Frag = bf16x8;
  static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma<c10::Half> {
  using Frag = f16x8;
  static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

template <typename T>
__device__ __forceinline__ typename Mfma<T>::Frag frag(const u16* at) {
  return *reinterpret_cast<const typename Mfma<T>::Frag*>(at);
}

// rows [row0, row0 + rows) of a row-major [., width] array into LDS rows
// of `lw` halves, 16 bytes at a time; rows at or beyond `end` are not
// loaded and read as 0
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ src,
                                           u16* dst, long row0, int rows,
                                           long end, int width, int lw) {
  const int per_row = width / 8;
  for (int c = threadIdx.x; c < rows * per_row; c += kBlock) {
    const int row = c / per_row, col = (c - row * per_row) * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row0 + row < end)
      v = *reinterpret_cast<const u32x4*>(src + (row0 + row) * width + col);
    *reinterpret_cast<u32x4*>(dst + row * lw + col) = v;
  }
}

// the row of a weight panel that M tile `half` of a group of 32 output
// columns takes as its row i: a lane's registers of the two tiles are
// then the eight consecutive columns 8 (l >> 4) .. 8 (l >> 4) + 7
__device__ __forceinline__ int interleaved_row(int i, int half) {
  return 8 * (i >> 2) + 4 * half + (i & 3);
}

// ---------------------------------------------------------------------------
// fwd
// ---------------------------------------------------------------------------
// LDS: W_e [H][D + 8], the tile's ea [64][D + 8], its dst | src indices
// [2][64] and r2 [64] as fp32.  The loops over tiles and feature tiles
// are uniform in the block, so every thread reaches every barrier.
template <typename T>
__global__ void __launch_bounds__(kBlock) pair_affine_wide_fwd_kernel(
    const T* __restrict__ P, const T* __restrict__ r2,
    const T* __restrict__ ea, const T* __restrict__ wr,
    const T* __restrict__ We, const T* __restrict__ b,
    const long* __restrict__ didx, const long* __restrict__ sidx,
    T* __restrict__ z, long E, int H, int D) {
  using P8 = Pack<T, 8>;
  extern __shared__ __align__(16) unsigned char pair_affine_wide_lds[];
  const int lw = D + kPad;
  u16* s_w = reinterpret_cast<u16*>(pair_affine_wide_lds);
  u16* s_e = s_w + H * lw;
  long* s_i = reinterpret_cast<long*>(s_e + kTile * lw);
  float* s_r = reinterpret_cast<float*>(s_i + 2 * kTile);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, q = lane >> 4;
  const int el = 16 * wave + col;            // this lane's edge of the tile
  stage_rows<T>(We, s_w, 0, H, H, D, lw);
  const long n_tiles = (E + kTile - 1) / kTile;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long e0 = t * kTile;
    stage_rows<T>(ea, s_e, e0, kTile, E, D, lw);
    if (tid < 2 * kTile) {
      if (P) {
        const long e = e0 + (tid & (kTile - 1));
        s_i[tid] = e < E ? (tid < kTile ? didx[e] : sidx[e]) : 0;
      }
    } else if (tid < 3 * kTile && r2) {
      const long e = e0 + tid - 2 * kTile;
      s_r[tid - 2 * kTile] = e < E ? ld1<float>(r2, e) : 0.f;
    }
    __syncthreads();
    const long e = e0 + el;
    for (int ft = 0; ft < H / 64; ++ft) {
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m] = {0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < D / 32; ++ks) {
        const int kk = ks * 32 + q * 8;
        const auto ef = frag<T>(s_e + el * lw + kk);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int f = 64 * ft + 32 * (m >> 1) + interleaved_row(col, m & 1);
          acc[m] = Mfma<T>::run(frag<T>(s_w + f * lw + kk), ef, acc[m]);
        }
      }
      if (e < E) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int f0 = 64 * ft + 32 * p + 8 * q;
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = 0.f;
          if (P) {
            const P8 pi = *reinterpret_cast<const P8*>(
                P + s_i[el] * 2 * H + f0);
            const P8 pj = *reinterpret_cast<const P8*>(
                P + (s_i[kTile + el] * 2 + 1) * H + f0);
#pragma unroll
            for (int r = 0; r < 8; ++r)
              v[r] = ld<float>(pi, r) + ld<float>(pj, r);
          }
          if (r2) {
            const float rr = s_r[el];
            const P8 w = *reinterpret_cast<const P8*>(wr + f0);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += rr * ld<float>(w, r);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[r] += acc[2 * p][r];
            v[4 + r] += acc[2 * p + 1][r];
          }
          if (b) {
            const P8 bv = *reinterpret_cast<const P8*>(b + f0);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += ld<float>(bv, r);
          }
          P8 out;
#pragma unroll
          for (int r = 0; r < 8; ++r) st(out, r, v[r]);
          *reinterpret_cast<P8*>(z + e * H + f0) = out;
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// edge
// ---------------------------------------------------------------------------
// LDS: W_e^T [D][H + 8], the tile's g [64][H + 8], w_r [H] as fp32.  dea
// comes from the fragments; dr2, when asked for, from the staged tile on
// the vector ALU: four lanes per edge sum a quarter of the features each
// in ascending order and meet in two __shfl_xor steps.
template <typename T>
__global__ void __launch_bounds__(kBlock) pair_affine_wide_edge_kernel(
    const T* __restrict__ g, const T* __restrict__ wr,
    const T* __restrict__ weT, T* __restrict__ dr2, T* __restrict__ dea,
    long E, int H, int D) {
  using P8 = Pack<T, 8>;
  extern __shared__ __align__(16) unsigned char pair_affine_wide_lds[];
  const int lw = H + kPad;
  u16* s_w = reinterpret_cast<u16*>(pair_affine_wide_lds);
  u16* s_g = s_w + D * lw;
  float* s_wr = reinterpret_cast<float*>(s_g + kTile * lw);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, q = lane >> 4;
  const int el = 16 * wave + col;
  const int n_kt = D / 32;
  stage_rows<T>(weT, s_w, 0, D, D, H, lw);
  if (dr2)
    for (int f = tid; f < H; f += kBlock) s_wr[f] = ld1<float>(wr, f);
  const long n_tiles = (E + kTile - 1) / kTile;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long e0 = t * kTile;
    stage_rows<T>(g, s_g, e0, kTile, E, H, lw);
    __syncthreads();
    f32x4 acc[kMaxKT][2];
#pragma unroll
    for (int kt = 0; kt < kMaxKT; ++kt)
      acc[kt][0] = acc[kt][1] = {0.f, 0.f, 0.f, 0.f};
    for (int fs = 0; fs < H / 32; ++fs) {
      const int ff = fs * 32 + q * 8;
      const auto gf = frag<T>(s_g + el * lw + ff);
#pragma unroll
      for (int kt = 0; kt < kMaxKT; ++kt) {
        if (kt < n_kt) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int k = 32 * kt + interleaved_row(col, h);
            acc[kt][h] =
                Mfma<T>::run(frag<T>(s_w + k * lw + ff), gf, acc[kt][h]);
          }
        }
      }
    }
    const long e = e0 + el;
    if (e < E) {
#pragma unroll
      for (int kt = 0; kt < kMaxKT; ++kt) {
        if (kt < n_kt) {
          P8 out;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st(out, r, acc[kt][0][r]);
            st(out, 4 + r, acc[kt][1][r]);
          }
          *reinterpret_cast<P8*>(dea + e * D + 32 * kt + 8 * q) = out;
        }
      }
    }
    if (dr2) {
      const int er = tid >> 2, part = tid & 3;
      const int quarter = H / 4;
      float s = 0.f;
      for (int f = part * quarter; f < (part + 1) * quarter; f += 8) {
        const P8 gv = *reinterpret_cast<const P8*>(s_g + er * lw + f);
#pragma unroll
        for (int r = 0; r < 8; ++r) s += ld<float>(gv, r) * s_wr[f + r];
      }
      s += __shfl_xor(s, 1, 4);
      s += __shfl_xor(s, 2, 4);
      if (part == 0 && e0 + er < E) st1(dr2, e0 + er, s);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// param
// ---------------------------------------------------------------------------
// rows (2 ep, 2 ep + 1) x 8 columns, 16 bytes each -> the transposed LDS
// image [col][e]: a dword holds column col0 + t of the two rows
__device__ __forceinline__ void store_pair_t(u16* dst, int col0, int ep,
                                             u32x4 v0, u32x4 v1) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const unsigned a = v0[t >> 1], c = v1[t >> 1];
    *reinterpret_cast<unsigned*>(dst + (col0 + t) * kStageLd + 2 * ep) =
        (t & 1) ? (a >> 16) | (c & 0xffff0000u) : (a & 0xffffu) | (c << 16);
  }
}

// grid (chunk, feature tile).  LDS: g^T [64 features][64 + 8 edges] and
// the column operand [D + 16][64 + 8]: rows 0 .. D - 1 are ea^T, row D is
// r2, row D + 1 is 1 on live edges, the rest stays 0.  A staging unit is
// a pair of rows x 8 columns: 256 units of g, 4 D of ea.
template <typename T>
__global__ void __launch_bounds__(kBlock) pair_affine_wide_param_kernel(
    const T* __restrict__ g, const T* __restrict__ r2,
    const T* __restrict__ ea, float* __restrict__ partial, long E, int H,
    int D, long chunk_len) {
  extern __shared__ __align__(16) unsigned char pair_affine_wide_lds[];
  u16* s_g = reinterpret_cast<u16*>(pair_affine_wide_lds);
  u16* s_p = s_g + 64 * kStageLd;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, q = lane >> 4;
  const long chunk = blockIdx.x;
  const int f_base = blockIdx.y * 64;
  const long lo = chunk * chunk_len;
  const long hi = lo + chunk_len < E ? lo + chunk_len : E;
  const int n_nt = D / 16 + 1;
  const int per_row = D / 8;
  const u16* __restrict__ r2b = reinterpret_cast<const u16*>(r2);
  const u16 one = Bits<T>::put(1.f);

  for (int i = tid; i < 16 * kStageLd; i += kBlock) s_p[D * kStageLd + i] = 0;

  f32x4 acc[kMaxNT];
#pragma unroll
  for (int j = 0; j < kMaxNT; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};

  u32x4 gv[2], ev[2][2];
  u16 rv = 0, ov = 0;
  const int g_ep = (tid & 15) | ((tid >> 7) << 4);
  const int g_c8 = ((tid >> 4) & 7) * 8;
  auto load = [&](long e0) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long e = e0 + 2 * g_ep + r;
      gv[r] = e < hi
          ? *reinterpret_cast<const u32x4*>(g + e * H + f_base + g_c8) : zero;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = it * kBlock + tid;
      if (u < 4 * D) {
        const int ep = (u & 15) | (((u >> 4) / per_row) << 4);
        const int c8 = ((u >> 4) % per_row) * 8;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const long e = e0 + 2 * ep + r;
          ev[it][r] = e < hi
              ? *reinterpret_cast<const u32x4*>(ea + e * D + c8) : zero;
        }
      }
    }
    if (tid < kTile) {
      const bool ok = e0 + tid < hi;
      rv = ok && r2 ? r2b[e0 + tid] : (u16)0;
      ov = ok ? one : (u16)0;
    }
  };
  auto store = [&]() {
    store_pair_t(s_g, g_c8, g_ep, gv[0], gv[1]);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int u = it * kBlock + tid;
      if (u < 4 * D) {
        const int ep = (u & 15) | (((u >> 4) / per_row) << 4);
        const int c8 = ((u >> 4) % per_row) * 8;
        store_pair_t(s_p, c8, ep, ev[it][0], ev[it][1]);
      }
    }
    if (tid < kTile) {
      s_p[D * kStageLd + tid] = rv;
      s_p[(D + 1) * kStageLd + tid] = ov;
    }
  };

  if (lo < hi) load(lo);
  for (long e0 = lo; e0 < hi; e0 += kTile) {
    __syncthreads();               // the previous stage's reads are done
    store();
    __syncthreads();
    if (e0 + kTile < hi) load(e0 + kTile);   // in flight under the MFMAs
#pragma unroll
    for (int s = 0; s < kTile / 32; ++s) {
      const int ee = s * 32 + q * 8;
      const auto gf = frag<T>(s_g + (16 * wave + col) * kStageLd + ee);
#pragma unroll
      for (int j = 0; j < kMaxNT; ++j)
        if (j < n_nt)
          acc[j] = Mfma<T>::run(
              gf, frag<T>(s_p + (16 * j + col) * kStageLd + ee), acc[j]);
    }
  }

  // result: rows 4 q + reg are four consecutive features, col is the
  // column of [ea | r2 | 1 | 0 ...]; slot 0 is dw_r, 1 .. D dW_e, 1 + D db
  const int slots = 2 + D;
  const int f0 = f_base + 16 * wave + 4 * q;
#pragma unroll
  for (int j = 0; j < kMaxNT; ++j) {
    if (j < n_nt) {
      const int c = 16 * j + col;
      const int slot = c < D ? 1 + c : (c == D ? 0 : (c == D + 1 ? 1 + D : -1));
      if (slot >= 0)
        *reinterpret_cast<f32x4*>(partial + (chunk * slots + slot) * H + f0) =
            acc[j];
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using OptTensor = c10::optional<torch::Tensor>;

bool half_type(at::ScalarType t) {
  return t == at::ScalarType::BFloat16 || t == at::ScalarType::Half;
}

void check_envelope(at::ScalarType dtype, long E, long H, long D) {
  TORCH_CHECK(half_type(dtype), "pair_affine_wide: bf16 or f16 only");
  TORCH_CHECK(D % 32 == 0 && D >= 32 && D <= kMaxD && H % 64 == 0 &&
                  H >= 64 && H <= kMaxH,
              "pair_affine_wide: D must be a multiple of 32 in [32, ", kMaxD,
              "] and H a multiple of 64 in [64, ", kMaxH, "]; got D=", D,
              " H=", H);
  TORCH_CHECK(E >= 0 && E < (1L << 31),
              "pair_affine_wide: E must be below 2^31");
}

void check_lds(size_t lds, const char* what) {
  const size_t limit = std::min<size_t>(
      kLdsBudget, at::cuda::getCurrentDeviceProperties()->sharedMemPerBlock);
  TORCH_CHECK(lds <= limit, what, " needs ", lds, " bytes of LDS, the limit is ",
              limit);
}

// A contiguous GPU tensor of `dtype` with `numel` elements that starts
// on 16 bytes (a copy where the given one does not); a null pointer for
// an absent operand.  `keep` holds the tensor the pointer belongs to.
const void* operand(const OptTensor& t, at::ScalarType dtype, long numel,
                    torch::Tensor& keep, const char* what) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                  t->scalar_type() == dtype && t->numel() == numel,
              "pair_affine_wide: ", what,
              " must be a contiguous GPU tensor of ", numel,
              " elements of the common dtype");
  keep = aligned16(t->data_ptr()) ? *t : t->clone();
  return keep.data_ptr();
}

// persistent blocks over `tiles` tiles: as many as the LDS of the CUs
// holds at once, at most eight per CU and the grid cap
unsigned persistent_blocks(long tiles, size_t lds) {
  const auto* prop = at::cuda::getCurrentDeviceProperties();
  const size_t cu_lds = std::max<size_t>(prop->maxSharedMemoryPerMultiProcessor,
                                         prop->sharedMemPerBlock);
  const long per_cu = std::max<long>(1, std::min<long>(8, cu_lds / lds));
  const long cap = std::min<long>(
      kGridCap, per_cu * std::max(1, prop->multiProcessorCount));
  return (unsigned)std::max<long>(1, std::min<long>(tiles, cap));
}

template <typename F>
void dispatch_half(at::ScalarType dtype, F&& f) {
  if (dtype == at::ScalarType::BFloat16)
    f(c10::BFloat16());
  else
    f(c10::Half());
}

}  // namespace

// z[E, H]; ea[E, D] with We[H, D] is needed, P[N, 2H] (with didx, sidx),
// r2[E] with w_r[H] and b[H] may each be absent
torch::Tensor pair_affine_wide_fwd(OptTensor P, OptTensor r2, torch::Tensor ea,
                                   OptTensor wr, torch::Tensor We, OptTensor b,
                                   OptTensor didx, OptTensor sidx, long E,
                                   long H) {
  TORCH_CHECK(ea.is_cuda() && ea.dim() == 2 && We.dim() == 2,
              "pair_affine_wide_fwd: ea [E, D] and W_e [H, D] on the GPU");
  const long D = ea.size(1);
  const auto dtype = ea.scalar_type();
  check_envelope(dtype, E, H, D);
  TORCH_CHECK(r2.has_value() == wr.has_value(),
              "pair_affine_wide_fwd: r2 goes with w_r");
  long N = 0;
  if (P.has_value()) {
    TORCH_CHECK(P->dim() == 2 && P->size(1) == 2 * H,
                "pair_affine_wide_fwd: P must be [N, 2H]");
    TORCH_CHECK(didx.has_value() && sidx.has_value(),
                "pair_affine_wide_fwd: P needs both indices");
    N = P->size(0);
  }
  torch::Tensor kP, kr, ke, kw, kW, kb, dk, sk;
  const void* Pv = operand(P, dtype, N * 2 * H, kP, "P");
  const void* rv = operand(r2, dtype, E, kr, "r2");
  const void* ev = operand(ea, dtype, E * D, ke, "ea");
  const void* wv = operand(wr, dtype, H, kw, "w_r");
  const void* Wv = operand(We, dtype, H * D, kW, "W_e");
  const void* bv = operand(b, dtype, H, kb, "b");
  const long* dp =
      P.has_value() ? index_ptr(didx, E, dk, "pair_affine_wide: dst") : nullptr;
  const long* sp =
      P.has_value() ? index_ptr(sidx, E, sk, "pair_affine_wide: src") : nullptr;
  if (E == 0 || (P.has_value() && N == 0))
    return torch::zeros({E, H}, ea.options());
  const size_t lds = (size_t)(H + kTile) * (D + kPad) * 2 +
                     2 * kTile * sizeof(long) + kTile * sizeof(float);
  check_lds(lds, "pair_affine_wide_fwd");
  auto z = torch::empty({E, H}, ea.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  const long tiles = (E + kTile - 1) / kTile;
  dispatch_half(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(pair_affine_wide_fwd_kernel<T>,
                       dim3(persistent_blocks(tiles, lds)), dim3(kBlock), lds,
                       stream, (const T*)Pv, (const T*)rv, (const T*)ev,
                       (const T*)wv, (const T*)Wv, (const T*)bv, dp, sp,
                       (T*)z.data_ptr(), E, (int)H, (int)D);
  });
  check_launch("pair_affine_wide_fwd_kernel");
  return z;
}

// (dr2[E] or undefined when w_r is absent, dea[E, D]); weT is W_e^T [D, H]
std::vector<torch::Tensor> pair_affine_wide_edge(torch::Tensor g, OptTensor wr,
                                                 torch::Tensor weT) {
  TORCH_CHECK(g.is_cuda() && g.dim() == 2 && weT.dim() == 2,
              "pair_affine_wide_edge: g [E, H] and W_e^T [D, H] on the GPU");
  const long E = g.size(0), H = g.size(1), D = weT.size(0);
  const auto dtype = g.scalar_type();
  check_envelope(dtype, E, H, D);
  torch::Tensor kg, kw, kW;
  const void* gv = operand(g, dtype, E * H, kg, "g");
  const void* wv = operand(wr, dtype, H, kw, "w_r");
  const void* Wv = operand(weT, dtype, D * H, kW, "W_e^T");
  torch::Tensor dr2, dea = torch::empty({E, D}, g.options());
  if (wr.has_value()) dr2 = torch::empty({E}, g.options());
  if (E == 0) return {dr2, dea};
  const size_t lds =
      (size_t)(D + kTile) * (H + kPad) * 2 + (size_t)H * sizeof(float);
  check_lds(lds, "pair_affine_wide_edge");
  auto stream = at::hip::getCurrentHIPStream().stream();
  const long tiles = (E + kTile - 1) / kTile;
  dispatch_half(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(pair_affine_wide_edge_kernel<T>,
                       dim3(persistent_blocks(tiles, lds)), dim3(kBlock), lds,
                       stream, (const T*)gv, (const T*)wv, (const T*)Wv,
                       wr.has_value() ? (T*)dr2.data_ptr() : nullptr,
                       (T*)dea.data_ptr(), E, (int)H, (int)D);
  });
  check_launch("pair_affine_wide_edge_kernel");
  return {dr2, dea};
}

// (dw_r[H] or undefined when r2 is absent, dW_e[H, D], db[H] or
// undefined when want_bias is false)
std::vector<torch::Tensor> pair_affine_wide_param(torch::Tensor g,
                                                  OptTensor r2,
                                                  torch::Tensor ea,
                                                  bool want_bias) {
  TORCH_CHECK(g.is_cuda() && g.dim() == 2 && ea.dim() == 2 &&
                  ea.size(0) == g.size(0),
              "pair_affine_wide_param: g [E, H] and ea [E, D] on the GPU");
  const long E = g.size(0), H = g.size(1), D = ea.size(1);
  const auto dtype = g.scalar_type();
  check_envelope(dtype, E, H, D);
  torch::Tensor kg, kr, ke;
  const void* gv = operand(g, dtype, E * H, kg, "g");
  const void* rv = operand(r2, dtype, E, kr, "r2");
  const void* ev = operand(ea, dtype, E * D, ke, "ea");
  torch::Tensor dwr, dWe, db;
  auto make = [&](std::vector<int64_t> shape) {
    return E == 0 ? torch::zeros(shape, g.options())
                  : torch::empty(shape, g.options());
  };
  if (r2.has_value()) dwr = make({H});
  dWe = make({H, D});
  if (want_bias) db = make({H});
  if (E == 0) return {dwr, dWe, db};
  const long n_chunks = pair_affine_param_chunks(E);
  const long chunk_len = (E + n_chunks - 1) / n_chunks;
  const size_t lds = (size_t)(64 + D + 16) * kStageLd * 2;
  check_lds(lds, "pair_affine_wide_param");
  auto partial = torch::empty({n_chunks, 2 + D, H},
                              g.options().dtype(torch::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  dispatch_half(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(pair_affine_wide_param_kernel<T>,
                       dim3((unsigned)n_chunks, (unsigned)(H / 64)),
                       dim3(kBlock), lds, stream, (const T*)gv, (const T*)rv,
                       (const T*)ev, partial.data_ptr<float>(), E, (int)H,
                       (int)D, chunk_len);
  });
  check_launch("pair_affine_wide_param_kernel");
  pair_affine_param_reduce(partial, dwr, dWe, db, H, D, n_chunks);
  return {dwr, dWe, db};
}
