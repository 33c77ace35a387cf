// Segment-varlen attention for GPS global attention (gfx950).
//
// Graph batches are many variable-size segments (molecules 10-128
// nodes, OC20 slabs ~80, supercells 1k+); the dense-batch SDPA path
// pads every graph to max_N and runs masked attention over padding.
// This kernel processes one (graph, head) per workgroup with K and V
// staged through LDS in tiles, one thread per query row, and an
// online softmax — no padding, no masks, no [B, maxN, ...]
// materialization, and no segment-length limit (r2: the r1 kernel
// required seg <= 256 and fp32 only).
//
// dtype: fp32 or bf16 inputs; LDS staging and accumulation in fp32.
//
// Two kernel generations live here:
//  * varlen_attn_kernel (head_dim <= 64): the original forward entry
//    point, per-thread rows as runtime-indexed LDS slices.
//  * varlen_attn_fwd_kernel / _dq_kernel / _dkv_kernel (head_dim <=
//    128): the training path.  Templated on a compile-time per-lane
//    width so the thread's own rows live in registers; the forward
//    also stores the row log-sum-exp, and the backward is two
//    atomic-free passes (thread = query row for dQ, thread = key row
//    for dK/dV) that recompute P from LSE.
//  * varlen_attn_bwd2_q_kernel / _bwd2_k_kernel (head_dim <= 128): the
//    double backward of force training, the same two-pass mapping
//    with at most 32 head dims per lane.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "check_launch.h"

namespace {

constexpr int kMaxDh = 64;
constexpr int kTile = 128;      // K/V rows staged per LDS pass
constexpr int kThreads = 128;

template <typename T>
__device__ inline float to_f32(T v);
template <>
__device__ inline float to_f32<float>(float v) { return v; }
template <>
__device__ inline float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <typename T>
__device__ inline T from_f32(float v);
template <>
__device__ inline float from_f32<float>(float v) { return v; }
template <>
__device__ inline __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void varlen_attn_kernel(
    const T* __restrict__ Q,   // [N, H, dh]
    const T* __restrict__ K,
    const T* __restrict__ V,
    T* __restrict__ O,         // [N, H, dh]
    const long* __restrict__ ptr,  // [G+1] node offsets per graph
    int H, int dh, float scale) {
  __shared__ float lK[kTile * kMaxDh];
  __shared__ float lV[kTile * kMaxDh];
  // per-thread state slices (runtime-indexed; LDS not registers)
  __shared__ float lAcc[kThreads * (kMaxDh + 1)];
  __shared__ float lQ[kThreads * (kMaxDh + 1)];

  int g = blockIdx.x;
  int h = blockIdx.y;
  long lo = ptr[g], hi = ptr[g + 1];
  int n = (int)(hi - lo);
  if (n <= 0) return;

  float* acc = &lAcc[threadIdx.x * (kMaxDh + 1)];
  float* qv = &lQ[threadIdx.x * (kMaxDh + 1)];

  // queries handled by this thread: q0, q0+kThreads, ...  To keep the
  // tile loop uniform across the block (needed for __syncthreads),
  // every thread walks all tiles even when it has no query row.
  for (int q0 = 0; q0 < n; q0 += kThreads) {
    int q = q0 + threadIdx.x;
    bool hasq = q < n;
    float m = -1e30f, l = 0.f;
    if (hasq) {
      const T* qp = &Q[((lo + q) * (long)H + h) * dh];
      for (int d = 0; d < dh; ++d) qv[d] = to_f32<T>(qp[d]);
      for (int d = 0; d < dh; ++d) acc[d] = 0.f;
    }
    for (int t0 = 0; t0 < n; t0 += kTile) {
      int tn = n - t0 < kTile ? n - t0 : kTile;
      __syncthreads();
      for (int i = threadIdx.x; i < tn * dh; i += kThreads) {
        int row = i / dh, d = i - (i / dh) * dh;
        lK[row * kMaxDh + d] =
            to_f32<T>(K[((lo + t0 + row) * (long)H + h) * dh + d]);
        lV[row * kMaxDh + d] =
            to_f32<T>(V[((lo + t0 + row) * (long)H + h) * dh + d]);
      }
      __syncthreads();
      if (hasq) {
        for (int k = 0; k < tn; ++k) {
          float s = 0.f;
          const float* kp = &lK[k * kMaxDh];
          for (int d = 0; d < dh; ++d) s += qv[d] * kp[d];
          s *= scale;
          float m_new = s > m ? s : m;
          float alpha = __expf(m - m_new);
          float p = __expf(s - m_new);
          l = l * alpha + p;
          const float* vp = &lV[k * kMaxDh];
          for (int d = 0; d < dh; ++d)
            acc[d] = acc[d] * alpha + p * vp[d];
          m = m_new;
        }
      }
    }
    if (hasq) {
      float inv = 1.f / l;
      T* op = &O[((lo + q) * (long)H + h) * dh];
      for (int d = 0; d < dh; ++d) op[d] = from_f32<T>(acc[d] * inv);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------
// Training path: forward with LSE, and the two backward passes.
//
// An instance is VCfg<DHL, L, T>: every row (query or key) is owned by
// L adjacent lanes, each holding DHL consecutive head dims of it in
// registers (compile-time unrolled; dims past the runtime head_dim are
// zero, in registers and in the LDS tiles alike, so no inner loop
// carries a bound check).  L = 2 covers 64 < head_dim <= 128 with 64
// registers per row per lane; the two partial dot products meet in
// one __shfl_xor, a fixed order, so results stay bitwise reproducible.
// The other side is staged through LDS in T-row fp32 tiles.  All lanes
// read the same tile row (a broadcast); with L = 2 the two lane
// halves of a row are kSub = DHL + 4 floats apart, which puts their
// 16-byte reads on different banks (DHL alone would be 64 dwords = the
// same bank) and keeps them 16-byte aligned.

constexpr int kBlock = 128;            // threads per workgroup
constexpr long kLdsBudget = 160 * 1024;

template <int DHL_, int L_, int T_>
struct VCfg {
  static constexpr int DHL = DHL_;     // head dims per lane
  static constexpr int L = L_;         // lanes per row
  static constexpr int T = T_;         // tile rows per LDS pass
  static constexpr int kRows = kBlock / L;   // rows owned per pass
  static constexpr int kCap = L * DHL;       // head_dim ceiling
  static constexpr int kSub = DHL + (L > 1 ? 4 : 0);
  static constexpr int kRowStride = L * kSub;
  static constexpr int kTileFloats = T * kRowStride;
  // static LDS bytes per pass (no dynamic LDS): two tiles; the dK/dV
  // pass also stages LSE and D of the tile's query rows
  static constexpr long kLdsFwd = 2L * kTileFloats * sizeof(float);
  static constexpr long kLdsDq = kLdsFwd;
  static constexpr long kLdsDkv = kLdsFwd + 2L * T * sizeof(float);
};

using VCfg16 = VCfg<16, 1, 64>;
using VCfg32 = VCfg<32, 1, 64>;
using VCfg64 = VCfg<64, 1, 64>;
using VCfg128 = VCfg<64, 2, 32>;

// Stage tn rows of one head into an LDS tile, zero past head_dim.
// src points at (first row, head h); rows are rs elements apart.
template <typename C, typename T>
__device__ inline void stage_tile(float* __restrict__ dst,
                                  const T* __restrict__ src, long rs,
                                  int tn, int dh) {
  for (int i = threadIdx.x; i < tn * C::kCap; i += kBlock) {
    int row = i / C::kCap, d = i % C::kCap;
    float x = d < dh ? to_f32<T>(src[row * rs + d]) : 0.f;
    dst[row * C::kRowStride + (d / C::DHL) * C::kSub + d % C::DHL] = x;
  }
}

// This lane's DHL dims of a row into registers (times mul), zero
// where the row or the dim does not exist.
template <typename C, typename T>
__device__ inline void load_row(float (&r)[C::DHL],
                                const T* __restrict__ p, int sub, int dh,
                                bool on, float mul) {
#pragma unroll
  for (int d = 0; d < C::DHL; ++d) {
    int c = sub * C::DHL + d;
    r[d] = (on && c < dh) ? to_f32<T>(p[c]) * mul : 0.f;
  }
}

template <typename C, typename T>
__device__ inline void store_row(T* __restrict__ p,
                                 const float (&r)[C::DHL], int sub,
                                 int dh, float mul) {
#pragma unroll
  for (int d = 0; d < C::DHL; ++d) {
    int c = sub * C::DHL + d;
    if (c < dh) p[c] = from_f32<T>(r[d] * mul);
  }
}

// Register row times one lane-slice of an LDS tile row, summed over
// the row's L lanes.
template <typename C>
__device__ inline float dot_row(const float (&a)[C::DHL],
                                const float* __restrict__ b) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int d = 0; d < C::DHL; d += 4) {
    float4 x = *reinterpret_cast<const float4*>(b + d);
    s0 += a[d] * x.x;
    s1 += a[d + 1] * x.y;
    s2 += a[d + 2] * x.z;
    s3 += a[d + 3] * x.w;
  }
  float s = (s0 + s1) + (s2 + s3);
  if (C::L > 1) s += __shfl_xor(s, 1);
  if (C::L > 2) s += __shfl_xor(s, 2);
  return s;
}

template <typename C>
__device__ inline void axpy_row(float (&acc)[C::DHL], float a,
                                const float* __restrict__ b) {
#pragma unroll
  for (int d = 0; d < C::DHL; d += 4) {
    float4 x = *reinterpret_cast<const float4*>(b + d);
    acc[d] += a * x.x;
    acc[d + 1] += a * x.y;
    acc[d + 2] += a * x.z;
    acc[d + 3] += a * x.w;
  }
}

// Forward, thread = query row, K/V tiled; also writes LSE = m + log l.
template <typename C, typename T>
__global__ __launch_bounds__(kBlock) void varlen_attn_fwd_kernel(
    const T* __restrict__ Q,   // [N, H, dh]
    const T* __restrict__ K, const T* __restrict__ V,
    T* __restrict__ O,         // [N, H, dh]
    float* __restrict__ LSE,   // [N, H]
    const long* __restrict__ ptr, int H, int dh, float scale) {
  __shared__ __align__(16) float lK[C::kTileFloats];
  __shared__ __align__(16) float lV[C::kTileFloats];

  const int h = blockIdx.y;
  const long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  const int r = threadIdx.x / C::L, sub = threadIdx.x % C::L;
  const long rs = (long)H * dh;

  // every thread walks all tiles, with or without a row of its own,
  // so the __syncthreads() stay block-uniform; the segment's row
  // chunks are dealt round-robin to the gridDim.z workgroups of this
  // (graph, head), and a workgroup without a chunk leaves at once
  for (int q0 = blockIdx.z * C::kRows; q0 < n;
       q0 += gridDim.z * C::kRows) {
    const int q = q0 + r;
    const bool hasq = q < n;
    const long qoff = ((lo + q) * (long)H + h) * dh;
    float qv[C::DHL], acc[C::DHL];
    load_row<C, T>(qv, Q + qoff, sub, dh, hasq, scale);
#pragma unroll
    for (int d = 0; d < C::DHL; ++d) acc[d] = 0.f;
    float m = -1e30f, l = 0.f;
    for (int t0 = 0; t0 < n; t0 += C::T) {
      const int tn = n - t0 < C::T ? n - t0 : C::T;
      const long toff = ((lo + t0) * (long)H + h) * dh;
      __syncthreads();
      stage_tile<C, T>(lK, K + toff, rs, tn, dh);
      stage_tile<C, T>(lV, V + toff, rs, tn, dh);
      __syncthreads();
      if (hasq) {
        for (int k = 0; k < tn; ++k) {
          const int o = k * C::kRowStride + sub * C::kSub;
          float s = dot_row<C>(qv, lK + o);
          float m_new = s > m ? s : m;
          float alpha = __expf(m - m_new);
          float p = __expf(s - m_new);
          l = l * alpha + p;
#pragma unroll
          for (int d = 0; d < C::DHL; ++d) acc[d] *= alpha;
          axpy_row<C>(acc, p, lV + o);
          m = m_new;
        }
      }
    }
    if (hasq) {
      store_row<C, T>(O + qoff, acc, sub, dh, 1.f / l);
      if (sub == 0) LSE[(lo + q) * (long)H + h] = m + logf(l);
    }
  }
}

// Backward pass 1, thread = query row, K/V tiled:
//   D_i = sum_d dO_id O_id            (also written out for pass 2)
//   dQ_i = scale * sum_j P_ij (dO_i.v_j - D_i) k_j
template <typename C, typename T>
__global__ __launch_bounds__(kBlock) void varlen_attn_dq_kernel(
    const T* __restrict__ Q, const T* __restrict__ K,
    const T* __restrict__ V, const T* __restrict__ O,
    const float* __restrict__ LSE, const T* __restrict__ dO,
    T* __restrict__ dQ, float* __restrict__ D,   // D [N, H]
    const long* __restrict__ ptr, int H, int dh, float scale) {
  __shared__ __align__(16) float lK[C::kTileFloats];
  __shared__ __align__(16) float lV[C::kTileFloats];

  const int h = blockIdx.y;
  const long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  const int r = threadIdx.x / C::L, sub = threadIdx.x % C::L;
  const long rs = (long)H * dh;

  for (int q0 = blockIdx.z * C::kRows; q0 < n;
       q0 += gridDim.z * C::kRows) {
    const int q = q0 + r;
    const bool hasq = q < n;
    const long qoff = ((lo + q) * (long)H + h) * dh;
    float qv[C::DHL], gv[C::DHL], dq[C::DHL];
    load_row<C, T>(qv, Q + qoff, sub, dh, hasq, scale);
    load_row<C, T>(gv, dO + qoff, sub, dh, hasq, 1.f);
    float lse = 0.f, Di = 0.f;
    if (hasq) {
#pragma unroll
      for (int d = 0; d < C::DHL; ++d) {
        int c = sub * C::DHL + d;
        if (c < dh) Di += gv[d] * to_f32<T>(O[qoff + c]);
      }
      if (C::L > 1) Di += __shfl_xor(Di, 1);
      lse = LSE[(lo + q) * (long)H + h];
      if (sub == 0) D[(lo + q) * (long)H + h] = Di;
    }
#pragma unroll
    for (int d = 0; d < C::DHL; ++d) dq[d] = 0.f;
    for (int t0 = 0; t0 < n; t0 += C::T) {
      const int tn = n - t0 < C::T ? n - t0 : C::T;
      const long toff = ((lo + t0) * (long)H + h) * dh;
      __syncthreads();
      stage_tile<C, T>(lK, K + toff, rs, tn, dh);
      stage_tile<C, T>(lV, V + toff, rs, tn, dh);
      __syncthreads();
      if (hasq) {
        for (int k = 0; k < tn; ++k) {
          const int o = k * C::kRowStride + sub * C::kSub;
          float s = dot_row<C>(qv, lK + o);
          float dp = dot_row<C>(gv, lV + o);
          float ds = __expf(s - lse) * (dp - Di);
          axpy_row<C>(dq, ds, lK + o);
        }
      }
    }
    if (hasq) store_row<C, T>(dQ + qoff, dq, sub, dh, scale);
  }
}

// Backward pass 2, thread = key row, Q/dO/LSE/D tiled:
//   dV_j = sum_i P_ij dO_i
//   dK_j = scale * sum_i P_ij (dO_i.v_j - D_i) q_i
template <typename C, typename T>
__global__ __launch_bounds__(kBlock) void varlen_attn_dkv_kernel(
    const T* __restrict__ Q, const T* __restrict__ K,
    const T* __restrict__ V, const float* __restrict__ LSE,
    const float* __restrict__ D, const T* __restrict__ dO,
    T* __restrict__ dK, T* __restrict__ dV,
    const long* __restrict__ ptr, int H, int dh, float scale) {
  __shared__ __align__(16) float lQ[C::kTileFloats];
  __shared__ __align__(16) float lG[C::kTileFloats];
  __shared__ float lLse[C::T];
  __shared__ float lD[C::T];

  const int h = blockIdx.y;
  const long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  const int r = threadIdx.x / C::L, sub = threadIdx.x % C::L;
  const long rs = (long)H * dh;

  for (int j0 = blockIdx.z * C::kRows; j0 < n;
       j0 += gridDim.z * C::kRows) {
    const int j = j0 + r;
    const bool hask = j < n;
    const long koff = ((lo + j) * (long)H + h) * dh;
    float kv[C::DHL], vv[C::DHL], dk[C::DHL], dv[C::DHL];
    load_row<C, T>(kv, K + koff, sub, dh, hask, scale);
    load_row<C, T>(vv, V + koff, sub, dh, hask, 1.f);
#pragma unroll
    for (int d = 0; d < C::DHL; ++d) dk[d] = dv[d] = 0.f;
    for (int t0 = 0; t0 < n; t0 += C::T) {
      const int tn = n - t0 < C::T ? n - t0 : C::T;
      const long toff = ((lo + t0) * (long)H + h) * dh;
      __syncthreads();
      stage_tile<C, T>(lQ, Q + toff, rs, tn, dh);
      stage_tile<C, T>(lG, dO + toff, rs, tn, dh);
      for (int i = threadIdx.x; i < tn; i += kBlock) {
        lLse[i] = LSE[(lo + t0 + i) * (long)H + h];
        lD[i] = D[(lo + t0 + i) * (long)H + h];
      }
      __syncthreads();
      if (hask) {
        for (int i = 0; i < tn; ++i) {
          const int o = i * C::kRowStride + sub * C::kSub;
          float s = dot_row<C>(kv, lQ + o);
          float dp = dot_row<C>(vv, lG + o);
          float p = __expf(s - lLse[i]);
          axpy_row<C>(dv, p, lG + o);
          axpy_row<C>(dk, p * (dp - lD[i]), lQ + o);
        }
      }
    }
    if (hask) {
      store_row<C, T>(dV + koff, dv, sub, dh, 1.f);
      store_row<C, T>(dK + koff, dk, sub, dh, scale);
    }
  }
}

// ---------------------------------------------------------------
// Second order: the backward of the backward pair above.  Inputs are
// the first order's (q, k, v, O, LSE, g = dO) and the cotangents
// (cq, ck, cv) of its outputs (dQ, dK, dV); outputs are the gradients
// of R = <cq,dQ> + <ck,dK> + <cv,dV> with respect to q, k, v and g,
// with O and LSE taken as functions of (q, k, v).  Per pair (i, j):
//   P = exp(s - LSE_i)          s = scale q_i.k_j
//   a = g_i.v_j                 T = scale (cq_i.k_j + q_i.ck_j)
//   W = g_i.cv_j                D_i = g_i.O_i = sum_j P a
//   t_i = sum_j P T,  e_i = sum_j P T a - 2 t_i D_i + sum_j P W
//   E = (T - t_i) a - D_i T + W,  GS = P (E - e_i),  dS = P (a - D_i)
//   gg_i = sum_j P [(T - t_i) v_j + cv_j]
//   gv_j = sum_i P (T - t_i) g_i
//   gq_i = scale sum_j [GS k_j + dS ck_j]
//   gk_j = scale sum_i [GS q_i + dS cq_i]
// Same mapping as the first order: a query-side kernel (which also
// writes the row statistics) and then a key-side kernel.
//
// The stored LSE only shifts the exponent: the query side sums
// l_i = sum_j exp(s - LSE_i) along with the other statistics, divides
// them by it and hands LSE_i + log l_i on, so every P row sums to one
// in this kernel's own arithmetic and the rounding of the stored LSE
// (a relative error common to a whole row of P) drops out.  For the
// same reason D_i is summed as sum_j P a in fp32 and not taken from
// the stored O, which in bf16 carries an output rounding; O is not
// read at all.
//
// A pair costs five dot products and a thread group carries five
// (query side) or six (key side) register rows, so a lane holds at
// most 32 head dims and a row spreads over L = 1, 2 or 4 lanes.

template <int DHL_, int L_, int T_>
struct VCfg2 {
  static constexpr int DHL = DHL_;
  static constexpr int L = L_;
  static constexpr int T = T_;
  static constexpr int kRows = kBlock / L;
  static constexpr int kCap = L * DHL;
  // lane slices of a tile row DHL + 4 floats apart: with DHL = 32 the
  // L slices then start on banks 0, 36, 8, 44 (mod 64), so the L
  // distinct 16-byte reads of a wave never share a bank
  static constexpr int kSub = DHL + (L > 1 ? 4 : 0);
  static constexpr int kRowStride = L * kSub;
  static constexpr int kTileFloats = T * kRowStride;
  // query side: K, V, ck, cv tiles; key side: q, g, cq tiles and
  // LSE, D, t, e of the tile's query rows
  static constexpr long kLdsQ = 4L * kTileFloats * sizeof(float);
  static constexpr long kLdsK =
      3L * kTileFloats * sizeof(float) + 4L * T * sizeof(float);
};

using VCfg2_16 = VCfg2<16, 1, 64>;
using VCfg2_32 = VCfg2<32, 1, 64>;
using VCfg2_64 = VCfg2<32, 2, 32>;
using VCfg2_128 = VCfg2<32, 4, 32>;

// Second order, thread group = query row; K, V, ck, cv tiled.  Two
// sweeps over the key tiles: the row statistics l, D, t, e first (e
// needs the finished t), then gg_i and gq_i.  A segment that fits one tile
// is staged once.
template <typename C, typename T>
__global__ __launch_bounds__(kBlock) void varlen_attn_bwd2_q_kernel(
    const T* __restrict__ Q, const T* __restrict__ K,
    const T* __restrict__ V, const float* __restrict__ LSE,
    const T* __restrict__ dO, const T* __restrict__ cQ,
    const T* __restrict__ cK, const T* __restrict__ cV,
    T* __restrict__ gQ, T* __restrict__ gdO,
    float* __restrict__ S,      // [N, H, 4]: LSE + log l, D, t, e
    const long* __restrict__ ptr, int H, int dh, float scale) {
  __shared__ __align__(16) float lK[C::kTileFloats];
  __shared__ __align__(16) float lV[C::kTileFloats];
  __shared__ __align__(16) float lCk[C::kTileFloats];
  __shared__ __align__(16) float lCv[C::kTileFloats];

  const int h = blockIdx.y;
  const long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  const int r = threadIdx.x / C::L, sub = threadIdx.x % C::L;
  const long rs = (long)H * dh;
  const bool one_tile = n <= C::T;
  bool staged = false;

  for (int q0 = blockIdx.z * C::kRows; q0 < n;
       q0 += gridDim.z * C::kRows) {
    const int q = q0 + r;
    const bool hasq = q < n;
    const long qoff = ((lo + q) * (long)H + h) * dh;
    float qv[C::DHL], gv[C::DHL], cqv[C::DHL];
    load_row<C, T>(qv, Q + qoff, sub, dh, hasq, scale);
    load_row<C, T>(gv, dO + qoff, sub, dh, hasq, 1.f);
    load_row<C, T>(cqv, cQ + qoff, sub, dh, hasq, scale);
    float lse = hasq ? LSE[(lo + q) * (long)H + h] : 0.f;
    float li = 0.f, Di = 0.f, ti = 0.f, ui = 0.f, wi = 0.f, ei = 0.f;
    float gg[C::DHL], gq[C::DHL];
#pragma unroll
    for (int d = 0; d < C::DHL; ++d) gg[d] = gq[d] = 0.f;
    for (int sweep = 0; sweep < 2; ++sweep) {
      for (int t0 = 0; t0 < n; t0 += C::T) {
        const int tn = n - t0 < C::T ? n - t0 : C::T;
        if (!(one_tile && staged)) {      // block-uniform
          const long toff = ((lo + t0) * (long)H + h) * dh;
          __syncthreads();
          stage_tile<C, T>(lK, K + toff, rs, tn, dh);
          stage_tile<C, T>(lV, V + toff, rs, tn, dh);
          stage_tile<C, T>(lCk, cK + toff, rs, tn, dh);
          stage_tile<C, T>(lCv, cV + toff, rs, tn, dh);
          __syncthreads();
          staged = true;
        }
        if (hasq) {
          // sums run per tile and the tile sums are then added up: the
          // rounding error of a long segment grows with sqrt(T) +
          // sqrt(n / T) additions instead of sqrt(n)
          float l_t = 0.f, D_t = 0.f, t_t = 0.f, u_t = 0.f, w_t = 0.f;
          float gg_t[C::DHL], gq_t[C::DHL];
#pragma unroll
          for (int d = 0; d < C::DHL; ++d) gg_t[d] = gq_t[d] = 0.f;
          for (int k = 0; k < tn; ++k) {
            const int o = k * C::kRowStride + sub * C::kSub;
            const float s = dot_row<C>(qv, lK + o);
            const float a = dot_row<C>(gv, lV + o);
            const float tt =
                dot_row<C>(cqv, lK + o) + dot_row<C>(qv, lCk + o);
            const float w = dot_row<C>(gv, lCv + o);
            const float p = expf(s - lse);
            if (sweep == 0) {
              const float pt = p * tt;
              l_t += p;
              D_t += p * a;
              t_t += pt;
              u_t += pt * a;
              w_t += p * w;
            } else {
              const float tc = tt - ti;
              const float gs = p * ((tc * a - Di * tt + w) - ei);
              const float ds = p * (a - Di);
              axpy_row<C>(gg_t, p * tc, lV + o);
              axpy_row<C>(gg_t, p, lCv + o);
              axpy_row<C>(gq_t, gs, lK + o);
              axpy_row<C>(gq_t, ds, lCk + o);
            }
          }
          if (sweep == 0) {
            li += l_t;
            Di += D_t;
            ti += t_t;
            ui += u_t;
            wi += w_t;
          } else {
#pragma unroll
            for (int d = 0; d < C::DHL; ++d) {
              gg[d] += gg_t[d];
              gq[d] += gq_t[d];
            }
          }
        }
      }
      if (sweep == 0 && hasq) {
        // li > 0: a sum of exponentials whose largest is >= 1 / n
        const float inv = 1.f / li;
        Di *= inv;
        ti *= inv;
        ui *= inv;
        wi *= inv;
        ei = ui - 2.f * ti * Di + wi;
        lse += logf(li);
      }
    }
    if (hasq) {
      store_row<C, T>(gdO + qoff, gg, sub, dh, 1.f);
      store_row<C, T>(gQ + qoff, gq, sub, dh, scale);
      if (sub == 0) {
        *reinterpret_cast<float4*>(S + ((lo + q) * (long)H + h) * 4) =
            make_float4(lse, Di, ti, ei);
      }
    }
  }
}

// Second order, thread group = key row; q, g, cq and the per-row
// statistics (LSE + log l, D, t, e) tiled:  gv_j and gk_j.
template <typename C, typename T>
__global__ __launch_bounds__(kBlock) void varlen_attn_bwd2_k_kernel(
    const T* __restrict__ Q, const T* __restrict__ K,
    const T* __restrict__ V, const float* __restrict__ S,
    const T* __restrict__ dO, const T* __restrict__ cQ,
    const T* __restrict__ cK, const T* __restrict__ cV,
    T* __restrict__ gK, T* __restrict__ gV,
    const long* __restrict__ ptr, int H, int dh, float scale) {
  __shared__ __align__(16) float lQ[C::kTileFloats];
  __shared__ __align__(16) float lG[C::kTileFloats];
  __shared__ __align__(16) float lCq[C::kTileFloats];
  __shared__ float lLse[C::T];
  __shared__ float lD[C::T];
  __shared__ float lT[C::T];
  __shared__ float lE[C::T];

  const int h = blockIdx.y;
  const long lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
  const int n = (int)(hi - lo);
  if (n <= 0) return;
  const int r = threadIdx.x / C::L, sub = threadIdx.x % C::L;
  const long rs = (long)H * dh;
  const bool one_tile = n <= C::T;
  bool staged = false;

  for (int j0 = blockIdx.z * C::kRows; j0 < n;
       j0 += gridDim.z * C::kRows) {
    const int j = j0 + r;
    const bool hask = j < n;
    const long koff = ((lo + j) * (long)H + h) * dh;
    float kv[C::DHL], vv[C::DHL], ckv[C::DHL], cvv[C::DHL];
    float gk[C::DHL], gvv[C::DHL];
    load_row<C, T>(kv, K + koff, sub, dh, hask, scale);
    load_row<C, T>(vv, V + koff, sub, dh, hask, 1.f);
    load_row<C, T>(ckv, cK + koff, sub, dh, hask, scale);
    load_row<C, T>(cvv, cV + koff, sub, dh, hask, 1.f);
#pragma unroll
    for (int d = 0; d < C::DHL; ++d) gk[d] = gvv[d] = 0.f;
    for (int t0 = 0; t0 < n; t0 += C::T) {
      const int tn = n - t0 < C::T ? n - t0 : C::T;
      if (!(one_tile && staged)) {        // block-uniform
        const long toff = ((lo + t0) * (long)H + h) * dh;
        __syncthreads();
        stage_tile<C, T>(lQ, Q + toff, rs, tn, dh);
        stage_tile<C, T>(lG, dO + toff, rs, tn, dh);
        stage_tile<C, T>(lCq, cQ + toff, rs, tn, dh);
        for (int i = threadIdx.x; i < tn; i += kBlock) {
          const float4 st = *reinterpret_cast<const float4*>(
              S + ((lo + t0 + i) * (long)H + h) * 4);
          lLse[i] = st.x;
          lD[i] = st.y;
          lT[i] = st.z;
          lE[i] = st.w;
        }
        __syncthreads();
        staged = true;
      }
      if (hask) {
        float gk_t[C::DHL], gv_t[C::DHL];   // per-tile sums, as above
#pragma unroll
        for (int d = 0; d < C::DHL; ++d) gk_t[d] = gv_t[d] = 0.f;
        for (int i = 0; i < tn; ++i) {
          const int o = i * C::kRowStride + sub * C::kSub;
          const float s = dot_row<C>(kv, lQ + o);
          const float a = dot_row<C>(vv, lG + o);
          const float tt =
              dot_row<C>(kv, lCq + o) + dot_row<C>(ckv, lQ + o);
          const float w = dot_row<C>(cvv, lG + o);
          const float p = expf(s - lLse[i]);
          const float Di = lD[i];
          const float tc = tt - lT[i];
          const float gs = p * ((tc * a - Di * tt + w) - lE[i]);
          const float ds = p * (a - Di);
          axpy_row<C>(gv_t, p * tc, lG + o);
          axpy_row<C>(gk_t, gs, lQ + o);
          axpy_row<C>(gk_t, ds, lCq + o);
        }
#pragma unroll
        for (int d = 0; d < C::DHL; ++d) {
          gk[d] += gk_t[d];
          gvv[d] += gv_t[d];
        }
      }
    }
    if (hask) {
      store_row<C, T>(gV + koff, gvv, sub, dh, 1.f);
      store_row<C, T>(gK + koff, gk, sub, dh, scale);
    }
  }
}

// Calls f(VCfg instance) for the narrowest instance that holds dh.
template <typename F>
void with_instance(long dh, F&& f) {
  TORCH_CHECK(dh >= 1 && dh <= VCfg128::kCap,
              "varlen attention: head_dim must be in [1, 128]");
  if (dh <= VCfg16::kCap) f(VCfg16{});
  else if (dh <= VCfg32::kCap) f(VCfg32{});
  else if (dh <= VCfg64::kCap) f(VCfg64{});
  else f(VCfg128{});
}

// The same for the second-order instances.
template <typename F>
void with_instance2(long dh, F&& f) {
  TORCH_CHECK(dh >= 1 && dh <= VCfg2_128::kCap,
              "varlen attention: head_dim must be in [1, 128]");
  if (dh <= VCfg2_16::kCap) f(VCfg2_16{});
  else if (dh <= VCfg2_32::kCap) f(VCfg2_32{});
  else if (dh <= VCfg2_64::kCap) f(VCfg2_64{});
  else f(VCfg2_128{});
}

void check_qkv(const torch::Tensor& Q, const torch::Tensor& K,
               const torch::Tensor& V, const torch::Tensor& ptr) {
  TORCH_CHECK(Q.is_cuda() && K.is_cuda() && V.is_cuda() && ptr.is_cuda());
  TORCH_CHECK(Q.dim() == 3 && K.sizes() == Q.sizes() &&
              V.sizes() == Q.sizes());
  TORCH_CHECK(Q.is_contiguous() && K.is_contiguous() && V.is_contiguous());
  TORCH_CHECK(Q.scalar_type() == at::ScalarType::Float ||
              Q.scalar_type() == at::ScalarType::BFloat16,
              "varlen attention expects fp32 or bf16 q/k/v");
  TORCH_CHECK(K.scalar_type() == Q.scalar_type() &&
              V.scalar_type() == Q.scalar_type());
  TORCH_CHECK(ptr.scalar_type() == at::ScalarType::Long &&
              ptr.dim() == 1 && ptr.numel() >= 1);
}

template <typename T>
const T* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}
template <typename T>
T* mptr(torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

// Workgroups per (graph, head).  Segment lengths live on the device,
// so the split follows the mean length N / G, which the shapes give
// without a sync: 1.5 mean-length's worth of row chunks, at most 8.
// Each row is computed by one thread in one fixed order whatever the
// split, so it does not change a single bit of the result.
inline unsigned row_split(long N, long G, long rows) {
  long z = (3 * N + 2 * G * rows - 1) / (2 * G * rows);
  return (unsigned)std::min<long>(std::max<long>(z, 1), 8);
}

template <typename T>
void launch_fwd(const torch::Tensor& Q, const torch::Tensor& K,
                const torch::Tensor& V, torch::Tensor& O,
                torch::Tensor& LSE, const torch::Tensor& ptr) {
  const int H = Q.size(1), dh = Q.size(2);
  const long G = ptr.numel() - 1;
  const float scale = 1.0f / std::sqrt((float)dh);
  auto stream = at::hip::getCurrentHIPStream().stream();
  with_instance(dh, [&](auto c) {
    using C = decltype(c);
    const dim3 grid(G, H, row_split(Q.size(0), G, C::kRows));
    hipLaunchKernelGGL((varlen_attn_fwd_kernel<C, T>), grid,
                       dim3(kBlock), 0, stream, cptr<T>(Q), cptr<T>(K),
                       cptr<T>(V), mptr<T>(O), LSE.data_ptr<float>(),
                       ptr.data_ptr<long>(), H, dh, scale);
  });
  check_launch("varlen_attention_fwd");
}

template <typename T>
void launch_bwd(const torch::Tensor& Q, const torch::Tensor& K,
                const torch::Tensor& V, const torch::Tensor& O,
                const torch::Tensor& LSE, const torch::Tensor& dO,
                torch::Tensor& dQ, torch::Tensor& dK, torch::Tensor& dV,
                torch::Tensor& D, const torch::Tensor& ptr) {
  const int H = Q.size(1), dh = Q.size(2);
  const long G = ptr.numel() - 1;
  const float scale = 1.0f / std::sqrt((float)dh);
  auto stream = at::hip::getCurrentHIPStream().stream();
  with_instance(dh, [&](auto c) {
    using C = decltype(c);
    const dim3 grid(G, H, row_split(Q.size(0), G, C::kRows));
    hipLaunchKernelGGL((varlen_attn_dq_kernel<C, T>), grid,
                       dim3(kBlock), 0, stream, cptr<T>(Q), cptr<T>(K),
                       cptr<T>(V), cptr<T>(O), LSE.data_ptr<float>(),
                       cptr<T>(dO), mptr<T>(dQ), D.data_ptr<float>(),
                       ptr.data_ptr<long>(), H, dh, scale);
    check_launch("varlen_attention_bwd (dQ pass)");
    // same stream: D is complete before this pass reads it
    hipLaunchKernelGGL((varlen_attn_dkv_kernel<C, T>), grid,
                       dim3(kBlock), 0, stream, cptr<T>(Q), cptr<T>(K),
                       cptr<T>(V), LSE.data_ptr<float>(),
                       D.data_ptr<float>(), cptr<T>(dO), mptr<T>(dK),
                       mptr<T>(dV), ptr.data_ptr<long>(), H, dh, scale);
    check_launch("varlen_attention_bwd (dK/dV pass)");
  });
}

template <typename T>
void launch_bwd2(const torch::Tensor& Q, const torch::Tensor& K,
                 const torch::Tensor& V, const torch::Tensor& LSE,
                 const torch::Tensor& dO, const torch::Tensor& cQ, const torch::Tensor& cK,
                 const torch::Tensor& cV, torch::Tensor& gQ,
                 torch::Tensor& gK, torch::Tensor& gV, torch::Tensor& gdO,
                 torch::Tensor& S, const torch::Tensor& ptr) {
  const int H = Q.size(1), dh = Q.size(2);
  const long G = ptr.numel() - 1;
  const float scale = 1.0f / std::sqrt((float)dh);
  auto stream = at::hip::getCurrentHIPStream().stream();
  with_instance2(dh, [&](auto c) {
    using C = decltype(c);
    const dim3 grid(G, H, row_split(Q.size(0), G, C::kRows));
    hipLaunchKernelGGL((varlen_attn_bwd2_q_kernel<C, T>), grid,
                       dim3(kBlock), 0, stream, cptr<T>(Q), cptr<T>(K),
                       cptr<T>(V), LSE.data_ptr<float>(), cptr<T>(dO),
                       cptr<T>(cQ), cptr<T>(cK), cptr<T>(cV),
                       mptr<T>(gQ), mptr<T>(gdO), S.data_ptr<float>(),
                       ptr.data_ptr<long>(), H, dh, scale);
    check_launch("varlen_attention_bwd2 (query pass)");
    // same stream: the row statistics are complete before this pass
    hipLaunchKernelGGL((varlen_attn_bwd2_k_kernel<C, T>), grid,
                       dim3(kBlock), 0, stream, cptr<T>(Q), cptr<T>(K),
                       cptr<T>(V), S.data_ptr<float>(), cptr<T>(dO),
                       cptr<T>(cQ), cptr<T>(cK), cptr<T>(cV), mptr<T>(gK),
                       mptr<T>(gV), ptr.data_ptr<long>(), H, dh, scale);
    check_launch("varlen_attention_bwd2 (key pass)");
  });
}

}  // namespace

// LDS bytes (static; these kernels use no dynamic LDS) of the instance
// that serves head_dim dh.  pass: 0 forward, 1 dQ, 2 dK/dV, 3 and 4
// the query and key pass of the second order.
long varlen_attention_lds_bytes(long dh, long pass) {
  TORCH_CHECK(pass >= 0 && pass <= 4, "pass must be in [0, 4]");
  long bytes = 0;
  if (pass >= 3) {
    with_instance2(dh, [&](auto c) {
      using C = decltype(c);
      bytes = pass == 3 ? C::kLdsQ : C::kLdsK;
    });
    return bytes;
  }
  with_instance(dh, [&](auto c) {
    using C = decltype(c);
    bytes = pass == 0 ? C::kLdsFwd : pass == 1 ? C::kLdsDq : C::kLdsDkv;
  });
  return bytes;
}

// {tile rows T, rows per workgroup pass B} of the instance serving dh.
std::vector<long> varlen_attention_tiling(long dh) {
  std::vector<long> out;
  with_instance(dh, [&](auto c) {
    using C = decltype(c);
    out = {C::T, C::kRows};
  });
  return out;
}

// The same for the second-order instance serving dh.
std::vector<long> varlen_attention_tiling2(long dh) {
  std::vector<long> out;
  with_instance2(dh, [&](auto c) {
    using C = decltype(c);
    out = {C::T, C::kRows};
  });
  return out;
}

std::vector<torch::Tensor> varlen_attention_fwd(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V,
    torch::Tensor ptr) {
  check_qkv(Q, K, V, ptr);
  const long N = Q.size(0), H = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(H >= 1 && H <= 65535, "head count must be in [1, 65535]");
  TORCH_CHECK(varlen_attention_lds_bytes(dh, 0) <= kLdsBudget,
              "varlen_attention_fwd: LDS over 160 KiB");
  auto O = torch::empty_like(Q);
  auto LSE = torch::empty({N, H}, Q.options().dtype(torch::kFloat));
  if (N == 0 || ptr.numel() == 1) return {O, LSE};
  auto p = ptr.contiguous();
  if (Q.scalar_type() == at::ScalarType::Float)
    launch_fwd<float>(Q, K, V, O, LSE, p);
  else
    launch_fwd<__hip_bfloat16>(Q, K, V, O, LSE, p);
  return {O, LSE};
}

std::vector<torch::Tensor> varlen_attention_bwd(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V, torch::Tensor O,
    torch::Tensor LSE, torch::Tensor dO, torch::Tensor ptr) {
  check_qkv(Q, K, V, ptr);
  const long N = Q.size(0), H = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(H >= 1 && H <= 65535, "head count must be in [1, 65535]");
  for (const torch::Tensor* t : {&O, &dO})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->sizes() == Q.sizes() &&
                t->scalar_type() == Q.scalar_type(),
                "varlen_attention_bwd: O and dO must match q");
  TORCH_CHECK(LSE.is_cuda() && LSE.is_contiguous() &&
              LSE.scalar_type() == at::ScalarType::Float &&
              LSE.dim() == 2 && LSE.size(0) == N && LSE.size(1) == H,
              "varlen_attention_bwd: LSE must be [N, H] fp32");
  TORCH_CHECK(varlen_attention_lds_bytes(dh, 1) <= kLdsBudget &&
              varlen_attention_lds_bytes(dh, 2) <= kLdsBudget,
              "varlen_attention_bwd: LDS over 160 KiB");
  auto dQ = torch::empty_like(Q);
  auto dK = torch::empty_like(Q);
  auto dV = torch::empty_like(Q);
  if (N == 0 || ptr.numel() == 1) return {dQ, dK, dV};
  auto D = torch::empty_like(LSE);
  auto p = ptr.contiguous();
  if (Q.scalar_type() == at::ScalarType::Float)
    launch_bwd<float>(Q, K, V, O, LSE, dO, dQ, dK, dV, D, p);
  else
    launch_bwd<__hip_bfloat16>(Q, K, V, O, LSE, dO, dQ, dK, dV, D, p);
  return {dQ, dK, dV};
}

// Second order: gradients of <cQ,dQ> + <cK,dK> + <cV,dV> with respect
// to (Q, K, V, dO), in the input dtype.  Every cotangent is a tensor;
// the caller passes zeros for one that autograd did not supply.  O is
// checked like the first order's but not read (see the kernels).
std::vector<torch::Tensor> varlen_attention_bwd2(
    torch::Tensor Q, torch::Tensor K, torch::Tensor V, torch::Tensor O,
    torch::Tensor LSE, torch::Tensor dO, torch::Tensor cQ,
    torch::Tensor cK, torch::Tensor cV, torch::Tensor ptr) {
  check_qkv(Q, K, V, ptr);
  const long N = Q.size(0), H = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(H >= 1 && H <= 65535, "head count must be in [1, 65535]");
  for (const torch::Tensor* t : {&O, &dO, &cQ, &cK, &cV})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->sizes() == Q.sizes() &&
                t->scalar_type() == Q.scalar_type(),
                "varlen_attention_bwd2: O, dO, cQ, cK, cV must match q");
  TORCH_CHECK(LSE.is_cuda() && LSE.is_contiguous() &&
              LSE.scalar_type() == at::ScalarType::Float &&
              LSE.dim() == 2 && LSE.size(0) == N && LSE.size(1) == H,
              "varlen_attention_bwd2: LSE must be [N, H] fp32");
  TORCH_CHECK(varlen_attention_lds_bytes(dh, 3) <= kLdsBudget &&
              varlen_attention_lds_bytes(dh, 4) <= kLdsBudget,
              "varlen_attention_bwd2: LDS over 160 KiB");
  auto gQ = torch::empty_like(Q);
  auto gK = torch::empty_like(Q);
  auto gV = torch::empty_like(Q);
  auto gdO = torch::empty_like(Q);
  if (N == 0 || ptr.numel() == 1) return {gQ, gK, gV, gdO};
  auto S = torch::empty({N, H, 4}, Q.options().dtype(torch::kFloat));
  auto p = ptr.contiguous();
  if (Q.scalar_type() == at::ScalarType::Float)
    launch_bwd2<float>(Q, K, V, LSE, dO, cQ, cK, cV, gQ, gK, gV, gdO,
                       S, p);
  else
    launch_bwd2<__hip_bfloat16>(Q, K, V, LSE, dO, cQ, cK, cV, gQ, gK,
                                gV, gdO, S, p);
  return {gQ, gK, gV, gdO};
}

torch::Tensor varlen_attention(torch::Tensor Q, torch::Tensor K,
                               torch::Tensor V, torch::Tensor ptr) {
  TORCH_CHECK(Q.is_cuda() && Q.is_contiguous());
  TORCH_CHECK(Q.scalar_type() == at::ScalarType::Float ||
              Q.scalar_type() == at::ScalarType::BFloat16,
              "varlen_attention expects fp32 or bf16 q/k/v");
  TORCH_CHECK(K.scalar_type() == Q.scalar_type() &&
              V.scalar_type() == Q.scalar_type());
  long N = Q.size(0);
  int H = Q.size(1), dh = Q.size(2);
  TORCH_CHECK(dh <= kMaxDh, "head_dim must be <= 64");
  long G = ptr.numel() - 1;
  auto O = torch::empty_like(Q);
  if (N == 0 || G == 0) return O;
  float scale = 1.0f / std::sqrt((float)dh);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto p = ptr.contiguous();
  if (Q.scalar_type() == at::ScalarType::Float) {
    hipLaunchKernelGGL((varlen_attn_kernel<float>), dim3(G, H),
                       dim3(kThreads), 0, stream, Q.data_ptr<float>(),
                       K.data_ptr<float>(), V.data_ptr<float>(),
                       O.data_ptr<float>(), p.data_ptr<long>(), H, dh,
                       scale);
  } else {
    hipLaunchKernelGGL((varlen_attn_kernel<__hip_bfloat16>), dim3(G, H),
                       dim3(kThreads), 0, stream,
                       reinterpret_cast<const __hip_bfloat16*>(Q.data_ptr()),
                       reinterpret_cast<const __hip_bfloat16*>(K.data_ptr()),
                       reinterpret_cast<const __hip_bfloat16*>(V.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(O.data_ptr()),
                       p.data_ptr<long>(), H, dh, scale);
  }
  return O;
}
