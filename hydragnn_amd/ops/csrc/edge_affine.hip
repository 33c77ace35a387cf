// Pair-affine edge layer for MI355X (gfx950, CDNA4): the first layer of
// EGNN's edge MLP without the [E, 2F + 1 + D] concatenation, and the
// three kernels that close it under differentiation.
//
//   P[N, 2H] node-side projections (dst half | src half), r2[E],
//   ea[E, D], w_r[H], W_e as its transpose weT[D, H], b[H];
//   i = didx[e] the destination and j = sidx[e] the source of edge e.
//
//   fwd   : z[e, f]  = P[i, f] + P[j, H + f] + r2[e] w_r[f]
//                      + sum_k ea[e, k] weT[k, f] + b[f]
//   node  : dP[i, f]     = sum_{e -> i} g[e, f]
//           dP[j, H + f] = sum_{e <- j} g[e, f]
//   edge  : dr2[e]    = sum_f g[e, f] w_r[f]
//           dea[e, k] = sum_f g[e, f] weT[k, f]
//   param : dw_r[f]    = sum_e r2[e] g[e, f]
//           dW_e[f, k] = sum_e ea[e, k] g[e, f]
//           db[f]      = sum_e g[e, f]
//
// Every operand group of fwd may be absent (a null pointer): it then
// contributes nothing and loads nothing.  The gradients of node, edge
// and param are fwd again with some groups absent, so all orders of
// differentiation stay on these kernels (ops/edge_affine.py).
//
// fwd and edge give an edge to L adjacent lanes, L the least power of
// two >= the number of feature packs (at most 64; lanes loop beyond).
// In fwd a lane keeps its pack while the block grid-strides over tiles
// of 256 / L edges, so its packs of w_r, b and weT stay in registers;
// the tile's r2 and ea rows, which are narrow, unaligned and shared by
// the lanes of an edge, are loaded coalesced into LDS once per tile and
// read from there as broadcasts.  The two rows of P are gathered as
// packs.  edge reduces over the lanes of a group with __shfl_xor and
// its first lane stores the 1 + D results.  node maps one thread to one
// (node, pack of the 2H row): the first half walks the CSR of the
// destinations, the second half that of the sources, in ascending edge
// id with four positions loaded ahead of their ordered adds.  param
// cuts E into chunks; a block owns a (chunk, feature tile), a thread a
// feature and, where the tile is narrower than the block, one of the
// 256 / tile interleaved slices of the chunk's edges; the slices are
// added in slice order through LDS, the chunks by a second kernel in
// chunk order.  No atomics and no zero fill: every output element has
// one writer and a fixed order.
//
// All sums run in the accumulator type (fp32 for bf16/f16); every
// product is rounded to it before it is added (contraction is off for
// the file, and packed fp32 arithmetic is kept out of it); results are
// rounded once.  A pack is 16 bytes (VEC = 16 / sizeof(T)) when
// H * sizeof(T) is a multiple of 16 and every feature operand starts on
// 16 bytes, and one element otherwise.

#include <torch/extension.h>
#include <ATen/OpMathType.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "segment_common.h"

namespace {

using namespace segment;

constexpr int kMaxD = 16;
constexpr int kAhead = 4;        // node: positions loaded ahead of the adds
constexpr int kMaxChunks = 512;  // param: chunks of E
constexpr int kChunkUnit = 256;  // param: fewest edges worth a chunk

// no fused multiply-add anywhere below: a product is rounded, then added
#pragma clang fp contract(off)

// no packed fp32 arithmetic in the device code of this file, as in
// painn_message.hip: the bit-exact contract rests on plain IEEE
// products and sums, and these kernels wait on their loads
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The block's tile of r2 (n rows from row0) and ea (n rows of D) into
// LDS, coalesced; rows past E read as 0.  Either source may be null.
template <typename T, typename ACC>
__device__ __forceinline__ void load_tile(
    const T* __restrict__ r2, const T* __restrict__ ea, ACC* s_r, ACC* s_e,
    long row0, int n, long E, int D) {
  if (r2) {
    for (int i = threadIdx.x; i < n; i += kBlock)
      s_r[i] = row0 + i < E ? ld1<ACC>(r2, row0 + i) : (ACC)0;
  }
  if (ea) {
    const long base = row0 * D, end = E * D;
    for (int i = threadIdx.x; i < n * D; i += kBlock)
      s_e[i] = base + i < end ? ld1<ACC>(ea, base + i) : (ACC)0;
  }
}

// ---------------------------------------------------------------------------
// fwd
// ---------------------------------------------------------------------------
// L lanes per edge, L a power of two <= 64 that divides the block; the
// loops over feature rounds and over tiles are uniform in the block, so
// every thread reaches every barrier.  DMAX bounds D at compile time:
// the weT packs are registers, never an indexed array.
template <typename T, typename ACC, int VEC, int DMAX>
__global__ void __launch_bounds__(kBlock) pair_affine_fwd_kernel(
    const T* __restrict__ P, const T* __restrict__ r2,
    const T* __restrict__ ea, const T* __restrict__ wr,
    const T* __restrict__ weT, const T* __restrict__ b,
    const long* __restrict__ didx, const long* __restrict__ sidx,
    T* __restrict__ z, long E, long Fp, int D, int L) {
  using Pk = Pack<T, VEC>;
  extern __shared__ __align__(16) unsigned char pair_affine_lds[];
  const int G = kBlock / L;                 // edges of a tile
  ACC* s_r = reinterpret_cast<ACC*>(pair_affine_lds);
  ACC* s_e = s_r + G;
  const Pk* __restrict__ Pp = reinterpret_cast<const Pk*>(P);
  const Pk* __restrict__ wrp = reinterpret_cast<const Pk*>(wr);
  const Pk* __restrict__ wep = reinterpret_cast<const Pk*>(weT);
  const Pk* __restrict__ bp = reinterpret_cast<const Pk*>(b);
  Pk* __restrict__ zp = reinterpret_cast<Pk*>(z);
  const int lane = (int)(threadIdx.x & (L - 1));
  const int grp = (int)(threadIdx.x / L);
  const long n_tiles = (E + G - 1) / G;
  for (long fb = 0; fb < Fp; fb += L) {
    const long f = fb + lane;
    const bool live = f < Fp;
    Pk wrv = {}, bv = {}, wev[DMAX];
    if (live) {
      if (r2) wrv = wrp[f];
      if (b) bv = bp[f];
#pragma unroll
      for (int k = 0; k < DMAX; ++k)
        if (ea && k < D) wev[k] = wep[k * Fp + f];
    }
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
      load_tile<T, ACC>(r2, ea, s_r, s_e, t * G, G, E, D);
      __syncthreads();
      const long e = t * G + grp;
      if (live && e < E) {
        ACC acc[VEC];
        if (P) {
          const Pk pi = Pp[didx[e] * 2 * Fp + f];
          const Pk pj = Pp[(sidx[e] * 2 + 1) * Fp + f];
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = ld<ACC>(pi, v) + ld<ACC>(pj, v);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = (ACC)0;
        }
        if (r2) {
          const ACC r = s_r[grp];
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += mul_rn(r, ld<ACC>(wrv, v));
        }
        if (ea) {
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            if (k < D) {
              const ACC a = s_e[grp * D + k];
#pragma unroll
              for (int v = 0; v < VEC; ++v)
                acc[v] += mul_rn(a, ld<ACC>(wev[k], v));
            }
          }
        }
        if (b) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += ld<ACC>(bv, v);
        }
        Pk out;
#pragma unroll
        for (int v = 0; v < VEC; ++v) st(out, v, acc[v]);
        zp[e * Fp + f] = out;
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------
// node
// ---------------------------------------------------------------------------
template <typename T, typename ACC, int VEC>
__global__ void __launch_bounds__(kBlock) pair_affine_node_kernel(
    const T* __restrict__ g, const long* __restrict__ d_rowptr,
    const long* __restrict__ d_perm, const long* __restrict__ s_rowptr,
    const long* __restrict__ s_perm, T* __restrict__ dP, long N, long Fp) {
  using Pk = Pack<T, VEC>;
  const Pk* __restrict__ gp = reinterpret_cast<const Pk*>(g);
  Pk* __restrict__ op = reinterpret_cast<Pk*>(dP);
  const long total = N * 2 * Fp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / (2 * Fp);
    const long c = i - n * 2 * Fp;
    const bool second = c >= Fp;                 // the src half of the row
    const long f = second ? c - Fp : c;
    const long* __restrict__ rowptr = second ? s_rowptr : d_rowptr;
    const long* __restrict__ perm = second ? s_perm : d_perm;
    const long lo = rowptr[n], hi = rowptr[n + 1];
    ACC acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = (ACC)0;
    long p = lo;
    for (; p + kAhead <= hi; p += kAhead) {
      Pk gv[kAhead];
#pragma unroll
      for (int a = 0; a < kAhead; ++a) {
        const long e = perm ? perm[p + a] : p + a;
        gv[a] = gp[e * Fp + f];
      }
#pragma unroll
      for (int a = 0; a < kAhead; ++a)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += ld<ACC>(gv[a], v);
    }
    for (; p < hi; ++p) {
      const long e = perm ? perm[p] : p;
      const Pk gv = gp[e * Fp + f];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += ld<ACC>(gv, v);
    }
    Pk out;
#pragma unroll
    for (int v = 0; v < VEC; ++v) st(out, v, acc[v]);
    op[i] = out;
  }
}

// ---------------------------------------------------------------------------
// edge
// ---------------------------------------------------------------------------
// dr2 is computed when it is not null, dea when D > 0.  The parameter
// packs are read where they are used: (1 + D) H values that every edge
// shares stay in cache, and holding them would cost the registers of
// the 1 + D running sums.
template <typename T, typename ACC, int VEC, int DMAX>
__global__ void __launch_bounds__(kBlock) pair_affine_edge_kernel(
    const T* __restrict__ g, const T* __restrict__ wr,
    const T* __restrict__ weT, T* __restrict__ dr2, T* __restrict__ dea,
    long E, long Fp, int D, int L) {
  using Pk = Pack<T, VEC>;
  const Pk* __restrict__ gp = reinterpret_cast<const Pk*>(g);
  const Pk* __restrict__ wrp = reinterpret_cast<const Pk*>(wr);
  const Pk* __restrict__ wep = reinterpret_cast<const Pk*>(weT);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & (L - 1));
  const long step = (long)gridDim.x * blockDim.x / L;
  for (long e = tid / L; e < E; e += step) {
    ACC sr = (ACC)0, se[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) se[k] = (ACC)0;
    for (long f = lane; f < Fp; f += L) {
      const Pk gv = gp[e * Fp + f];
      if (dr2) {
        const Pk w = wrp[f];
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          sr += mul_rn(ld<ACC>(gv, v), ld<ACC>(w, v));
      }
#pragma unroll
      for (int k = 0; k < DMAX; ++k) {
        if (k < D) {
          const Pk w = wep[k * Fp + f];
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            se[k] += mul_rn(ld<ACC>(gv, v), ld<ACC>(w, v));
        }
      }
    }
    // lanes past Fp hold 0; after log2 L steps every lane of the group
    // holds the same sums
    for (int m = L >> 1; m > 0; m >>= 1) {
      if (dr2) sr += __shfl_xor(sr, m, L);
#pragma unroll
      for (int k = 0; k < DMAX; ++k)
        if (k < D) se[k] += __shfl_xor(se[k], m, L);
    }
    if (lane == 0) {
      if (dr2) st1(dr2, e, sr);
#pragma unroll
      for (int k = 0; k < DMAX; ++k)
        if (k < D) st1(dea, e * D + k, se[k]);
    }
  }
}

// ---------------------------------------------------------------------------
// param
// ---------------------------------------------------------------------------
// partial[chunk, 2 + D, H] in the accumulator type: slot 0 is dw_r,
// slots 1 .. D the columns of dW_e, slot 1 + D is db.  FT, the width of
// a feature tile, is a power of two <= 64; S = 256 / FT slices share a
// chunk, slice s taking the edges s, s + S, ... of every tile of 256.
// The loops over blocks' work items and over tiles are uniform in the
// block.  LDS holds the tile (256 (1 + D) values) and is reused for the
// 256 (2 + D) values of the slices' sums.
template <typename T, typename ACC, int DMAX>
__global__ void __launch_bounds__(kBlock) pair_affine_param_kernel(
    const T* __restrict__ g, const T* __restrict__ r2,
    const T* __restrict__ ea, ACC* __restrict__ partial, long E, long H,
    int D, int FT, long chunk_len, long n_chunks, long n_ftiles) {
  extern __shared__ __align__(16) unsigned char pair_affine_lds[];
  ACC* s_r = reinterpret_cast<ACC*>(pair_affine_lds);
  ACC* s_e = s_r + kBlock;
  ACC* s_sum = s_r;                          // [2 + D][S][FT], after the walk
  const int S = kBlock / FT;
  const int s = (int)(threadIdx.x / FT);
  const int fl = (int)(threadIdx.x & (FT - 1));
  const int slots = 2 + D;
  for (long item = blockIdx.x; item < n_chunks * n_ftiles;
       item += gridDim.x) {
    const long chunk = item / n_ftiles;
    const long f = (item - chunk * n_ftiles) * FT + fl;
    const bool live = f < H;
    const long lo = chunk * chunk_len;
    const long hi = lo + chunk_len < E ? lo + chunk_len : E;
    ACC ar = (ACC)0, ab = (ACC)0, ae[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) ae[k] = (ACC)0;
    for (long e0 = lo; e0 < hi; e0 += kBlock) {
      const int n = (int)(hi - e0 < kBlock ? hi - e0 : kBlock);
      load_tile<T, ACC>(r2, ea, s_r, s_e, e0, n, hi, D);
      __syncthreads();
      if (live) {
#pragma unroll 4
        for (int i = s; i < n; i += S) {
          const ACC gv = ld1<ACC>(g, (e0 + i) * H + f);
          ab += gv;
          if (r2) ar += mul_rn(s_r[i], gv);
          if (ea) {
#pragma unroll
            for (int k = 0; k < DMAX; ++k)
              if (k < D) ae[k] += mul_rn(s_e[i * D + k], gv);
          }
        }
      }
      __syncthreads();
    }
    s_sum[(0 * S + s) * FT + fl] = ar;
#pragma unroll
    for (int k = 0; k < DMAX; ++k)
      if (k < D) s_sum[((1 + k) * S + s) * FT + fl] = ae[k];
    s_sum[((1 + D) * S + s) * FT + fl] = ab;
    __syncthreads();
    for (int q = threadIdx.x; q < slots * FT; q += kBlock) {
      const int slot = q / FT, ql = q - slot * FT;
      const long qf = (item - chunk * n_ftiles) * FT + ql;
      ACC tot = s_sum[(slot * S + 0) * FT + ql];
      for (int t = 1; t < S; ++t) tot += s_sum[(slot * S + t) * FT + ql];
      if (qf < H) partial[(chunk * slots + slot) * H + qf] = tot;
    }
    __syncthreads();
  }
}

// dw_r, dW_e[H, D] and db from the partials, chunks in ascending order;
// a null output is skipped
template <typename T, typename ACC>
__global__ void __launch_bounds__(kBlock) pair_affine_param_reduce_kernel(
    const ACC* __restrict__ partial, T* __restrict__ dwr,
    T* __restrict__ dWe, T* __restrict__ db, long H, int D, long n_chunks) {
  const int slots = 2 + D;
  const long total = (long)slots * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int slot = (int)(i / H);
    const long f = i - (long)slot * H;
    T* out = slot == 0 ? dwr : (slot == 1 + D ? db : dWe);
    if (!out) continue;
    ACC tot = partial[(long)slot * H + f];
    for (long c = 1; c < n_chunks; ++c)
      tot += partial[(c * slots + slot) * H + f];
    const long at = (slot == 0 || slot == 1 + D) ? f : f * D + (slot - 1);
    st1(out, at, tot);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using OptTensor = c10::optional<torch::Tensor>;

// a null pointer for an absent operand; a present one must be a
// contiguous GPU tensor of `dtype` with `numel` elements
const void* operand(const OptTensor& t, at::ScalarType dtype, long numel,
                    const char* what) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                  t->scalar_type() == dtype && t->numel() == numel,
              "pair_affine: ", what, " must be a contiguous GPU tensor of ",
              numel, " elements of the common dtype");
  return t->data_ptr();
}

void check_sizes(long E, long H, long D) {
  TORCH_CHECK(E >= 0 && E < (1L << 31), "pair_affine: E must be below 2^31");
  TORCH_CHECK(H >= 0, "pair_affine: H must not be negative");
  TORCH_CHECK(D >= 0 && D <= kMaxD, "pair_affine: D must be in [0, ",
              kMaxD, "]");
}

}  // namespace

// z[E, H]; P[N, 2H], r2[E] with w_r[H], ea[E, D] with weT[D, H] and b[H]
// may each be absent; didx and sidx are needed with P
torch::Tensor pair_affine_fwd(OptTensor P, OptTensor r2, OptTensor ea,
                              OptTensor wr, OptTensor weT, OptTensor b,
                              OptTensor didx, OptTensor sidx, long E, long H,
                              torch::Tensor like) {
  const long D = ea.has_value() ? ea->size(-1) : 0;
  check_sizes(E, H, D);
  TORCH_CHECK(r2.has_value() == wr.has_value() &&
                  ea.has_value() == weT.has_value(),
              "pair_affine_fwd: r2 goes with w_r and ea with W_e");
  TORCH_CHECK(like.is_cuda(), "pair_affine_fwd: GPU tensors only");
  const auto dtype = like.scalar_type();
  long N = 0;
  if (P.has_value()) {
    TORCH_CHECK(P->dim() == 2 && P->size(1) == 2 * H,
                "pair_affine_fwd: P must be [N, 2H]");
    TORCH_CHECK(didx.has_value() && sidx.has_value(),
                "pair_affine_fwd: P needs both indices");
    N = P->size(0);
  }
  const void* Pv = operand(P, dtype, N * 2 * H, "P");
  const void* rv = operand(r2, dtype, E, "r2");
  const void* ev = operand(ea, dtype, E * D, "ea");
  const void* wv = operand(wr, dtype, H, "w_r");
  const void* tv = operand(weT, dtype, D * H, "W_e^T");
  const void* bv = operand(b, dtype, H, "b");
  torch::Tensor dk, sk;
  const long* dp =
      P.has_value() ? index_ptr(didx, E, dk, "pair_affine: dst") : nullptr;
  const long* sp =
      P.has_value() ? index_ptr(sidx, E, sk, "pair_affine: src") : nullptr;
  if (E * H == 0 || (P.has_value() && N == 0) ||
      !(Pv || rv || (ev && D > 0) || bv))
    return torch::zeros({E, H}, like.options());
  if (D == 0) ev = tv = nullptr;
  auto z = torch::empty({E, H}, like.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, dtype,
      "pair_affine_fwd", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        constexpr int kVec = 16 / sizeof(scalar_t);
        scalar_t* zp = z.data_ptr<scalar_t>();
        const bool packed =
            H % kVec == 0 && all_aligned16(Pv, wv, tv, bv, zp);
        auto launch = [&](auto kernel, long Fp) {
          const int L = pow2_at_least(Fp, 64);
          const int G = kBlock / L;
          const long tiles = (E + G - 1) / G;
          const size_t lds = (size_t)G * (1 + D) * sizeof(acc_t);
          hipLaunchKernelGGL(
              kernel, dim3((unsigned)std::min<long>(tiles, kGridCap)),
              dim3(kBlock), lds, stream, (const scalar_t*)Pv,
              (const scalar_t*)rv, (const scalar_t*)ev, (const scalar_t*)wv,
              (const scalar_t*)tv, (const scalar_t*)bv, dp, sp, zp, E, Fp,
              (int)D, L);
        };
        if (packed && D <= 4)
          launch(pair_affine_fwd_kernel<scalar_t, acc_t, kVec, 4>, H / kVec);
        else if (packed)
          launch(pair_affine_fwd_kernel<scalar_t, acc_t, kVec, kMaxD>,
                 H / kVec);
        else if (D <= 4)
          launch(pair_affine_fwd_kernel<scalar_t, acc_t, 1, 4>, H);
        else
          launch(pair_affine_fwd_kernel<scalar_t, acc_t, 1, kMaxD>, H);
        check_launch("pair_affine_fwd_kernel");
      });
  return z;
}

// dP[N, 2H] from g[E, H] over the CSRs of the destinations (first half)
// and of the sources (second half)
torch::Tensor pair_affine_node(torch::Tensor g, torch::Tensor d_rowptr,
                               OptTensor d_perm, torch::Tensor s_rowptr,
                               OptTensor s_perm, long N) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.dim() == 2,
              "pair_affine_node: g must be a contiguous [E, H] GPU tensor");
  const long E = g.size(0), H = g.size(1);
  check_sizes(E, H, 0);
  TORCH_CHECK(N >= 0, "pair_affine_node: N must not be negative");
  torch::Tensor drk, srk, dpk, spk;
  const long* drp = rowptr_ptr(d_rowptr, N, drk);
  const long* srp = rowptr_ptr(s_rowptr, N, srk);
  const long* dpp = index_ptr(d_perm, E, dpk, "pair_affine: the dst perm");
  const long* spp = index_ptr(s_perm, E, spk, "pair_affine: the src perm");
  if (N * H == 0 || E == 0) return torch::zeros({N, 2 * H}, g.options());
  auto dP = torch::empty({N, 2 * H}, g.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, g.scalar_type(),
      "pair_affine_node", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        constexpr int kVec = 16 / sizeof(scalar_t);
        const scalar_t* gp = g.data_ptr<scalar_t>();
        scalar_t* op = dP.data_ptr<scalar_t>();
        auto launch = [&](auto kernel, long Fp) {
          hipLaunchKernelGGL(kernel, dim3(n_blocks(N * 2 * Fp)), dim3(kBlock),
                             0, stream, gp, drp, dpp, srp, spp, op, N, Fp);
        };
        if (H % kVec == 0 && all_aligned16(gp, op))
          launch(pair_affine_node_kernel<scalar_t, acc_t, kVec>, H / kVec);
        else
          launch(pair_affine_node_kernel<scalar_t, acc_t, 1>, H);
        check_launch("pair_affine_node_kernel");
      });
  return dP;
}

// (dr2[E], dea[E, D]), each undefined when its parameter is absent
std::vector<torch::Tensor> pair_affine_edge(torch::Tensor g, OptTensor wr,
                                            OptTensor weT) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.dim() == 2,
              "pair_affine_edge: g must be a contiguous [E, H] GPU tensor");
  const long E = g.size(0), H = g.size(1);
  const long D = weT.has_value() ? weT->size(0) : 0;
  check_sizes(E, H, D);
  const auto dtype = g.scalar_type();
  const void* wv = operand(wr, dtype, H, "w_r");
  const void* tv = operand(weT, dtype, D * H, "W_e^T");
  torch::Tensor dr2, dea;
  const bool empty = E * H == 0;
  auto make = [&](std::vector<int64_t> shape) {
    return empty ? torch::zeros(shape, g.options())
                 : torch::empty(shape, g.options());
  };
  if (wr.has_value()) dr2 = make({E});
  if (weT.has_value()) dea = make({E, D});
  if (empty || (!wr.has_value() && D == 0)) return {dr2, dea};
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, dtype,
      "pair_affine_edge", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        constexpr int kVec = 16 / sizeof(scalar_t);
        const scalar_t* gp = g.data_ptr<scalar_t>();
        scalar_t* o_r = wr.has_value() ? dr2.data_ptr<scalar_t>() : nullptr;
        scalar_t* o_e = D > 0 ? dea.data_ptr<scalar_t>() : nullptr;
        const bool packed = H % kVec == 0 && all_aligned16(gp, wv, tv);
        auto launch = [&](auto kernel, long Fp) {
          const int L = pow2_at_least(Fp, 64);
          hipLaunchKernelGGL(kernel, dim3(n_blocks(E * L)), dim3(kBlock), 0,
                             stream, gp, (const scalar_t*)wv,
                             (const scalar_t*)tv, o_r, o_e, E, Fp, (int)D, L);
        };
        if (packed && D <= 4)
          launch(pair_affine_edge_kernel<scalar_t, acc_t, kVec, 4>, H / kVec);
        else if (packed)
          launch(pair_affine_edge_kernel<scalar_t, acc_t, kVec, kMaxD>,
                 H / kVec);
        else if (D <= 4)
          launch(pair_affine_edge_kernel<scalar_t, acc_t, 1, 4>, H);
        else
          launch(pair_affine_edge_kernel<scalar_t, acc_t, 1, kMaxD>, H);
        check_launch("pair_affine_edge_kernel");
      });
  return {dr2, dea};
}

// chunks of E of a pair_affine_param launch: a function of E alone
long pair_affine_param_chunks(long E) {
  return std::max<long>(
      1, std::min<long>(kMaxChunks, (E + kChunkUnit - 1) / kChunkUnit));
}

// dw_r[H], dW_e[H, D] and db[H] from partial[n_chunks, 2 + D, H] in the
// accumulator type, chunks in ascending order, rounded once; an
// undefined output is skipped.  The second kernel of pair_affine_param,
// also of the wide route (edge_affine_mfma.hip).
void pair_affine_param_reduce(const torch::Tensor& partial,
                              torch::Tensor& dwr, torch::Tensor& dWe,
                              torch::Tensor& db, long H, long D,
                              long n_chunks) {
  const torch::Tensor& any = dwr.defined() ? dwr : (dWe.defined() ? dWe : db);
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, any.scalar_type(),
      "pair_affine_param_reduce", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        hipLaunchKernelGGL(
            (pair_affine_param_reduce_kernel<scalar_t, acc_t>),
            dim3(n_blocks((2 + D) * H)), dim3(kBlock), 0, stream,
            partial.data_ptr<acc_t>(),
            dwr.defined() ? dwr.data_ptr<scalar_t>() : nullptr,
            D > 0 && dWe.defined() ? dWe.data_ptr<scalar_t>() : nullptr,
            db.defined() ? db.data_ptr<scalar_t>() : nullptr, H, (int)D,
            n_chunks);
        check_launch("pair_affine_param_reduce_kernel");
      });
}

// (dw_r[H], dW_e[H, D], db[H]); dw_r and dW_e are undefined when r2 or
// ea is absent, db when want_bias is false
std::vector<torch::Tensor> pair_affine_param(torch::Tensor g, OptTensor r2,
                                             OptTensor ea, bool want_bias) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() && g.dim() == 2,
              "pair_affine_param: g must be a contiguous [E, H] GPU tensor");
  const long E = g.size(0), H = g.size(1);
  const long D = ea.has_value() ? ea->size(-1) : 0;
  check_sizes(E, H, D);
  const auto dtype = g.scalar_type();
  const void* rv = operand(r2, dtype, E, "r2");
  const void* ev = operand(ea, dtype, E * D, "ea");
  torch::Tensor dwr, dWe, db;
  const bool empty = E * H == 0;
  auto make = [&](std::vector<int64_t> shape) {
    return empty ? torch::zeros(shape, g.options())
                 : torch::empty(shape, g.options());
  };
  if (r2.has_value()) dwr = make({H});
  if (ea.has_value()) dWe = make({H, D});
  if (want_bias) db = make({H});
  if (empty || !(r2.has_value() || D > 0 || want_bias))
    return {dwr, dWe, db};
  if (D == 0) ev = nullptr;
  const long n_chunks = pair_affine_param_chunks(E);
  const long chunk_len = (E + n_chunks - 1) / n_chunks;
  // at most one wave across the features: at least four slices, whose
  // shorter chains of additions also carry less rounding error
  const int FT = pow2_at_least(H, 64);
  const long n_ftiles = (H + FT - 1) / FT;
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, dtype,
      "pair_affine_param", [&] {
        using acc_t = at::opmath_type<scalar_t>;
        auto partial = torch::empty(
            {n_chunks, 2 + D, H},
            g.options().dtype(c10::CppTypeToScalarType<acc_t>::value));
        acc_t* pp = partial.data_ptr<acc_t>();
        const size_t lds = (size_t)kBlock * (2 + D) * sizeof(acc_t);
        auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(
              kernel,
              dim3((unsigned)std::min<long>(n_chunks * n_ftiles, kGridCap)),
              dim3(kBlock), lds, stream, g.data_ptr<scalar_t>(),
              (const scalar_t*)rv, (const scalar_t*)ev, pp, E, H, (int)D, FT,
              chunk_len, n_chunks, n_ftiles);
        };
        if (D <= 4)
          launch(pair_affine_param_kernel<scalar_t, acc_t, 4>);
        else
          launch(pair_affine_param_kernel<scalar_t, acc_t, kMaxD>);
        check_launch("pair_affine_param_kernel");
        pair_affine_param_reduce(partial, dwr, dWe, db, H, D, n_chunks);
      });
  return {dwr, dWe, db};
}
