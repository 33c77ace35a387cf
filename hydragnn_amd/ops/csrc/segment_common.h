// What the segment kernel family shares (pna_aggr, gather_mul,
// painn_message, edge_affine): the bit-pattern packs and their
// conversions, the rounded product, the launch geometry, the alignment
// test of the packed route and the checks of the CSR operands.
//
// A file whose sums must not be fused with their products states
// `#pragma clang fp contract(off)` (and, where its contract needs it, the
// no-packed-fp32-ops attribute push and pop) itself, around its own
// kernels: they are that file's contract, and pna_aggr, which shares
// this header, has neither.  mul_rn carries the pragma in its own body,
// so its product is never fused wherever the header is included.
#pragma once

#include <torch/extension.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "check_launch.h"

namespace segment {

constexpr int kBlock = 256;
constexpr int kGridCap = 8192;

template <int BYTES> struct UIntOf;
template <> struct UIntOf<2> { using type = unsigned short; };
template <> struct UIntOf<4> { using type = unsigned int; };
template <> struct UIntOf<8> { using type = unsigned long; };

// A pack holds the bit patterns of its elements, and elements go to and
// from the accumulator type without an object of T in between: objects
// of the half class types (their constructors take a generic `this`)
// would keep the operand arrays in scratch memory instead of registers.
// The conversions are c10's own: round to nearest even for bf16,
// __float2half for f16.
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  typename UIntOf<sizeof(T)>::type v[VEC];
};

template <typename T> struct Bits;
template <> struct Bits<float> {
  static __device__ __forceinline__ float get(unsigned int b) {
    return __uint_as_float(b);
  }
  static __device__ __forceinline__ unsigned int put(float x) {
    return __float_as_uint(x);
  }
};
template <> struct Bits<double> {
  static __device__ __forceinline__ double get(unsigned long b) {
    return __longlong_as_double((long long)b);
  }
  static __device__ __forceinline__ unsigned long put(double x) {
    return (unsigned long)__double_as_longlong(x);
  }
};
template <> struct Bits<c10::BFloat16> {
  static __device__ __forceinline__ float get(unsigned short b) {
    return __uint_as_float((unsigned int)b << 16);
  }
  static __device__ __forceinline__ unsigned short put(float x) {
    return c10::detail::round_to_nearest_even(x);
  }
};
template <> struct Bits<c10::Half> {
  static __device__ __forceinline__ float get(unsigned short b) {
    return __half2float(__ushort_as_half(b));
  }
  static __device__ __forceinline__ unsigned short put(float x) {
    return __half_as_ushort(__float2half(x));
  }
};

// element k of a pack in the accumulator type; a value rounded to T
template <typename ACC, typename T, int VEC>
__device__ __forceinline__ ACC ld(const Pack<T, VEC>& p, int k) {
  return Bits<T>::get(p.v[k]);
}

template <typename T, int VEC, typename ACC>
__device__ __forceinline__ void st(Pack<T, VEC>& p, int k, ACC x) {
  p.v[k] = Bits<T>::put(x);
}

// element i of a plain array of T
template <typename ACC, typename T>
__device__ __forceinline__ ACC ld1(const T* __restrict__ a, long i) {
  return ld<ACC>(reinterpret_cast<const Pack<T, 1>*>(a)[i], 0);
}

template <typename T, typename ACC>
__device__ __forceinline__ void st1(T* __restrict__ a, long i, ACC x) {
  st(reinterpret_cast<Pack<T, 1>*>(a)[i], 0, x);
}

// A product rounded to its type.  __fmul_rn / __dmul_rn are a plain
// product in the HIP headers, which the compiler's default (contract =
// fast) would still fuse with an add that follows in the caller; the
// pragma takes the product out of that.  Forced inline like ld and st:
// the inliner's own judgement refuses a callee that lacks a target
// attribute of its caller, and painn_message and edge_affine compile
// their kernels under one (no-packed-fp32-ops).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fmul_rn(a, b);
}
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return __dmul_rn(a, b);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// blocks of a grid-stride launch over `threads` threads: at least one,
// at most the grid cap
inline int n_blocks(long threads) {
  long b = (threads + kBlock - 1) / kBlock;
  return (int)std::min<long>(std::max<long>(b, 1), kGridCap);
}

// a null pointer (an absent operand) counts as aligned
inline bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

template <typename... Ptrs>
inline bool all_aligned16(Ptrs... ptrs) {
  return (aligned16(ptrs) && ...);
}

// the least power of two >= n, at most cap
inline int pow2_at_least(long n, int cap) {
  int L = 1;
  while (L < cap && L < n) L <<= 1;
  return L;
}

// An index or perm over n edges: a null pointer when absent (the
// identity), else int64 [n] on the device.  `keep` holds the tensor the
// pointer belongs to, a contiguous copy where idx is not contiguous.
inline const long* index_ptr(const c10::optional<torch::Tensor>& idx, long n,
                             torch::Tensor& keep, const char* what) {
  if (!idx.has_value()) return nullptr;
  TORCH_CHECK(idx->is_cuda() && idx->dtype() == torch::kLong &&
                  idx->dim() == 1 && idx->numel() == n,
              what, " must be int64 [", n, "] on the device");
  keep = idx->contiguous();
  return keep.data_ptr<long>();
}

// the row pointer of a CSR over N rows
inline const long* rowptr_ptr(const torch::Tensor& rowptr, long N,
                              torch::Tensor& keep) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.dtype() == torch::kLong &&
                  rowptr.dim() == 1 && N >= 0 && rowptr.numel() == N + 1,
              "rowptr must be int64 [N + 1] on the device");
  keep = rowptr.contiguous();
  return keep.data_ptr<long>();
}

}  // namespace segment
