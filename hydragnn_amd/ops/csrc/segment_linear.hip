// Segment linear-attention primitives (CDNA4/gfx950).
//
// Rows are [N, H, .] and contiguous, graphs are contiguous row ranges
// given by the int64 rowptr ptr[G+1]; g(i) is the graph of row i.
//
//   segment_outer_sum   K[g,h,al,be] = sum_{i in g} A[i,h,al] B[i,h,be]
//   segment_matvec      O[i,h,be] = sum_al A[i,h,al] K[g(i),h,al,be]
//                       (trans: O[i,h,al] = sum_be A[i,h,be] K[..,al,be])
//
// Each primitive's gradients are the other primitive, so the pair is
// closed under differentiation (ops/segment_linear.py).  Segment matrices
// are always in the accumulator type (fp32 for fp32 and bf16 rows, fp64
// for fp64 rows), as output of the first and as input of the second; row
// outputs are rounded once to the row dtype.  No atomics anywhere.
//
//   seglin_outer_kernel   one workgroup per (graph, head, z).  The 256
//       threads form a 16 x 16 grid over the a x b matrix; thread
//       (ai, bi) owns the PA x QB register tile al = ai*PA + p,
//       be = bi + 16 q.  Row tiles of R = 32 rows of A and B are staged
//       in LDS in the accumulator type and every thread walks the tile's
//       rows in ascending order, one FMA per row and element.  Workgroup
//       z takes the contiguous run of row tiles
//       [z*ceil(T/Z), (z+1)*ceil(T/Z)) of its segment's T tiles and
//       writes the partial [g, h, z, a, b]; with Z = 1 that is K itself
//       and the sum is the plain ascending-row sum.
//   seglin_zsum_kernel    adds the Z partials of an element in ascending
//       z with one thread per element: a fixed association.
//   seglin_matvec_kernel  one workgroup per (graph, head, z).  The
//       segment matrix is staged in LDS once (transposed while staging
//       when trans, so the inner loop is the same) as M[win][wout]; a row
//       is owned by 16 adjacent lanes, lane l computes the outputs
//       j = l + 16 q from the row staged in LDS, k ascending.  The four
//       rows of a wave read the same M words (broadcast) and the 16
//       lanes of a row read consecutive ones.  Workgroup z takes the row
//       passes z, z+Z, .. of 16 rows each; a row's result does not
//       depend on Z.
//
// Z is a function of the host-known shapes only (the mean segment
// length N / G), so there is no sync and the association is the same
// every run.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "check_launch.h"

namespace {

template <typename T> struct sl_acc { using type = float; };
template <> struct sl_acc<double> { using type = double; };

constexpr int SL_BLOCK = 256;
constexpr int SL_R = 32;          // outer sum: rows per LDS tile
constexpr int SL_LPR = 16;        // matvec: lanes per row
constexpr int SL_BW = SL_BLOCK / SL_LPR;   // matvec: rows per pass
constexpr int SL_MAX_A = 128, SL_MAX_B = 132;
constexpr int SL_MAX_Z = 32;
constexpr long SL_LDS_BUDGET = 160 * 1024;

// Row range of graph g, empty when the pointer is not a valid range of
// [0, N].
__device__ __forceinline__ void seg_range(const long* __restrict__ ptr,
                                          long g, long N, long& lo,
                                          long& cnt) {
  lo = ptr[g];
  cnt = ptr[g + 1] - lo;
  if (lo < 0 || cnt < 0 || lo + cnt > N) cnt = 0;
}

template <typename T, int PA, int QB>
__global__ __launch_bounds__(SL_BLOCK) void seglin_outer_kernel(
    const T* __restrict__ A, const T* __restrict__ B,
    const long* __restrict__ ptr,
    typename sl_acc<T>::type* __restrict__ out, long N, int H, int a,
    int b) {
  using ACC = typename sl_acc<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int AP = 16 * PA, BP = 16 * QB;
  ACC* As = reinterpret_cast<ACC*>(smem);    // [SL_R][AP]
  ACC* Bs = As + SL_R * AP;                  // [SL_R][BP]
  const int tid = threadIdx.x;
  const int ai = tid >> 4, bi = tid & 15;
  const long g = blockIdx.x;
  const int h = blockIdx.y, z = blockIdx.z, Z = gridDim.z;
  long lo, cnt;
  seg_range(ptr, g, N, lo, cnt);
  const long tiles = (cnt + SL_R - 1) / SL_R;
  const long per = (tiles + Z - 1) / Z;
  const long t0 = std::min<long>((long)z * per, tiles);
  const long t1 = std::min<long>(t0 + per, tiles);

  ACC acc[PA][QB];
#pragma unroll
  for (int p = 0; p < PA; ++p)
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[p][q] = 0;

  for (long t = t0; t < t1; ++t) {
    const long r0 = lo + t * SL_R;
    const int nr = (int)std::min<long>(SL_R, lo + cnt - r0);
    __syncthreads();
    for (int idx = tid; idx < nr * a; idx += SL_BLOCK) {
      const int r = idx / a, c = idx - r * a;
      As[r * AP + c] =
          static_cast<ACC>(A[((r0 + r) * H + h) * (long)a + c]);
    }
    for (int idx = tid; idx < nr * b; idx += SL_BLOCK) {
      const int r = idx / b, c = idx - r * b;
      Bs[r * BP + c] =
          static_cast<ACC>(B[((r0 + r) * H + h) * (long)b + c]);
    }
    __syncthreads();
    // columns past a or b hold whatever LDS held; they only reach
    // accumulators that are never stored
    for (int r = 0; r < nr; ++r) {
      ACC av[PA], bv[QB];
#pragma unroll
      for (int p = 0; p < PA; ++p) av[p] = As[r * AP + ai * PA + p];
#pragma unroll
      for (int q = 0; q < QB; ++q) bv[q] = Bs[r * BP + bi + 16 * q];
#pragma unroll
      for (int p = 0; p < PA; ++p)
#pragma unroll
        for (int q = 0; q < QB; ++q)
          acc[p][q] = fma(av[p], bv[q], acc[p][q]);
    }
  }

  ACC* o = out + (((long)g * H + h) * Z + z) * (long)a * b;
#pragma unroll
  for (int p = 0; p < PA; ++p) {
    const int al = ai * PA + p;
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int be = bi + 16 * q;
      if (al < a && be < b) o[(long)al * b + be] = acc[p][q];
    }
  }
}

template <typename ACC>
__global__ __launch_bounds__(SL_BLOCK) void seglin_zsum_kernel(
    const ACC* __restrict__ part, ACC* __restrict__ out, long GH, long ab,
    int Z) {
  const long idx = (long)blockIdx.x * SL_BLOCK + threadIdx.x;
  if (idx >= GH * ab) return;
  const long gh = idx / ab, e = idx - gh * ab;
  const ACC* p = part + gh * Z * ab + e;
  ACC s = p[0];
  for (int z = 1; z < Z; ++z) s += p[(long)z * ab];
  out[idx] = s;
}

template <typename T, int QO>
__global__ __launch_bounds__(SL_BLOCK) void seglin_matvec_kernel(
    const T* __restrict__ A, const typename sl_acc<T>::type* __restrict__ K,
    const long* __restrict__ ptr, T* __restrict__ O, long N, int H, int a,
    int b, int trans) {
  using ACC = typename sl_acc<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int win = trans ? b : a, wout = trans ? a : b;
  const int wp = win | 1;                    // odd row stride for As
  ACC* Ms = reinterpret_cast<ACC*>(smem);    // [win][wout]
  ACC* As = Ms + win * wout;                 // [SL_BW][wp]
  const int tid = threadIdx.x;
  const int row = tid / SL_LPR, l = tid % SL_LPR;
  const long g = blockIdx.x;
  const int h = blockIdx.y, z = blockIdx.z, Z = gridDim.z;
  long lo, cnt;
  seg_range(ptr, g, N, lo, cnt);
  const long passes = (cnt + SL_BW - 1) / SL_BW;
  if (z >= passes) return;                   // whole workgroup

  const ACC* Kg = K + ((long)g * H + h) * (long)a * b;
  if (!trans) {
    for (int idx = tid; idx < a * b; idx += SL_BLOCK) Ms[idx] = Kg[idx];
  } else {
    // Ms[be][al] = K[al][be]
    for (int idx = tid; idx < a * b; idx += SL_BLOCK) {
      const int al = idx / b, be = idx - al * b;
      Ms[be * a + al] = Kg[idx];
    }
  }

  for (long ps = z; ps < passes; ps += Z) {
    const long r0 = lo + ps * SL_BW;
    const int nr = (int)std::min<long>(SL_BW, lo + cnt - r0);
    __syncthreads();
    for (int idx = tid; idx < nr * win; idx += SL_BLOCK) {
      const int r = idx / win, c = idx - r * win;
      As[r * wp + c] =
          static_cast<ACC>(A[((r0 + r) * H + h) * (long)win + c]);
    }
    __syncthreads();
    if (row < nr) {
      ACC acc[QO];
#pragma unroll
      for (int q = 0; q < QO; ++q) acc[q] = 0;
      const ACC* ar = As + row * wp;
      for (int k = 0; k < win; ++k) {
        const ACC x = ar[k];
        const ACC* m = Ms + k * wout + l;
#pragma unroll
        for (int q = 0; q < QO; ++q)
          if (l + 16 * q < wout) acc[q] = fma(x, m[16 * q], acc[q]);
      }
      T* o = O + ((r0 + row) * H + h) * (long)wout;
#pragma unroll
      for (int q = 0; q < QO; ++q)
        if (l + 16 * q < wout) o[l + 16 * q] = static_cast<T>(acc[q]);
    }
  }
}

inline long round16(long x) { return (x + 15) / 16 * 16; }

// register-tile instance that serves a width: 16 * tile >= width
inline int pa_of(long a) { return a <= 64 ? 4 : 8; }
inline int qb_of(long w) { return w <= 32 ? 2 : w <= 48 ? 3 : w <= 80 ? 5 : 9; }

long lds_bytes(long a, long b, long acc, long pass) {
  if (pass == 0)
    return round16((long)SL_R * 16 * (pa_of(a) + qb_of(b)) * acc);
  const long win = pass == 1 ? a : b, wout = pass == 1 ? b : a;
  return round16((win * wout + (long)SL_BW * (win | 1)) * acc);
}

long acc_bytes_of(at::ScalarType t) {
  TORCH_CHECK(t == at::ScalarType::Float || t == at::ScalarType::Double ||
                  t == at::ScalarType::BFloat16,
              "segment_linear: rows must be fp32, bf16 or fp64");
  return t == at::ScalarType::Double ? 8 : 4;
}

void check_envelope(long a, long b) {
  TORCH_CHECK(a >= 1 && a <= SL_MAX_A && b >= 1 && b <= SL_MAX_B,
              "segment_linear: outside the kernel envelope (1 <= a <= ",
              SL_MAX_A, ", 1 <= b <= ", SL_MAX_B, "), got a=", a, " b=", b);
}

void check_rows(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && t.is_contiguous(),
              "segment_linear: ", what,
              " must be a contiguous [N, H, w] device tensor");
}

void check_ptr(const torch::Tensor& ptr) {
  TORCH_CHECK(ptr.is_cuda() && ptr.dim() == 1 && ptr.is_contiguous() &&
                  ptr.scalar_type() == at::ScalarType::Long &&
                  ptr.numel() >= 1,
              "segment_linear: ptr must be a contiguous int64 [G+1] "
              "device vector");
}

// Workgroups per (graph, head): 1.5 mean-length's worth of work units
// of `rows` rows, no more than fill the device a few times over.
int split_of(long N, long G, long H, long rows) {
  long z = (3 * N + 2 * G * rows - 1) / (2 * G * rows);
  const long fill = (2048 + G * H - 1) / (G * H);
  z = std::min<long>(z, fill);
  return (int)std::min<long>(std::max<long>(z, 1), SL_MAX_Z);
}

hipStream_t sl_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

template <typename T, int PA>
void launch_outer_qb(int qb, dim3 grid, size_t lds, const T* A, const T* B,
                     const long* ptr, typename sl_acc<T>::type* out, long N,
                     int H, int a, int b) {
#define SL_OUTER(QB)                                                       \
  hipLaunchKernelGGL((seglin_outer_kernel<T, PA, QB>), grid,               \
                     dim3(SL_BLOCK), lds, sl_stream(), A, B, ptr, out, N,  \
                     H, a, b)
  switch (qb) {
    case 2: SL_OUTER(2); break;
    case 3: SL_OUTER(3); break;
    case 5: SL_OUTER(5); break;
    default: SL_OUTER(9); break;
  }
#undef SL_OUTER
}

template <typename T>
void launch_matvec(int qo, dim3 grid, size_t lds, const T* A,
                   const typename sl_acc<T>::type* K, const long* ptr, T* O,
                   long N, int H, int a, int b, int trans) {
#define SL_MATVEC(QO)                                                      \
  hipLaunchKernelGGL((seglin_matvec_kernel<T, QO>), grid, dim3(SL_BLOCK),  \
                     lds, sl_stream(), A, K, ptr, O, N, H, a, b, trans)
  switch (qo) {
    case 2: SL_MATVEC(2); break;
    case 3: SL_MATVEC(3); break;
    case 5: SL_MATVEC(5); break;
    default: SL_MATVEC(9); break;
  }
#undef SL_MATVEC
}

}  // namespace

// Dynamic-LDS bytes of a launch for row dtype `dtype`.  pass: 0 outer
// sum, 1 matvec, 2 matvec with trans.
long segment_linear_lds_bytes(long a, long b, at::ScalarType dtype,
                              long pass) {
  TORCH_CHECK(pass >= 0 && pass <= 2, "pass must be 0, 1 or 2");
  check_envelope(a, b);
  return lds_bytes(a, b, acc_bytes_of(dtype), pass);
}

// {row-tile length R of the outer sum, rows one matvec workgroup handles
// per pass}.  Neither depends on (a, b, dtype) in this mapping; the
// arguments keep the interface open for one where they do.
std::vector<long> segment_linear_tiling(long a, long b,
                                        at::ScalarType dtype) {
  check_envelope(a, b);
  acc_bytes_of(dtype);
  return {SL_R, SL_BW};
}

// K[G, H, a, b] in the accumulator type.  z <= 0 picks the split from
// the shapes.
torch::Tensor segment_outer_sum(torch::Tensor A, torch::Tensor B,
                                torch::Tensor ptr, long z) {
  check_rows(A, "A");
  check_rows(B, "B");
  check_ptr(ptr);
  TORCH_CHECK(B.scalar_type() == A.scalar_type() &&
                  B.size(0) == A.size(0) && B.size(1) == A.size(1),
              "segment_outer_sum: A and B must agree in dtype, N and H");
  const long N = A.size(0), H = A.size(1), a = A.size(2), b = B.size(2);
  const long G = ptr.numel() - 1;
  check_envelope(a, b);
  const long acc = acc_bytes_of(A.scalar_type());
  TORCH_CHECK(H <= 65535, "segment_outer_sum: head count above 65535");
  TORCH_CHECK(G < (1L << 31), "segment_outer_sum: too many graphs");
  TORCH_CHECK(z <= SL_MAX_Z, "segment_outer_sum: z above ", SL_MAX_Z);
  const long lds = lds_bytes(a, b, acc, 0);
  TORCH_CHECK(lds <= SL_LDS_BUDGET, "segment_outer_sum: LDS over 160 KiB");
  auto kopt = A.options().dtype(acc == 8 ? torch::kDouble : torch::kFloat);
  if (N == 0 || G == 0 || H == 0)
    return torch::zeros({G, H, a, b}, kopt);
  const int Z = z > 0 ? (int)z : split_of(N, G, H, SL_R);
  auto K = torch::empty({G, H, a, b}, kopt);
  torch::Tensor part;
  if (Z > 1) part = torch::empty({G, H, (long)Z, a, b}, kopt);
  const dim3 grid(G, H, Z);
  AT_DISPATCH_FLOATING_TYPES_AND(
      at::ScalarType::BFloat16, A.scalar_type(), "segment_outer_sum", [&] {
        using ACC = typename sl_acc<scalar_t>::type;
        ACC* out = (Z > 1 ? part : K).data_ptr<ACC>();
        const scalar_t* pa = A.data_ptr<scalar_t>();
        const scalar_t* pb = B.data_ptr<scalar_t>();
        if (pa_of(a) == 4)
          launch_outer_qb<scalar_t, 4>(qb_of(b), grid, lds, pa, pb,
                                       ptr.data_ptr<long>(), out, N,
                                       (int)H, (int)a, (int)b);
        else
          launch_outer_qb<scalar_t, 8>(qb_of(b), grid, lds, pa, pb,
                                       ptr.data_ptr<long>(), out, N,
                                       (int)H, (int)a, (int)b);
        check_launch("segment_outer_sum");
        if (Z > 1) {
          const long total = G * H * a * b;
          hipLaunchKernelGGL(
              seglin_zsum_kernel<ACC>,
              dim3((total + SL_BLOCK - 1) / SL_BLOCK), dim3(SL_BLOCK), 0,
              sl_stream(), part.data_ptr<ACC>(), K.data_ptr<ACC>(), G * H,
              a * b, Z);
          check_launch("segment_outer_sum (partial sum)");
        }
      });
  return K;
}

// O[N, H, b] (trans: [N, H, a]) in A's dtype; K is [G, H, a, b] in the
// accumulator type of A's dtype.
torch::Tensor segment_matvec(torch::Tensor A, torch::Tensor K,
                             torch::Tensor ptr, bool trans) {
  check_rows(A, "A");
  check_ptr(ptr);
  TORCH_CHECK(K.is_cuda() && K.dim() == 4 && K.is_contiguous(),
              "segment_matvec: K must be a contiguous [G, H, a, b] device "
              "tensor");
  const long N = A.size(0), H = A.size(1), a = K.size(2), b = K.size(3);
  const long G = ptr.numel() - 1;
  check_envelope(a, b);
  const long acc = acc_bytes_of(A.scalar_type());
  TORCH_CHECK(K.scalar_type() ==
                  (acc == 8 ? at::ScalarType::Double : at::ScalarType::Float),
              "segment_matvec: K must be in the accumulator type of A");
  TORCH_CHECK(K.size(0) == G && K.size(1) == H,
              "segment_matvec: K must be [G, H, a, b] for ptr and A");
  const long win = trans ? b : a, wout = trans ? a : b;
  TORCH_CHECK(A.size(2) == win, "segment_matvec: A must have width ", win);
  TORCH_CHECK(H <= 65535, "segment_matvec: head count above 65535");
  TORCH_CHECK(G < (1L << 31), "segment_matvec: too many graphs");
  const long lds = lds_bytes(a, b, acc, trans ? 2 : 1);
  TORCH_CHECK(lds <= SL_LDS_BUDGET, "segment_matvec: LDS over 160 KiB");
  auto O = torch::empty({N, H, wout}, A.options());
  if (N == 0 || G == 0 || H == 0) return O;
  const dim3 grid(G, H, split_of(N, G, H, SL_BW));
  AT_DISPATCH_FLOATING_TYPES_AND(
      at::ScalarType::BFloat16, A.scalar_type(), "segment_matvec", [&] {
        using ACC = typename sl_acc<scalar_t>::type;
        launch_matvec<scalar_t>(qb_of(wout), grid, lds,
                                A.data_ptr<scalar_t>(), K.data_ptr<ACC>(),
                                ptr.data_ptr<long>(),
                                O.data_ptr<scalar_t>(), N, (int)H, (int)a,
                                (int)b, trans ? 1 : 0);
      });
  check_launch("segment_matvec");
  return O;
}
