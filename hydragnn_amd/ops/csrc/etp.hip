// Fused equivariant tensor-product contraction kernels (CDNA4/gfx950).
//
// The MACE hot path is per-edge / per-node SMALL trilinear contractions
//   out[i, c, o] = sum_entries coef * A[i, c, a] * B[i, b] * C[i, c, g]
// (entry table = flattened Wigner-3j paths).  hipBLASLt runs these as
// tiny-batched GEMMs at ~2% of HBM bandwidth; here one kernel does the
// whole contraction: a 32-thread group per (i, c) pair stages the A/B/C
// rows in LDS, each thread owns one output index and walks its slice of
// the (sorted-by-output) entry table.  VGPR use stays low (no
// runtime-indexed register arrays -> no scratch), so occupancy is high
// and the kernel runs at the memory-bound roofline.
//
// The same kernel computes every first- and second-order derivative of
// the contraction: gradients of a trilinear form are trilinear forms
// with role-permuted entry tables (see ops/etp.py), so force training
// (create_graph=True double backward) never leaves this kernel family.
// The sweep kernels at the end of the file produce several of those
// derivatives per launch, with every row staged once.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace {

// accumulator type: fp32 for bf16/half/float inputs, fp64 for double
// (fp64 ETP support: slices and channel reductions keep full width)
template <typename T> struct acc_of { using type = float; };
template <> struct acc_of<double> { using type = double; };

// out[i,c,o] = sum over entries(coef, a, b, g, o) of
//              coef * A[i,c,a] * B[i,b] * C[i,c,g]
//
// One THREAD per (i, c): its A/B/C rows and do-accumulator live in a
// per-thread LDS slice (runtime entry indices would force register
// arrays to scratch otherwise).  Every thread walks the SAME entry
// list in lockstep (entry words are wave-uniform LDS broadcasts), so
// there is no divergence; global loads/stores are per-thread
// contiguous rows -> coalesced across adjacent threads.  Slice stride
// is padded to an odd word count to spread LDS banks.
template <typename T>
__global__ void etp_general_kernel(
    const T* __restrict__ A, const T* __restrict__ B,
    const T* __restrict__ C, T* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long NC, int nch, int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ bi,
    const long* __restrict__ ci) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = ((da + db + dg + do_) | 1);  // odd word stride
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);

  // stage the entry table once per block
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }

  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* my = slices + (size_t)threadIdx.x * stride;
  ACC* ma = my;
  ACC* mb = ma + da;
  ACC* mc = mb + db;
  ACC* mo = mc + dg;
  if (i < NC) {
    long e = i / nch;
    int c = (int)(i - e * nch);
    long ea = ai ? ai[e] : e;
    long eb = bi ? bi[e] : e;
    long ec = ci ? ci[e] : e;
    const T* ap = A + (ea * nch + c) * da;
    const T* bp = B + eb * db;
    const T* cp = C + (ec * nch + c) * dg;
    for (int k = 0; k < da; ++k) ma[k] = (ACC)ap[k];
    for (int k = 0; k < db; ++k) mb[k] = (ACC)bp[k];
    for (int k = 0; k < dg; ++k) mc[k] = (ACC)cp[k];
    for (int k = 0; k < do_; ++k) mo[k] = 0.f;
  }
  __syncthreads();
  if (i < NC) {
    for (int k = 0; k < n_ent; ++k) {
      int4 q = ent_lds[k];
      mo[q.w] += coef_lds[k] * ma[q.x] * mb[q.y] * mc[q.z];
    }
    T* op = out + i * do_;
    for (int k = 0; k < do_; ++k) op[k] = (T)mo[k];
  }
}

// Register-accumulation variant (LDS-pressure fallback): the entry table is
// sorted by output slot with per-output (start, count) ranges
// (ETPTable.device_tensors), so each output accumulates in a REGISTER
// and stores once — the r1 kernel's mo[q.w] += ... formed a serially
// dependent LDS read-modify-write chain (consecutive entries hit the
// same address; PMC: SQ busy only ~13% of wall time = latency-bound).
// The LDS accumulator slice disappears too (smaller stride -> higher
// occupancy).
template <typename T>
__global__ void etp_general_racc_kernel(
    const T* __restrict__ A, const T* __restrict__ B,
    const T* __restrict__ C, T* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs,
    const int2* __restrict__ o_ranges, int n_ent,
    long NC, int nch, int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ bi,
    const long* __restrict__ ci) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = ((da + db + dg) | 1);
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  int2* rng_lds = reinterpret_cast<int2*>(coef_lds + n_ent);

  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  for (int k = threadIdx.x; k < do_; k += blockDim.x)
    rng_lds[k] = o_ranges[k];

  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* my = slices + (size_t)threadIdx.x * stride;
  ACC* ma = my;
  ACC* mb = ma + da;
  ACC* mc = mb + db;
  if (i < NC) {
    long e = i / nch;
    int c = (int)(i - e * nch);
    long ea = ai ? ai[e] : e;
    long eb = bi ? bi[e] : e;
    long ec = ci ? ci[e] : e;
    const T* ap = A + (ea * nch + c) * da;
    const T* bp = B + eb * db;
    const T* cp = C + (ec * nch + c) * dg;
    for (int k = 0; k < da; ++k) ma[k] = (ACC)ap[k];
    for (int k = 0; k < db; ++k) mb[k] = (ACC)bp[k];
    for (int k = 0; k < dg; ++k) mc[k] = (ACC)cp[k];
  }
  __syncthreads();
  if (i >= NC) return;
  T* op = out + i * do_;
  for (int o = 0; o < do_; ++o) {
    int s = rng_lds[o].x;
    int cnt = rng_lds[o].y;
    ACC acc = (ACC)0;
    for (int k = s; k < s + cnt; ++k) {
      int4 q = ent_lds[k];
      acc += coef_lds[k] * ma[q.x] * mb[q.y] * mc[q.z];
    }
    op[o] = (T)acc;
  }
}

// Occupancy variant of etp_general: A/B/C rows are PRIVATE per thread
// and only ~1-3 cache lines each, so after first touch they are
// L1-hot — staging them in LDS buys nothing but caps the block count
// at 1/CU (zero latency hiding; PMC showed SQ busy ~10% of kernel
// wall time).  Here only the runtime-indexed OUTPUT accumulator lives
// in LDS; operand reads go straight to L1.  The host picks whichever
// variant yields more blocks/CU.
template <typename T>
__global__ void etp_general_l1_kernel(
    const T* __restrict__ A, const T* __restrict__ B,
    const T* __restrict__ C, T* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long NC, int nch, int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ bi,
    const long* __restrict__ ci) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = do_ | 1;
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* mo = slices + (size_t)threadIdx.x * stride;
  __syncthreads();
  if (i >= NC) return;
  long e = i / nch;
  int c = (int)(i - e * nch);
  long ea = ai ? ai[e] : e;
  long eb = bi ? bi[e] : e;
  long ec = ci ? ci[e] : e;
  const T* ap = A + (ea * nch + c) * da;
  const T* bp = B + eb * db;
  const T* cp = C + (ec * nch + c) * dg;
  for (int k = 0; k < do_; ++k) mo[k] = 0.f;
  for (int k = 0; k < n_ent; ++k) {
    int4 q = ent_lds[k];
    mo[q.w] += coef_lds[k] * (ACC)ap[q.x] * (ACC)bp[q.y] *
               (ACC)cp[q.z];
  }
  T* op = out + i * do_;
  for (int k = 0; k < do_; ++k) op[k] = (T)mo[k];
}

// out[e,b] = sum_c sum over entries(coef, a, b, g, o) of
//            coef * A[e,c,a] * C[e,c,g] * D[e,c,o]
// (the B-slot gradient: reduce over channels).  Same structure as
// etp_general: one thread per (e, c), rows + db-accumulator in a
// per-thread LDS slice, uniform entry walk; the channel reduction is
// db fp32 atomicAdds per thread (db <= 12, light contention).
template <typename T>
__global__ void etp_reduce_kernel(
    const T* __restrict__ A, const T* __restrict__ C,
    const T* __restrict__ D,
    typename acc_of<T>::type* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long E, int nch, int da, int db, int dg, int do_) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = ((da + dg + do_ + db) | 1);
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  long NC = E * nch;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* my = slices + (size_t)threadIdx.x * stride;
  ACC* ma = my;
  ACC* mc = ma + da;
  ACC* md = mc + dg;
  ACC* mb = md + do_;
  if (i < NC) {
    const T* ap = A + i * da;
    const T* cp = C + i * dg;
    const T* dp = D + i * do_;
    for (int k = 0; k < da; ++k) ma[k] = (ACC)ap[k];
    for (int k = 0; k < dg; ++k) mc[k] = (ACC)cp[k];
    for (int k = 0; k < do_; ++k) md[k] = (ACC)dp[k];
    for (int k = 0; k < db; ++k) mb[k] = 0.f;
  }
  __syncthreads();
  if (i < NC) {
    for (int k = 0; k < n_ent; ++k) {
      int4 q = ent_lds[k];
      mb[q.y] += coef_lds[k] * ma[q.x] * mc[q.z] * md[q.w];
    }
  }
  long e = i / nch;
  if (nch % 64 == 0) {
    // a wave spans exactly one edge's channels: shuffle-reduce each b
    // across the 64 lanes, then ONE atomic per b per wave
    for (int b = 0; b < db; ++b) {
      ACC v = (i < NC) ? mb[b] : (ACC)0;
      for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_down(v, off, 64);
      if ((threadIdx.x % 64) == 0 && i < NC)
        atomicAdd(&out[e * db + b], v);
    }
  } else if (i < NC) {
    for (int b = 0; b < db; ++b) atomicAdd(&out[e * db + b], mb[b]);
  }
}

// Fused gather + tensor product + segment sum:
//   out[r, c, o] = sum_{e in rowptr[r]..rowptr[r+1]} sum_k coef_k
//                  A[ai[e], c, a] B[bi[e], b] C[ci[e], c, g]
// One thread per (out row, channel); the edge loop restages each
// edge's rows into the thread's LDS slice — removes the materialized
// per-edge message tensor, its scatter pass, and the standalone node
// gather of the unfused pipeline.
template <typename T>
__global__ void etp_nodesum_kernel(
    const T* __restrict__ A, const T* __restrict__ B,
    const T* __restrict__ C, T* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    const long* __restrict__ rowptr, long R, int nch,
    int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ bi,
    const long* __restrict__ ci) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = ((da + db + dg + do_) | 1);
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  long RC = R * nch;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* my = slices + (size_t)threadIdx.x * stride;
  ACC* ma = my;
  ACC* mb = ma + da;
  ACC* mc = mb + db;
  ACC* mo = mc + dg;
  __syncthreads();
  if (i >= RC) return;
  long r = i / nch;
  int c = (int)(i - r * nch);
  for (int k = 0; k < do_; ++k) mo[k] = 0.f;
  long lo = rowptr[r], hi = rowptr[r + 1];
  for (long e = lo; e < hi; ++e) {
    long ea = ai ? ai[e] : e;
    long eb = bi ? bi[e] : e;
    long ec = ci ? ci[e] : e;
    const T* ap = A + (ea * nch + c) * da;
    const T* bp = B + eb * db;
    const T* cp = C + (ec * nch + c) * dg;
    for (int k = 0; k < da; ++k) ma[k] = (ACC)ap[k];
    for (int k = 0; k < db; ++k) mb[k] = (ACC)bp[k];
    for (int k = 0; k < dg; ++k) mc[k] = (ACC)cp[k];
    for (int k = 0; k < n_ent; ++k) {
      int4 q = ent_lds[k];
      mo[q.w] += coef_lds[k] * ma[q.x] * mb[q.y] * mc[q.z];
    }
  }
  T* op = out + i * do_;
  for (int k = 0; k < do_; ++k) op[k] = (T)mo[k];
}

// etp_reduce with per-slot row indices
template <typename T>
__global__ void etp_reduce_idx_kernel(
    const T* __restrict__ A, const T* __restrict__ C,
    const T* __restrict__ D,
    typename acc_of<T>::type* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long E, int nch, int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ ci,
    const long* __restrict__ di) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = ((da + dg + do_ + db) | 1);
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  long NC = E * nch;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* my = slices + (size_t)threadIdx.x * stride;
  ACC* ma = my;
  ACC* mc = ma + da;
  ACC* md = mc + dg;
  ACC* mb = md + do_;
  if (i < NC) {
    long e = i / nch;
    int c = (int)(i - e * nch);
    long ea = ai ? ai[e] : e;
    long ec = ci ? ci[e] : e;
    long ed = di ? di[e] : e;
    const T* ap = A + (ea * nch + c) * da;
    const T* cp = C + (ec * nch + c) * dg;
    const T* dp = D + (ed * nch + c) * do_;
    for (int k = 0; k < da; ++k) ma[k] = (ACC)ap[k];
    for (int k = 0; k < dg; ++k) mc[k] = (ACC)cp[k];
    for (int k = 0; k < do_; ++k) md[k] = (ACC)dp[k];
    for (int k = 0; k < db; ++k) mb[k] = 0.f;
  }
  __syncthreads();
  if (i < NC) {
    for (int k = 0; k < n_ent; ++k) {
      int4 q = ent_lds[k];
      mb[q.y] += coef_lds[k] * ma[q.x] * mc[q.z] * md[q.w];
    }
  }
  long e = i / nch;
  if (nch % 64 == 0) {
    for (int b = 0; b < db; ++b) {
      ACC v = (i < NC) ? mb[b] : (ACC)0;
      for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_down(v, off, 64);
      if ((threadIdx.x % 64) == 0 && i < NC)
        atomicAdd(&out[e * db + b], v);
    }
  } else if (i < NC) {
    for (int b = 0; b < db; ++b) atomicAdd(&out[e * db + b], mb[b]);
  }
}

// L1-operand reduce variant: only the small db-accumulator lives in
// LDS; A/C/D rows are read straight through L1 (each row is 1-2 hot
// cache lines).  LDS per thread drops from (da+dg+do+db) to db words
// -> ~6x more waves per CU than the staged variant; the staged reduce
// measured only ~700-950 GB/s of the 8 TB/s roofline (latency-bound
// at 1-2 workgroups/CU).
template <typename T>
__global__ void etp_reduce_l1_kernel(
    const T* __restrict__ A, const T* __restrict__ C,
    const T* __restrict__ D,
    typename acc_of<T>::type* __restrict__ out,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long E, int nch, int da, int db, int dg, int do_,
    const long* __restrict__ ai, const long* __restrict__ ci,
    const long* __restrict__ di) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int stride = db | 1;
  ACC* slices = reinterpret_cast<ACC*>(smem);
  int4* ent_lds = reinterpret_cast<int4*>(
      smem + (size_t)blockDim.x * stride * sizeof(ACC));
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  long NC = E * nch;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  ACC* mb = slices + (size_t)threadIdx.x * stride;
  __syncthreads();
  long e = i / nch;
  if (i < NC) {
    int c = (int)(i - e * nch);
    long ea = ai ? ai[e] : e;
    long ec = ci ? ci[e] : e;
    long ed = di ? di[e] : e;
    const T* ap = A + (ea * nch + c) * da;
    const T* cp = C + (ec * nch + c) * dg;
    const T* dp = D + (ed * nch + c) * do_;
    for (int k = 0; k < db; ++k) mb[k] = 0.f;
    for (int k = 0; k < n_ent; ++k) {
      int4 q = ent_lds[k];
      mb[q.y] += coef_lds[k] * (ACC)ap[q.x] * (ACC)cp[q.z] *
                 (ACC)dp[q.w];
    }
  }
  if (nch % 64 == 0) {
    for (int b = 0; b < db; ++b) {
      ACC v = (i < NC) ? mb[b] : (ACC)0;
      for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_down(v, off, 64);
      if ((threadIdx.x % 64) == 0 && i < NC)
        atomicAdd(&out[e * db + b], v);
    }
  } else if (i < NC) {
    for (int b = 0; b < db; ++b) atomicAdd(&out[e * db + b], mb[b]);
  }
}

// ---------------------------------------------------------------------
// Sweep family: several derivatives of the quadrilinear form
//   Q(a,b,g,o) = sum_k coef_k a[a_k] b[b_k] g[g_k] o[o_k]
// in ONE walk of the entry table, every row staged once.  Slot bits:
// a=1, b=2, g=4, o=8.
// ---------------------------------------------------------------------

// Per-thread LDS slice layout, shared by host (footprint) and device:
// four primal rows, then the present tangent rows, then the masked
// output rows; odd word stride as in etp_general_kernel.
struct SweepLayout {
  int p[4], t[4], o[4], stride;
  __host__ __device__ SweepLayout(int da, int db, int dg, int do_,
                                  int tmask, int omask) {
    const int d[4] = {da, db, dg, do_};
    int off = 0;
    for (int s = 0; s < 4; ++s) { p[s] = off; off += d[s]; }
    for (int s = 0; s < 4; ++s) {
      t[s] = off;
      if (tmask & (1 << s)) off += d[s];
    }
    for (int s = 0; s < 4; ++s) {
      o[s] = off;
      if (omask & (1 << s)) off += d[s];
    }
    stride = off | 1;
  }
};

// Row moves between global memory and the LDS slice.  With `vec` (the
// host found every base 16-byte aligned) a row whose length allows it
// moves in packs of 4 or 2 elements (8/4-byte accesses for 2-byte
// types, 16/8 for fp32, 16 for fp64) instead of one access per element.
template <typename T, int W> struct alignas(sizeof(T) * W) RowPack {
  T v[W];
};

template <int W, typename T, typename ACC>
__device__ inline void load_packs(const T* __restrict__ p, ACC* dst,
                                  int d) {
  for (int k = 0; k < d; k += W) {
    const RowPack<T, W> q = *reinterpret_cast<const RowPack<T, W>*>(p + k);
    for (int j = 0; j < W; ++j) dst[k + j] = (ACC)q.v[j];
  }
}

template <int W, typename T, typename ACC>
__device__ inline void store_packs(T* __restrict__ p, const ACC* src,
                                   int d) {
  for (int k = 0; k < d; k += W) {
    RowPack<T, W> q;
    for (int j = 0; j < W; ++j) q.v[j] = (T)src[k + j];
    *reinterpret_cast<RowPack<T, W>*>(p + k) = q;
  }
}

template <typename T, typename ACC>
__device__ inline void load_row(const T* __restrict__ p, ACC* dst, int d,
                                bool vec) {
  constexpr int WMAX = sizeof(T) == 8 ? 2 : 4;
  if (vec && d % WMAX == 0) {
    load_packs<WMAX>(p, dst, d);
  } else if (vec && d % 2 == 0) {
    load_packs<2>(p, dst, d);
  } else {
    for (int k = 0; k < d; ++k) dst[k] = (ACC)p[k];
  }
}

template <typename T, typename ACC>
__device__ inline void store_row(T* __restrict__ p, const ACC* src, int d,
                                 bool vec) {
  constexpr int WMAX = sizeof(T) == 8 ? 2 : 4;
  if (vec && d % WMAX == 0) {
    store_packs<WMAX>(p, src, d);
  } else if (vec && d % 2 == 0) {
    store_packs<2>(p, src, d);
  } else {
    for (int k = 0; k < d; ++k) p[k] = (T)src[k];
  }
}

// ORDER 1: out_s = dQ/ds at the primals, for each s in omask.
// ORDER 2: out_s = sum over r != s with a tangent present of dQ/ds with
//          slot r replaced by its tangent (absent tangents count as 0).
// Same mapping as etp_general_kernel: one thread per (row, channel),
// uniform entry walk, fp32/fp64 accumulation in the LDS slice.  The b
// output is per row: with nch == 64 one wave is exactly one row, so a
// shuffle reduction ends in one store in the output dtype (outB);
// otherwise per-thread partials go to a zeroed accumulator (outB_acc)
// with atomics and the host casts.
// OMASK / TMASK >= 0 fix the output and tangent masks at compile time
// (the masks training uses), so the entry loop is one straight block;
// -1 reads them from the arguments.
template <typename T, int ORDER, int OMASK, int TMASK>
__global__ void etp_sweep_kernel(
    const T* __restrict__ pA, const T* __restrict__ pB,
    const T* __restrict__ pG, const T* __restrict__ pO,
    const T* __restrict__ tA, const T* __restrict__ tB,
    const T* __restrict__ tG, const T* __restrict__ tO,
    T* __restrict__ outA, T* __restrict__ outB,
    typename acc_of<T>::type* __restrict__ outB_acc,
    T* __restrict__ outG, T* __restrict__ outO,
    const int4* __restrict__ entries,
    const float* __restrict__ coefs, int n_ent,
    long rows, int nch, int da, int db, int dg, int do_, int omask,
    bool vec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  const int om = OMASK >= 0 ? OMASK : omask;
  const int tm = ORDER == 1 ? 0
                 : TMASK >= 0 ? TMASK
                 : (tA ? 1 : 0) | (tB ? 2 : 0) | (tG ? 4 : 0) | (tO ? 8 : 0);
  const bool hta = tm & 1, htb = tm & 2, htg = tm & 4, hto = tm & 8;
  const SweepLayout L(da, db, dg, do_, tm, om);
  ACC* slices = reinterpret_cast<ACC*>(smem);
  // table after the slices, on a 16-byte boundary for the int4 reads
  size_t slice_bytes =
      ((size_t)blockDim.x * L.stride * sizeof(ACC) + 15) & ~(size_t)15;
  int4* ent_lds = reinterpret_cast<int4*>(smem + slice_bytes);
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }

  const long NC = rows * nch;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < NC;
  const long e = i / nch;
  ACC* my = slices + (size_t)threadIdx.x * L.stride;
  ACC* xa = my + L.p[0];
  ACC* xb = my + L.p[1];
  ACC* xg = my + L.p[2];
  ACC* xo = my + L.p[3];
  ACC* ya = my + L.t[0];
  ACC* yb = my + L.t[1];
  ACC* yg = my + L.t[2];
  ACC* yo = my + L.t[3];
  ACC* ra = my + L.o[0];
  ACC* rb = my + L.o[1];
  ACC* rg = my + L.o[2];
  ACC* ro = my + L.o[3];
  if (valid) {
    load_row(pA + i * da, xa, da, vec);
    load_row(pB + e * db, xb, db, vec);
    load_row(pG + i * dg, xg, dg, vec);
    load_row(pO + i * do_, xo, do_, vec);
    if (hta) load_row(tA + i * da, ya, da, vec);
    if (htb) load_row(tB + e * db, yb, db, vec);
    if (htg) load_row(tG + i * dg, yg, dg, vec);
    if (hto) load_row(tO + i * do_, yo, do_, vec);
    if (om & 1) for (int k = 0; k < da; ++k) ra[k] = (ACC)0;
    if (om & 2) for (int k = 0; k < db; ++k) rb[k] = (ACC)0;
    if (om & 4) for (int k = 0; k < dg; ++k) rg[k] = (ACC)0;
    if (om & 8) for (int k = 0; k < do_; ++k) ro[k] = (ACC)0;
  }
  __syncthreads();
  if (valid && n_ent > 0) {
    // The rows of one slice never overlap, so the only LDS accesses
    // that must stay ordered are two updates of one accumulator word.
    // Entry k's accumulator reads and entry k+1's operand reads are
    // therefore issued together, ahead of entry k's accumulator
    // writes: one LDS round trip per entry instead of one per update.
    int4 q = ent_lds[0];
    ACC c = (ACC)coef_lds[0];
    ACC a = xa[q.x], b = xb[q.y], g = xg[q.z], o = xo[q.w];
    ACC va = hta ? ya[q.x] : (ACC)0, vb = htb ? yb[q.y] : (ACC)0;
    ACC vg = htg ? yg[q.z] : (ACC)0, vo = hto ? yo[q.w] : (ACC)0;
    for (int k = 0; k < n_ent; ++k) {
      const ACC sa = (om & 1) ? ra[q.x] : (ACC)0;
      const ACC sb = (om & 2) ? rb[q.y] : (ACC)0;
      const ACC sg = (om & 4) ? rg[q.z] : (ACC)0;
      const ACC so = (om & 8) ? ro[q.w] : (ACC)0;
      const int kn = k + 1 < n_ent ? k + 1 : k;
      const int4 qn = ent_lds[kn];
      const ACC cn = (ACC)coef_lds[kn];
      const ACC an = xa[qn.x], bn = xb[qn.y], gn = xg[qn.z],
                on = xo[qn.w];
      const ACC van = hta ? ya[qn.x] : (ACC)0;
      const ACC vbn = htb ? yb[qn.y] : (ACC)0;
      const ACC vgn = htg ? yg[qn.z] : (ACC)0;
      const ACC von = hto ? yo[qn.w] : (ACC)0;
      if (ORDER == 1) {
        const ACC ab = c * a * b, go = c * g * o;
        if (om & 1) ra[q.x] = sa + b * go;
        if (om & 2) rb[q.y] = sb + a * go;
        if (om & 4) rg[q.z] = sg + ab * o;
        if (om & 8) ro[q.w] = so + ab * g;
      } else {
        // products of a pair and their directional derivatives
        const ACC ab = c * a * b, dab = c * (va * b + a * vb);
        const ACC go = c * g * o, dgo = c * (vg * o + g * vo);
        if (om & 1) ra[q.x] = sa + (vb * go + b * dgo);
        if (om & 2) rb[q.y] = sb + (va * go + a * dgo);
        if (om & 4) rg[q.z] = sg + (dab * o + ab * vo);
        if (om & 8) ro[q.w] = so + (dab * g + ab * vg);
      }
      q = qn; c = cn;
      a = an; b = bn; g = gn; o = on;
      va = van; vb = vbn; vg = vgn; vo = von;
    }
  }
  if (valid) {
    if (om & 1) store_row(outA + i * da, ra, da, vec);
    if (om & 4) store_row(outG + i * dg, rg, dg, vec);
    if (om & 8) store_row(outO + i * do_, ro, do_, vec);
  }
  if (om & 2) {
    if (nch == 64) {
      // blockDim is a multiple of 64, so this wave holds row e whole
      for (int k = 0; k < db; ++k) {
        ACC v = valid ? rb[k] : (ACC)0;
        for (int off = 32; off >= 1; off >>= 1)
          v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && valid) outB[e * db + k] = (T)v;
      }
    } else if (valid) {
      for (int k = 0; k < db; ++k) atomicAdd(&outB_acc[e * db + k], rb[k]);
    }
  }
}

}  // namespace

// defined in etp_static.hip
bool etp_static_launch(long table_id, int order, int omask, int tmask,
                       at::ScalarType dtype, long rows, int nch, int da,
                       int db, int dg, int do_, const void* const prim[4],
                       const void* const tang[4], void* const outs[4],
                       bool vec);
void etp_count_generic();

static hipStream_t etp_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// HYDRAGNN_ETP_SWEEP_VEC=0 keeps element-wise row accesses (A/B aid)
static bool etp_sweep_vec() {
  static bool v = []() {
    const char* e = getenv("HYDRAGNN_ETP_SWEEP_VEC");
    return !(e && e[0] == '0');
  }();
  return v;
}

static int etp_block_size() {
  static int b = []() {
    const char* e = getenv("HYDRAGNN_ETP_BLOCK");
    int v = e ? atoi(e) : 256;
    return (v == 64 || v == 128 || v == 256 || v == 512) ? v : 256;
  }();
  return b;
}

// etp_reduce prefers larger blocks (micro-bench: 512 -> +30% BW over
// 256 on the b1024 gY shape); separately tunable.
static int etp_reduce_block_size() {
  static int b = []() {
    const char* e = getenv("HYDRAGNN_ETP_REDUCE_BLOCK");
    int v = e ? atoi(e) : 512;
    return (v == 64 || v == 128 || v == 256 || v == 512) ? v : 512;
  }();
  return b;
}

static const long* idx_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<long>() : nullptr;
}

torch::Tensor etp_general(torch::Tensor A, torch::Tensor B, torch::Tensor C,
                          torch::Tensor entries, torch::Tensor coefs,
                          torch::Tensor o_ranges, long do_,
                          c10::optional<torch::Tensor> ai,
                          c10::optional<torch::Tensor> bi,
                          c10::optional<torch::Tensor> ci,
                          long n_rows, long static_id) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous());
  TORCH_CHECK(B.is_contiguous() && C.is_contiguous());
  long E = n_rows > 0 ? n_rows : A.size(0);
  long NC = E * A.size(1);
  int nch = A.size(1);
  int da = A.size(2), db = B.size(1), dg = C.size(2);
  TORCH_CHECK(da <= 192 && db <= 192 && dg <= 192 && do_ <= 192,
              "etp dims exceed kernel limits");
  auto out = torch::empty({E, A.size(1), do_}, A.options());
  if (NC == 0) return out;
  if (static_id >= 0 && !ai.has_value() && !bi.has_value() &&
      !ci.has_value() && E == A.size(0) && B.size(0) == E &&
      C.size(0) == E && C.size(1) == nch &&
      B.scalar_type() == A.scalar_type() &&
      C.scalar_type() == A.scalar_type()) {
    // compile-time table (etp_static.hip): registers only, no LDS
    const void* prim[4] = {A.data_ptr(), B.data_ptr(), C.data_ptr(),
                           nullptr};
    const void* tang[4] = {nullptr, nullptr, nullptr, nullptr};
    void* outp[4] = {nullptr, nullptr, nullptr, out.data_ptr()};
    bool vec = etp_sweep_vec();
    for (const void* p : {prim[0], prim[1], prim[2],
                          (const void*)outp[3]})
      vec = vec && reinterpret_cast<uintptr_t>(p) % 16 == 0;
    if (etp_static_launch(static_id, 0, 8, 0, A.scalar_type(), E, nch,
                          da, db, dg, (int)do_, prim, tang, outp, vec))
      return out;
  }
  etp_count_generic();
  int n_ent = entries.size(0);
  int block = etp_block_size();
  size_t accs = A.scalar_type() == at::ScalarType::Double ? 8 : 4;
  int stride = (da + db + dg + (int)do_) | 1;
  size_t lds_full = (size_t)block * stride * accs + n_ent * 20;
  int stride_l1 = (int)do_ | 1;
  size_t lds_l1 = (size_t)block * stride_l1 * accs + n_ent * 20;
  // Variant choice (A/B'd on the default bench):
  //  - racc (r2 default): register accumulation over the
  //    output-sorted entry ranges — no LDS RMW dependency chain, no
  //    output slice in LDS.
  //  - staged (r1): full A/B/C/out slices in LDS.
  //  - L1: operands from L1, only the accumulator in LDS.
  // Fallback order by LDS budget; HYDRAGNN_ETP_VARIANT=staged|l1|racc
  // overrides.
  int stride_racc = (da + db + dg) | 1;
  size_t lds_racc = (size_t)block * stride_racc * accs + n_ent * 20 +
                    (size_t)do_ * 8;
  // Measured A/B (b1024 bench, same box): staged 30.8k g/s end-to-end
  // vs racc 29.8k — staged stays the default; racc (smaller slices)
  // is the fallback when the staged LDS budget is exceeded.
  int variant = lds_full <= 150 * 1024 ? 0
                : (lds_racc <= 150 * 1024 ? 2 : 1);
  const char* env = getenv("HYDRAGNN_ETP_VARIANT");
  if (env) {
    if (env[0] == 's') variant = 0;
    else if (env[0] == 'l') variant = 1;
    else if (env[0] == 'r') variant = 2;
  }
  size_t lds_bytes = variant == 2 ? lds_racc
                     : (variant == 1 ? lds_l1 : lds_full);
  TORCH_CHECK(lds_bytes <= 150 * 1024, "etp LDS budget exceeded");
  long blocks = (NC + block - 1) / block;
  auto orng = o_ranges.to(torch::kInt32).contiguous();
  // fp64 runs with double LDS slices (acc_of<double>); others stage fp32
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, A.scalar_type(),
      "etp_general", [&] {
        if (variant == 2) {
          hipLaunchKernelGGL(
              etp_general_racc_kernel<scalar_t>, dim3(blocks),
              dim3(block), lds_bytes, etp_stream(),
              A.data_ptr<scalar_t>(), B.data_ptr<scalar_t>(),
              C.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
              reinterpret_cast<const int4*>(entries.data_ptr<int>()),
              coefs.data_ptr<float>(),
              reinterpret_cast<const int2*>(orng.data_ptr<int>()),
              n_ent, NC, nch, da, db, dg, (int)do_,
              idx_ptr(ai), idx_ptr(bi), idx_ptr(ci));
          return;
        }
        auto kern = variant == 1 ? etp_general_l1_kernel<scalar_t>
                                 : etp_general_kernel<scalar_t>;
        hipLaunchKernelGGL(
            kern, dim3(blocks), dim3(block),
            lds_bytes, etp_stream(),
            A.data_ptr<scalar_t>(), B.data_ptr<scalar_t>(),
            C.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
            reinterpret_cast<const int4*>(entries.data_ptr<int>()),
            coefs.data_ptr<float>(), n_ent,
            NC, nch, da, db, dg, (int)do_,
            idx_ptr(ai), idx_ptr(bi), idx_ptr(ci));
      });
  return out;
}

torch::Tensor etp_nodesum(torch::Tensor A, torch::Tensor B,
                          torch::Tensor C, torch::Tensor entries,
                          torch::Tensor coefs, long do_,
                          torch::Tensor rowptr,
                          c10::optional<torch::Tensor> ai,
                          c10::optional<torch::Tensor> bi,
                          c10::optional<torch::Tensor> ci) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous());
  TORCH_CHECK(B.is_contiguous() && C.is_contiguous());
  long R = rowptr.numel() - 1;
  int nch = A.size(1);
  int da = A.size(2), db = B.size(1), dg = C.size(2);
  auto out = torch::empty({R, (long)nch, do_}, A.options());
  long RC = R * nch;
  if (RC == 0) return out;
  int n_ent = entries.size(0);
  int block = etp_block_size();
  int stride = (da + db + dg + (int)do_) | 1;
  size_t accs = A.scalar_type() == at::ScalarType::Double ? 8 : 4;
  size_t lds_bytes = (size_t)block * stride * accs + n_ent * 20;
  TORCH_CHECK(lds_bytes <= 150 * 1024, "etp LDS budget exceeded");
  long blocks = (RC + block - 1) / block;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, A.scalar_type(),
      "etp_nodesum", [&] {
        hipLaunchKernelGGL(
            etp_nodesum_kernel<scalar_t>, dim3(blocks), dim3(block),
            lds_bytes, etp_stream(),
            A.data_ptr<scalar_t>(), B.data_ptr<scalar_t>(),
            C.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
            reinterpret_cast<const int4*>(entries.data_ptr<int>()),
            coefs.data_ptr<float>(), n_ent,
            rowptr.data_ptr<long>(), R, nch, da, db, dg, (int)do_,
            idx_ptr(ai), idx_ptr(bi), idx_ptr(ci));
      });
  return out;
}

torch::Tensor etp_reduce(torch::Tensor A, torch::Tensor C, torch::Tensor D,
                         torch::Tensor entries, torch::Tensor coefs,
                         long db,
                         c10::optional<torch::Tensor> ai,
                         c10::optional<torch::Tensor> ci,
                         c10::optional<torch::Tensor> di,
                         long n_rows) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous());
  long E = n_rows > 0 ? n_rows : A.size(0);
  int nch = A.size(1);
  int da = A.size(2), dg = C.size(2), do_ = D.size(2);
  TORCH_CHECK(db <= 12, "etp_reduce db limit");
  auto out = torch::zeros(
      {E, db}, A.options().dtype(
          A.scalar_type() == at::ScalarType::Double ? torch::kDouble
                                                    : torch::kFloat));
  if (E == 0) return out.to(A.scalar_type());
  int n_ent = entries.size(0);
  int block = etp_reduce_block_size();
  int stride = (da + dg + do_ + (int)db) | 1;
  size_t accs = A.scalar_type() == at::ScalarType::Double ? 8 : 4;
  size_t lds_bytes = (size_t)block * stride * accs + n_ent * 20;
  // staged is the measured default (963 GB/s vs the L1-operand
  // variant's 381: repeated per-entry L1 hits lose to LDS reads);
  // HYDRAGNN_ETP_REDUCE_VARIANT=l1 selects the low-LDS variant for
  // over-budget shapes
  const char* rv = getenv("HYDRAGNN_ETP_REDUCE_VARIANT");
  size_t lds_l1 = (size_t)block * ((db | 1)) * accs + n_ent * 20;
  bool use_l1 = (rv && rv[0] == 'l') ||
                (lds_bytes > 150 * 1024 && lds_l1 <= 150 * 1024);
  if (use_l1)
    lds_bytes = (size_t)block * ((db | 1)) * accs + n_ent * 20;
  TORCH_CHECK(lds_bytes <= 150 * 1024, "etp_reduce LDS budget exceeded");
  long blocks = (E * nch + block - 1) / block;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, A.scalar_type(),
      "etp_reduce", [&] {
        auto kern = use_l1 ? etp_reduce_l1_kernel<scalar_t>
                           : etp_reduce_idx_kernel<scalar_t>;
        hipLaunchKernelGGL(
            kern, dim3(blocks), dim3(block),
            lds_bytes, etp_stream(), A.data_ptr<scalar_t>(),
            C.data_ptr<scalar_t>(),
            D.data_ptr<scalar_t>(), out.data_ptr<typename acc_of<scalar_t>::type>(),
            reinterpret_cast<const int4*>(entries.data_ptr<int>()),
            coefs.data_ptr<float>(), n_ent, E, nch, da, (int)db, dg, do_,
            idx_ptr(ai), idx_ptr(ci), idx_ptr(di));
      });
  return out.to(A.scalar_type());
}

// ---- sweep family host side ----------------------------------------

static int etp_sweep_block_size() {
  static int b = []() {
    const char* e = getenv("HYDRAGNN_ETP_SWEEP_BLOCK");
    int v = e ? atoi(e) : 128;
    return (v == 64 || v == 128 || v == 256 || v == 512) ? v : 128;
  }();
  return b;
}

// Dynamic-LDS bytes of one sweep block: block x (input rows + tangent
// rows + output rows) x accumulator size + staged table.  ops/etp.py
// asks this before choosing the sweep over single-output kernels.
long etp_sweep_lds_bytes(long da, long db, long dg, long do_, long n_ent,
                         long tmask, long omask, long acc_bytes) {
  SweepLayout L((int)da, (int)db, (int)dg, (int)do_, (int)tmask,
                (int)omask);
  size_t slices =
      ((size_t)etp_sweep_block_size() * L.stride * acc_bytes + 15) &
      ~(size_t)15;
  return (long)(slices + (size_t)n_ent * 20);
}

// Returns {out_a, out_b, out_g, out_o}; slots outside omask come back
// undefined (None in Python).  order 1 takes no tangents.
std::vector<torch::Tensor> etp_sweep(
    torch::Tensor A, torch::Tensor B, torch::Tensor G, torch::Tensor O,
    c10::optional<torch::Tensor> tA, c10::optional<torch::Tensor> tB,
    c10::optional<torch::Tensor> tG, c10::optional<torch::Tensor> tO,
    torch::Tensor entries, torch::Tensor coefs, long omask, long order,
    long static_id) {
  TORCH_CHECK(A.is_cuda() && A.dim() == 3 && B.dim() == 2 &&
              G.dim() == 3 && O.dim() == 3, "etp_sweep: bad ranks");
  TORCH_CHECK(order == 1 || order == 2, "etp_sweep: order is 1 or 2");
  TORCH_CHECK(omask > 0 && omask < 16, "etp_sweep: empty output mask");
  const long rows = A.size(0);
  const int nch = A.size(1);
  const int da = A.size(2), db = B.size(1), dg = G.size(2),
            do_ = O.size(2);
  TORCH_CHECK(B.size(0) == rows && G.size(0) == rows &&
              O.size(0) == rows && G.size(1) == nch && O.size(1) == nch,
              "etp_sweep: slot shapes disagree");
  TORCH_CHECK(da <= 192 && db <= 192 && dg <= 192 && do_ <= 192,
              "etp dims exceed kernel limits");
  const torch::Tensor* prim[4] = {&A, &B, &G, &O};
  const c10::optional<torch::Tensor>* tang[4] = {&tA, &tB, &tG, &tO};
  int tmask = 0;
  for (int s = 0; s < 4; ++s) {
    TORCH_CHECK(prim[s]->is_cuda() && prim[s]->is_contiguous() &&
                prim[s]->scalar_type() == A.scalar_type(),
                "etp_sweep: primals must be contiguous, one dtype");
    if (tang[s]->has_value()) {
      const torch::Tensor& t = **tang[s];
      TORCH_CHECK(order == 2, "etp_sweep: tangents need order 2");
      TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == A.scalar_type() &&
                  t.sizes() == prim[s]->sizes(),
                  "etp_sweep: tangent must match its primal");
      tmask |= 1 << s;
    }
  }
  TORCH_CHECK(entries.is_contiguous() && coefs.is_contiguous() &&
              entries.size(0) == coefs.size(0));
  const int n_ent = entries.size(0);
  const bool dbl = A.scalar_type() == at::ScalarType::Double;
  const bool direct_b = nch == 64;

  std::vector<torch::Tensor> outs(4);
  if (omask & 1) outs[0] = torch::empty_like(A);
  if (omask & 4) outs[2] = torch::empty_like(G);
  if (omask & 8) outs[3] = torch::empty_like(O);
  torch::Tensor b_acc;
  if (omask & 2) {
    if (direct_b) {
      outs[1] = torch::empty_like(B);
    } else {
      b_acc = torch::zeros(
          {rows, (long)db},
          A.options().dtype(dbl ? torch::kDouble : torch::kFloat));
    }
  }
  const long NC = rows * nch;
  bool on_static = false;
  // packed row accesses need every base on a 16-byte boundary
  bool vec = etp_sweep_vec();
  if (NC > 0) {
    auto aligned = [](const torch::Tensor& t) {
      return !t.defined() ||
             reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
    };
    for (int s = 0; s < 4; ++s) {
      vec = vec && aligned(*prim[s]) && aligned(outs[s]) &&
            (!tang[s]->has_value() || aligned(**tang[s]));
    }
    if (static_id >= 0 && direct_b) {
      // compile-time table (etp_static.hip): registers only, no LDS
      const void* pp[4];
      const void* tp[4];
      void* op[4];
      for (int s = 0; s < 4; ++s) {
        pp[s] = prim[s]->data_ptr();
        tp[s] = tang[s]->has_value() ? (*tang[s])->data_ptr() : nullptr;
        op[s] = outs[s].defined() ? outs[s].data_ptr() : nullptr;
      }
      on_static = etp_static_launch(
          static_id, (int)order, (int)omask, tmask, A.scalar_type(), rows,
          nch, da, db, dg, do_, pp, tp, op, vec);
    }
  }
  if (NC > 0 && !on_static) {
    etp_count_generic();
    const int block = etp_sweep_block_size();
    const size_t lds_bytes = (size_t)etp_sweep_lds_bytes(
        da, db, dg, do_, n_ent, tmask, omask, dbl ? 8 : 4);
    TORCH_CHECK(lds_bytes <= 150 * 1024, "etp_sweep LDS budget exceeded");
    const long blocks = (NC + block - 1) / block;
    AT_DISPATCH_FLOATING_TYPES_AND2(
        at::ScalarType::BFloat16, at::ScalarType::Half, A.scalar_type(),
        "etp_sweep", [&] {
          using ACC = typename acc_of<scalar_t>::type;
          auto tp = [&](int s) -> const scalar_t* {
            return tang[s]->has_value()
                       ? (*tang[s])->data_ptr<scalar_t>() : nullptr;
          };
          auto op = [&](int s) -> scalar_t* {
            return outs[s].defined() ? outs[s].data_ptr<scalar_t>()
                                     : nullptr;
          };
          // compile-time masks for what training launches: edge
          // products (a,b,g | all four under tangents a,b,g), folds
          // (a,g | a,g,o under tangents a,g) and etp_reduce (a,g,o)
          auto kern = order == 1 ? etp_sweep_kernel<scalar_t, 1, -1, -1>
                                 : etp_sweep_kernel<scalar_t, 2, -1, -1>;
          if (order == 1 && omask == 7)
            kern = etp_sweep_kernel<scalar_t, 1, 7, -1>;
          else if (order == 1 && omask == 5)
            kern = etp_sweep_kernel<scalar_t, 1, 5, -1>;
          else if (order == 1 && omask == 13)
            kern = etp_sweep_kernel<scalar_t, 1, 13, -1>;
          else if (order == 2 && omask == 15 && tmask == 7)
            kern = etp_sweep_kernel<scalar_t, 2, 15, 7>;
          else if (order == 2 && omask == 13 && tmask == 5)
            kern = etp_sweep_kernel<scalar_t, 2, 13, 5>;
          hipLaunchKernelGGL(
              kern, dim3(blocks), dim3(block), lds_bytes, etp_stream(),
              A.data_ptr<scalar_t>(), B.data_ptr<scalar_t>(),
              G.data_ptr<scalar_t>(), O.data_ptr<scalar_t>(),
              tp(0), tp(1), tp(2), tp(3), op(0), op(1),
              b_acc.defined() ? b_acc.data_ptr<ACC>() : nullptr,
              op(2), op(3),
              reinterpret_cast<const int4*>(entries.data_ptr<int>()),
              coefs.data_ptr<float>(), n_ent, rows, nch, da, db, dg,
              do_, (int)omask, vec);
        });
  }
  if (b_acc.defined()) outs[1] = b_acc.to(A.scalar_type());
  return outs;
}
