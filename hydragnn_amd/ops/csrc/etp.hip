// Fused equivariant tensor-product contraction kernels (CDNA4/gfx950).
//
// The MACE hot path is per-edge / per-node SMALL trilinear contractions
//   out[i, c, o] = sum_entries coef * A[i, c, a] * B[i, b] * C[i, c, g]
// (entry table = flattened Wigner-3j paths).  hipBLASLt runs these as
// tiny-batched GEMMs at ~2% of HBM bandwidth; here one kernel does the
// whole contraction: one thread per (i, c) keeps its A/B/C rows and its
// output row in a per-thread LDS slice and walks the (sorted-by-output)
// entry table, staged in LDS once per block.  VGPR use stays low (no
// runtime-indexed register arrays -> no scratch).
//
// The same kernel template (etp_form_kernel) computes every first- and
// second-order derivative of the contraction: gradients of a trilinear
// form are trilinear forms with role-permuted entry tables (see
// ops/etp.py), and the channel-reduced b-slot gradient is its b-type
// instance, so force training (create_graph=True double backward) never
// leaves this kernel family.  The sweep kernels at the end of the file
// produce several of those derivatives per launch, with every row
// staged once.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <type_traits>

#include "check_launch.h"

namespace {

// accumulator type: fp32 for bf16/half/float inputs, fp64 for double
// (fp64 ETP support: slices and channel reductions keep full width)
template <typename T> struct acc_of { using type = float; };
template <> struct acc_of<double> { using type = double; };

// ---- helpers shared by the single-output form and the sweep ---------

// Dynamic LDS of a block: one slice of `stride` accumulator words per
// thread, then the entry table (int4 + float per entry) on a 16-byte
// boundary.  Host (footprint) and device (addresses) both use this.
__host__ __device__ inline size_t slice_bytes(int block, int stride,
                                              size_t acc_bytes) {
  return ((size_t)block * stride * acc_bytes + 15) & ~(size_t)15;
}

struct StagedTable {
  const int4* ent;
  const float* coef;
};

// Copies the entry table behind the block's slices.  The caller's
// __syncthreads() publishes it; afterwards every thread walks the same
// entries in lockstep (wave-uniform LDS broadcasts, no divergence).
__device__ inline StagedTable stage_table(char* smem, size_t slices,
                                          const int4* __restrict__ entries,
                                          const float* __restrict__ coefs,
                                          int n_ent) {
  int4* ent_lds = reinterpret_cast<int4*>(smem + slices);
  float* coef_lds = reinterpret_cast<float*>(ent_lds + n_ent);
  for (int k = threadIdx.x; k < n_ent; k += blockDim.x) {
    ent_lds[k] = entries[k];
    coef_lds[k] = coefs[k];
  }
  return {ent_lds, coef_lds};
}

// Sum of v over the 64 lanes of the wave, valid in lane 0.
template <typename ACC>
__device__ inline ACC wave_sum(ACC v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Channel reduction of a b-type output: out_row[k] += acc[k] over the
// threads of one row.  With nch % 64 == 0 a wave lies inside one row:
// shuffle-reduce each k across the 64 lanes, then ONE atomic per k per
// wave; otherwise one atomic per thread (db <= 12, light contention).
// Every thread of the block calls this (the shuffles need whole waves).
template <typename ACC>
__device__ inline void channel_sum_atomic(ACC* __restrict__ out_row,
                                          const ACC* acc, int db, int nch,
                                          bool valid) {
  if (nch % 64 == 0) {
    for (int k = 0; k < db; ++k) {
      ACC v = wave_sum(valid ? acc[k] : (ACC)0);
      if ((threadIdx.x % 64) == 0 && valid) atomicAdd(&out_row[k], v);
    }
  } else if (valid) {
    for (int k = 0; k < db; ++k) atomicAdd(&out_row[k], acc[k]);
  }
}

// Row `e` of a slot tensor, through its optional row-index list.
__device__ inline long row_of(const long* __restrict__ idx, long e) {
  return idx ? idx[e] : e;
}

// ---- single-output form ---------------------------------------------
//
// One slot of Q(a,b,g,o) = sum_k coef_k a[a_k] b[b_k] g[g_k] o[o_k] out,
// the other three in:
//   o-type (B_OUT = false): out[i,c,o] = sum_k coef A[i,c,a] B[i,b] G[i,c,g]
//   b-type (B_OUT = true):  out[i,b] = sum_c sum_k coef A[i,c,a] G[i,c,g] O[i,c,o]
// in0/in1/in2 are the three input slots in slot order.  The same form
// with role-permuted tables gives every gradient (see ops/etp.py).
//
// Per-thread LDS slice, shared by host (footprint) and device: the
// staged input rows in slot order, then the output slot's accumulator
// row; odd word stride to spread LDS banks.
struct FormLayout {
  int d[3], dout, stride;
  __host__ __device__ FormLayout(int da, int db, int dg, int do_,
                                 bool b_out, bool staged) {
    d[0] = da;
    d[1] = b_out ? dg : db;
    d[2] = b_out ? do_ : dg;
    dout = b_out ? db : do_;
    stride = ((staged ? d[0] + d[1] + d[2] : 0) + dout) | 1;
  }
};

// Entry word of each role: the three inputs in slot order, the output.
template <bool B_OUT> struct Roles {
  __device__ static int in0(int4 q) { return q.x; }
  __device__ static int in1(int4 q) { return B_OUT ? q.z : q.y; }
  __device__ static int in2(int4 q) { return B_OUT ? q.w : q.z; }
  __device__ static int out(int4 q) { return B_OUT ? q.y : q.w; }
};

// One THREAD per (output row, channel): its input rows and accumulator
// live in a per-thread LDS slice (runtime entry indices would force
// register arrays to scratch otherwise); global loads/stores are
// per-thread contiguous rows -> coalesced across adjacent threads.
//
// STAGED: input rows are copied into the slice; otherwise only the
//   accumulator is in LDS and operands are read through L1 per entry
//   (each row is 1-2 hot cache lines; for shapes whose staged slices
//   exceed the LDS budget).
// CSR: the thread sums positions rowptr[r]..rowptr[r+1] of its output
//   row r, restaging each position's rows (fused gather + tensor
//   product + segment sum); otherwise position r alone.
template <typename T, bool B_OUT, bool STAGED, bool CSR>
__global__ void etp_form_kernel(
    const T* __restrict__ in0, const T* __restrict__ in1,
    const T* __restrict__ in2,
    std::conditional_t<B_OUT, typename acc_of<T>::type, T>* __restrict__ out,
    const int4* __restrict__ entries, const float* __restrict__ coefs,
    int n_ent, const long* __restrict__ rowptr, long NC, int nch, int da,
    int db, int dg, int do_, const long* __restrict__ i0,
    const long* __restrict__ i1, const long* __restrict__ i2) {
  static_assert(STAGED || !CSR, "the CSR form restages rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using ACC = typename acc_of<T>::type;
  using R = Roles<B_OUT>;
  const FormLayout L(da, db, dg, do_, B_OUT, STAGED);
  const StagedTable tab = stage_table(
      smem, slice_bytes(blockDim.x, L.stride, sizeof(ACC)), entries, coefs,
      n_ent);

  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < NC;
  const long r = i / nch;
  const int c = (int)(i - r * nch);
  ACC* m0 = reinterpret_cast<ACC*>(smem) + (size_t)threadIdx.x * L.stride;
  ACC* m1 = m0 + (STAGED ? L.d[0] : 0);
  ACC* m2 = m1 + (STAGED ? L.d[1] : 0);
  ACC* mo = m2 + (STAGED ? L.d[2] : 0);
  const T *p0 = nullptr, *p1 = nullptr, *p2 = nullptr;

  // input rows of position e: in1 of the o-type form is the per-row b
  // slot, every other input is per (row, channel)
  auto rows_at = [&](long e) {
    p0 = in0 + (row_of(i0, e) * nch + c) * L.d[0];
    p1 = in1 + (B_OUT ? row_of(i1, e) * nch + c : row_of(i1, e)) * L.d[1];
    p2 = in2 + (row_of(i2, e) * nch + c) * L.d[2];
    if (STAGED) {
      for (int k = 0; k < L.d[0]; ++k) m0[k] = (ACC)p0[k];
      for (int k = 0; k < L.d[1]; ++k) m1[k] = (ACC)p1[k];
      for (int k = 0; k < L.d[2]; ++k) m2[k] = (ACC)p2[k];
    }
  };
  // coef * x * y * z left to right, accumulated in the slice
  auto walk = [&]() {
    for (int k = 0; k < n_ent; ++k) {
      const int4 q = tab.ent[k];
      if (STAGED)
        mo[R::out(q)] +=
            tab.coef[k] * m0[R::in0(q)] * m1[R::in1(q)] * m2[R::in2(q)];
      else
        mo[R::out(q)] += tab.coef[k] * (ACC)p0[R::in0(q)] *
                         (ACC)p1[R::in1(q)] * (ACC)p2[R::in2(q)];
    }
  };

  if (valid) {
    if (!CSR) rows_at(r);
    for (int k = 0; k < L.dout; ++k) mo[k] = 0.f;
  }
  __syncthreads();
  if (valid) {
    if (CSR) {
      const long lo = rowptr[r], hi = rowptr[r + 1];
      for (long e = lo; e < hi; ++e) {
        rows_at(e);
        walk();
      }
    } else {
      walk();
    }
  }
  if constexpr (B_OUT) {
    channel_sum_atomic(out + r * L.dout, mo, L.dout, nch, valid);
  } else if (valid) {
    T* op = out + i * L.dout;
    for (int k = 0; k < L.dout; ++k) op[k] = (T)mo[k];
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
// output rows; odd word stride as in FormLayout.
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
// Same mapping as etp_form_kernel: one thread per (row, channel),
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
  const StagedTable tab = stage_table(
      smem, slice_bytes(blockDim.x, L.stride, sizeof(ACC)), entries, coefs,
      n_ent);
  const int4* ent_lds = tab.ent;
  const float* coef_lds = tab.coef;

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
        const ACC v = wave_sum(valid ? rb[k] : (ACC)0);
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

// Block size from the environment: 64, 128, 256 or 512, else `dflt`.
static int env_block(const char* name, int dflt) {
  const char* e = getenv(name);
  int v = e ? atoi(e) : dflt;
  return (v == 64 || v == 128 || v == 256 || v == 512) ? v : dflt;
}

static int etp_block_size() {
  static int b = env_block("HYDRAGNN_ETP_BLOCK", 256);
  return b;
}

// the b-type form prefers larger blocks (micro-bench: 512 -> +30% BW
// over 256 on the b1024 gY shape); separately tunable.
static int etp_reduce_block_size() {
  static int b = env_block("HYDRAGNN_ETP_REDUCE_BLOCK", 512);
  return b;
}

static int etp_sweep_block_size() {
  static int b = env_block("HYDRAGNN_ETP_SWEEP_BLOCK", 128);
  return b;
}

constexpr size_t ETP_LDS_BUDGET = 150 * 1024;

// Dynamic-LDS bytes of one block of the single-output form, at the
// block size its launcher uses: block x slice x accumulator size +
// staged table.  launch_form() and ops/etp.py both ask this.
long etp_form_lds_bytes(long da, long db, long dg, long do_, long n_ent,
                        long acc_bytes, bool b_out, bool staged) {
  FormLayout L((int)da, (int)db, (int)dg, (int)do_, b_out, staged);
  int block = b_out ? etp_reduce_block_size() : etp_block_size();
  return (long)(slice_bytes(block, L.stride, acc_bytes) +
                (size_t)n_ent * 20);
}

using OptTensor = c10::optional<torch::Tensor>;

// One launch of the single-output form over `rows` output rows; the
// argument marshalling every entry point below shares.  in[] and idx[]
// are the three input slots in slot order and their optional row-index
// lists; d[] = (da, db, dg, do).  A rowptr selects the CSR instance.
static void launch_form(const char* what, bool b_out, bool staged,
                        const torch::Tensor (&in)[3],
                        const OptTensor (&idx)[3], const OptTensor& rowptr,
                        torch::Tensor& out, const torch::Tensor& entries,
                        const torch::Tensor& coefs, long rows, int nch,
                        const int (&d)[4]) {
  TORCH_CHECK(b_out ? !rowptr.has_value() : staged, what,
              ": no such instance");
  TORCH_CHECK(entries.is_contiguous() && coefs.is_contiguous() &&
              entries.size(0) == coefs.size(0));
  const int n_ent = entries.size(0);
  const at::ScalarType dtype = in[0].scalar_type();
  const size_t lds_bytes = (size_t)etp_form_lds_bytes(
      d[0], d[1], d[2], d[3], n_ent,
      dtype == at::ScalarType::Double ? 8 : 4, b_out, staged);
  TORCH_CHECK(lds_bytes <= ETP_LDS_BUDGET, what, " LDS budget exceeded");
  const int block = b_out ? etp_reduce_block_size() : etp_block_size();
  const long NC = rows * nch;
  const long blocks = (NC + block - 1) / block;
  auto ip = [&](int s) -> const long* {
    return idx[s].has_value() ? idx[s]->data_ptr<long>() : nullptr;
  };
  // fp64 runs with double LDS slices (acc_of<double>); others stage fp32
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::BFloat16, at::ScalarType::Half, dtype, "etp_form",
      [&] {
        using ACC = typename acc_of<scalar_t>::type;
        auto launch = [&](auto kern, auto* outp) {
          hipLaunchKernelGGL(
              kern, dim3(blocks), dim3(block), lds_bytes, etp_stream(),
              in[0].data_ptr<scalar_t>(), in[1].data_ptr<scalar_t>(),
              in[2].data_ptr<scalar_t>(), outp,
              reinterpret_cast<const int4*>(entries.data_ptr<int>()),
              coefs.data_ptr<float>(), n_ent,
              rowptr.has_value() ? rowptr->data_ptr<long>() : nullptr, NC,
              nch, d[0], d[1], d[2], d[3], ip(0), ip(1), ip(2));
        };
        if (b_out && staged)
          launch(etp_form_kernel<scalar_t, true, true, false>,
                 out.data_ptr<ACC>());
        else if (b_out)
          launch(etp_form_kernel<scalar_t, true, false, false>,
                 out.data_ptr<ACC>());
        else if (rowptr.has_value())
          launch(etp_form_kernel<scalar_t, false, true, true>,
                 out.data_ptr<scalar_t>());
        else
          launch(etp_form_kernel<scalar_t, false, true, false>,
                 out.data_ptr<scalar_t>());
      });
  check_launch(what);
}

torch::Tensor etp_general(torch::Tensor A, torch::Tensor B, torch::Tensor C,
                          torch::Tensor entries, torch::Tensor coefs,
                          long do_, c10::optional<torch::Tensor> ai,
                          c10::optional<torch::Tensor> bi,
                          c10::optional<torch::Tensor> ci,
                          long n_rows, long static_id) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous());
  TORCH_CHECK(B.is_contiguous() && C.is_contiguous());
  long E = n_rows > 0 ? n_rows : A.size(0);
  int nch = A.size(1);
  const int d[4] = {(int)A.size(2), (int)B.size(1), (int)C.size(2),
                    (int)do_};
  TORCH_CHECK(d[0] <= 192 && d[1] <= 192 && d[2] <= 192 && d[3] <= 192,
              "etp dims exceed kernel limits");
  auto out = torch::empty({E, A.size(1), do_}, A.options());
  if (E * nch == 0) return out;
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
                          d[0], d[1], d[2], d[3], prim, tang, outp, vec))
      return out;
  }
  etp_count_generic();
  launch_form("etp_general", false, true, {A, B, C}, {ai, bi, ci},
              c10::nullopt, out, entries, coefs, E, nch, d);
  return out;
}

// Fused gather + tensor product + segment sum:
//   out[r, c, o] = sum_{e in rowptr[r]..rowptr[r+1]} sum_k coef_k
//                  A[ai[e], c, a] B[bi[e], b] C[ci[e], c, g]
// removes the materialized per-edge message tensor, its scatter pass,
// and the standalone node gather of the unfused pipeline.
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
  const int d[4] = {(int)A.size(2), (int)B.size(1), (int)C.size(2),
                    (int)do_};
  auto out = torch::empty({R, (long)nch, do_}, A.options());
  if (R * nch == 0) return out;
  launch_form("etp_nodesum", false, true, {A, B, C}, {ai, bi, ci}, rowptr,
              out, entries, coefs, R, nch, d);
  return out;
}

// out[e,b] = sum_c sum_k coef A[ai[e],c,a] C[ci[e],c,g] D[di[e],c,o]
// (the B-slot gradient).  The kernel adds into a zeroed accumulator
// buffer; one cast to the input dtype follows.
torch::Tensor etp_reduce(torch::Tensor A, torch::Tensor C, torch::Tensor D,
                         torch::Tensor entries, torch::Tensor coefs,
                         long db,
                         c10::optional<torch::Tensor> ai,
                         c10::optional<torch::Tensor> ci,
                         c10::optional<torch::Tensor> di,
                         long n_rows) {
  TORCH_CHECK(A.is_cuda() && A.is_contiguous());
  TORCH_CHECK(C.is_contiguous() && D.is_contiguous());
  long E = n_rows > 0 ? n_rows : A.size(0);
  int nch = A.size(1);
  const int d[4] = {(int)A.size(2), (int)db, (int)C.size(2),
                    (int)D.size(2)};
  TORCH_CHECK(db <= 12, "etp_reduce db limit");
  const bool dbl = A.scalar_type() == at::ScalarType::Double;
  auto out = torch::zeros(
      {E, db}, A.options().dtype(dbl ? torch::kDouble : torch::kFloat));
  if (E * nch == 0) return out.to(A.scalar_type());
  // staged is the measured default (963 GB/s vs the L1-operand
  // instance's 381: repeated per-entry L1 hits lose to LDS reads); the
  // L1 instance takes shapes whose staged slices exceed the budget, and
  // every shape under HYDRAGNN_ETP_REDUCE_VARIANT=l1
  const char* rv = getenv("HYDRAGNN_ETP_REDUCE_VARIANT");
  const long n_ent = entries.size(0);
  const bool staged =
      !(rv && rv[0] == 'l') &&
      (size_t)etp_form_lds_bytes(d[0], d[1], d[2], d[3], n_ent,
                                 dbl ? 8 : 4, true, true) <= ETP_LDS_BUDGET;
  launch_form("etp_reduce", true, staged, {A, C, D}, {ai, ci, di},
              c10::nullopt, out, entries, coefs, E, nch, d);
  return out.to(A.scalar_type());
}

// ---- sweep family host side ----------------------------------------

// Dynamic-LDS bytes of one sweep block: block x (input rows + tangent
// rows + output rows) x accumulator size + staged table.  ops/etp.py
// asks this before choosing the sweep over single-output kernels.
long etp_sweep_lds_bytes(long da, long db, long dg, long do_, long n_ent,
                         long tmask, long omask, long acc_bytes) {
  SweepLayout L((int)da, (int)db, (int)dg, (int)do_, (int)tmask,
                (int)omask);
  return (long)(slice_bytes(etp_sweep_block_size(), L.stride, acc_bytes) +
                (size_t)n_ent * 20);
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
    TORCH_CHECK(lds_bytes <= ETP_LDS_BUDGET,
                "etp_sweep LDS budget exceeded");
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
    check_launch("etp_sweep");
  }
  if (b_acc.defined()) outs[1] = b_acc.to(A.scalar_type());
  return outs;
}
