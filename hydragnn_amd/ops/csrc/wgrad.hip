// Tall-skinny weight gradient (gfx950):
//
//   gW[n, k] = sum_e g[e, n] x[e, k]      gb[n] = sum_e g[e, n]
//
// for x [E, K] and g [E, N] row-major, 1 <= N, K <= 256 and E in the
// millions: the dW = g^T x of a per-edge or per-triplet nn.Linear.  The
// output is a handful of 16 x 16 tiles and the contraction is all of E, so
// the work is split over E, not over the output.
//
// Split.  E is cut into chunks of `rows` rows, a count and a length that
// come from the shapes alone (wgrad_split).  Block (chunk, panel) writes
// the partial [N, K] sum of its chunk for its panel of output tiles, and
// the bias partial where the panel starts at k = 0; a second kernel adds
// the partials in a fixed two-level order.  No atomics: equal inputs give
// equal bits.
//
// Staging.  The R rows of a stage are one contiguous span of R K (R N)
// elements of x (g).  The span is copied flat into LDS: scalar loads up
// to the first 16-byte boundary (the head) and after the last (the tail),
// 16-byte loads in between, element f of the span at LDS index m + f with
// m the misalignment of the span start in elements, so the 16-byte LDS
// stores are aligned too.  No row or column arithmetic, whatever the
// width.  bf16 and f16 become fp32 on the way.  The loads of stage s + 1
// are in flight in registers while the MFMAs of stage s run, and the two
// LDS buffers alternate, so a stage costs one barrier.
//
// MFMA.  v_mfma_f64_16x16x4_f64 for fp64, v_mfma_f32_16x16x4_f32 for the
// rest.  Lane l feeds A[l % 16][l / 16] = g[row l / 16][n0 + l % 16] and
// B[l / 16][l % 16] = x[row l / 16][k0 + l % 16]: both fragments are 16
// consecutive LDS elements per row and come straight from the flat image.
// Columns past N or K and rows past the chunk read as zero by a select on
// the fragment.  A wave holds WN x WK tiles in registers and reads WN + WK
// fragments for WN WK MFMAs; the four waves are a 2 x 2 grid over a panel
// of 2 WN x 2 WK tiles.  With four tiles or fewer (8 x 42, 64 x 8) every
// wave takes all the tiles and a quarter of the k steps, and the four
// results are added through LDS in wave order.
//
// Bias.  The A fragment is g itself, so gb is a VALU add per A fragment in
// the same loop, closed by a fixed shuffle tree over the four lane groups.
//
// A native 16x16x32 MFMA body for the half types is not here: they run the
// fp32 body (their products are exact in fp32).

#include <torch/extension.h>
#include <ATen/Dispatch.h>
#include <ATen/OpMathType.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "segment_common.h"

namespace {

using segment::Bits;
using segment::Pack;

constexpr int kThreads = 256;
constexpr int kStageBytes = 16384;   // one operand of one stage, in LDS
constexpr int kLdsPad = 8;           // elements: room for the misalignment
constexpr int kMaxWidth = 256;
constexpr int kMaxStageRows = 128;
constexpr long kMinRows = 256;       // rows of a chunk, at least
constexpr long kBlocksTarget = 512;  // two blocks on each of 256 CUs
constexpr long kMinChunkCap = 32;

template <typename ACC> struct Mfma;
template <> struct Mfma<float> {
  using frag = __attribute__((ext_vector_type(4))) float;
  static __device__ __forceinline__ frag run(float a, float b, frag c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // register r of lane l holds D[row(l, r)][l % 16]
  static __device__ __forceinline__ int row(int lane, int r) {
    return (lane >> 4) * 4 + r;
  }
};
template <> struct Mfma<double> {
  using frag = __attribute__((ext_vector_type(4))) double;
  static __device__ __forceinline__ frag run(double a, double b, frag c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) {
    return r * 4 + (lane >> 4);
  }
};

// One operand's span of one stage, on its way from memory to LDS.
template <typename T>
struct Stager {
  using ACC = at::opmath_type<T>;
  static constexpr int V = 16 / sizeof(T);          // elements of a load
  static constexpr int CAP = kStageBytes / sizeof(ACC);
  static constexpr int VPT = CAP / V / kThreads;    // 16-byte loads a thread
  static constexpr int AV = 16 / sizeof(ACC);       // elements of a store
  using P = Pack<T, V>;
  using U = typename segment::UIntOf<sizeof(T)>::type;
  using S = __attribute__((ext_vector_type(AV))) ACC;
  static_assert(VPT >= 1 && V <= kLdsPad, "stage geometry");

  P body[VPT];
  U edge;
  int m, h, nfull, len;

  // threads [0, V) own the head, [V, 2 V) the tail
  __device__ __forceinline__ int edge_elem(int tid) const {
    return tid < V ? tid : h + nfull * V + (tid - V);
  }
  __device__ __forceinline__ bool edge_ok(int tid) const {
    return tid < V ? tid < h : (tid < 2 * V && edge_elem(tid) < len);
  }

  __device__ __forceinline__ void load(const T* __restrict__ p, int n,
                                       int tid) {
    len = n;
    m = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) % V);
    h = (V - m) % V;
    if (h > len) h = len;
    nfull = (len - h) / V;
    const P* __restrict__ pv = reinterpret_cast<const P*>(p + h);
    for (int i = 0; i < VPT; ++i) {
      int j = tid + i * kThreads;
      if (j < nfull) body[i] = pv[j];
    }
    edge = 0;
    if (edge_ok(tid))
      edge = reinterpret_cast<const U*>(p)[edge_elem(tid)];
  }

  // element f of the span -> lds[m + f]
  __device__ __forceinline__ void store(ACC* __restrict__ lds, int tid) const {
    for (int i = 0; i < VPT; ++i) {
      int j = tid + i * kThreads;
      if (j < nfull) {
        S* dst = reinterpret_cast<S*>(lds + m + h + V * j);
        for (int q = 0; q < V / AV; ++q) {
          S s;
          for (int t = 0; t < AV; ++t)
            s[t] = segment::ld<ACC>(body[i], q * AV + t);
          dst[q] = s;
        }
      }
    }
    if (edge_ok(tid)) lds[m + edge_elem(tid)] = Bits<T>::get(edge);
  }
};

// partW[chunk, n, k] and partB[chunk, n] of one chunk of E.  SPLIT: the
// block owns WN x WK tiles at the origin and its waves share the k steps;
// otherwise it owns panel blockIdx.y of 2 WN x 2 WK tiles.
template <typename T, int WN, int WK, bool SPLIT>
__global__ __launch_bounds__(kThreads) void wgrad_partial_kernel(
    const T* __restrict__ G, const T* __restrict__ X,
    at::opmath_type<T>* __restrict__ partW,
    at::opmath_type<T>* __restrict__ partB, long E, int N, int K, long rows,
    int R, int npk) {
  using ACC = at::opmath_type<T>;
  using M = Mfma<ACC>;
  using St = Stager<T>;
  using frag = typename M::frag;
  constexpr int BUF = St::CAP + kLdsPad;
  extern __shared__ __align__(16) unsigned char wgrad_lds[];
  ACC* lds = reinterpret_cast<ACC*>(wgrad_lds);   // [2][g | x][BUF]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long chunk = blockIdx.x;
  const int pn = SPLIT ? 0 : (int)blockIdx.y / npk;
  const int pk = SPLIT ? 0 : (int)blockIdx.y % npk;
  const int wn = SPLIT ? 0 : wave >> 1;
  const int wk = SPLIT ? 0 : wave & 1;
  const int n0 = ((pn * 2 + wn) * WN) * 16;
  const int k0 = ((pk * 2 + wk) * WK) * 16;
  const long e0 = chunk * rows;
  const long e1 = e0 + rows < E ? e0 + rows : E;
  const int nrows = e1 > e0 ? (int)(e1 - e0) : 0;
  const int nstages = (nrows + R - 1) / R;

  // this lane's column of each fragment, clamped, and whether it exists
  int gc[WN], xc[WK];
  bool gm[WN], xm[WK];
  for (int i = 0; i < WN; ++i) {
    int n = n0 + i * 16 + (lane & 15);
    gm[i] = n < N;
    gc[i] = gm[i] ? n : N - 1;
  }
  for (int j = 0; j < WK; ++j) {
    int k = k0 + j * 16 + (lane & 15);
    xm[j] = k < K;
    xc[j] = xm[j] ? k : K - 1;
  }

  frag acc[WN][WK];
  ACC bs[WN];
  for (int i = 0; i < WN; ++i) {
    bs[i] = 0;
    for (int j = 0; j < WK; ++j) acc[i][j] = {0, 0, 0, 0};
  }

  St sg, sx;
  if (nstages > 0) {
    int v = nrows < R ? nrows : R;
    sg.load(G + e0 * N, v * N, tid);
    sx.load(X + e0 * K, v * K, tid);
  }
  for (int s = 0; s < nstages; ++s) {
    ACC* lg = lds + (s & 1) * 2 * BUF;
    ACC* lx = lg + BUF;
    const ACC* pg = lg + sg.m;
    const ACC* px = lx + sx.m;
    sg.store(lg, tid);
    sx.store(lx, tid);
    // the one barrier of a stage: the buffer written next was last read
    // two stages ago, before the barrier of the stage in between
    __syncthreads();
    const int left = nrows - s * R;
    const int valid = left < R ? left : R;
    if (s + 1 < nstages) {
      int v = left - R < R ? left - R : R;
      long e = e0 + (long)(s + 1) * R;
      sg.load(G + e * N, v * N, tid);
      sx.load(X + e * K, v * K, tid);
    }
    for (int ks = SPLIT ? wave : 0; ks * 4 < valid; ks += SPLIT ? 4 : 1) {
      const int row = ks * 4 + (lane >> 4);
      const bool rv = row < valid;
      ACC a[WN], b[WK];
      for (int i = 0; i < WN; ++i) {
        ACC v = pg[row * N + gc[i]];
        a[i] = rv && gm[i] ? v : (ACC)0;
        bs[i] += a[i];
      }
      for (int j = 0; j < WK; ++j) {
        ACC v = px[row * K + xc[j]];
        b[j] = rv && xm[j] ? v : (ACC)0;
      }
      for (int i = 0; i < WN; ++i)
        for (int j = 0; j < WK; ++j)
          acc[i][j] = M::run(a[i], b[j], acc[i][j]);
    }
  }

  ACC* outW = partW + chunk * N * K;
  ACC* outB = partB != nullptr ? partB + chunk * N : nullptr;
  if constexpr (!SPLIT) {
    for (int i = 0; i < WN; ++i)
      for (int j = 0; j < WK; ++j)
        for (int r = 0; r < 4; ++r) {
          int n = n0 + i * 16 + M::row(lane, r);
          int k = k0 + j * 16 + (lane & 15);
          if (n < N && k < K) outW[n * K + k] = acc[i][j][r];
        }
    // lane groups 0 + 1 and 2 + 3, then the two pairs
    for (int i = 0; i < WN; ++i) {
      ACC v = bs[i] + __shfl_xor(bs[i], 16);
      v = v + __shfl_xor(v, 32);
      if (outB != nullptr && pk == 0 && wk == 0 && lane < 16 && gm[i])
        outB[n0 + i * 16 + lane] = v;
    }
  } else {
    // red[wave][slot][lane]: 4 slots per tile, then one per bias fragment
    constexpr int SLOTS = WN * WK * 4 + WN;
    static_assert(4 * SLOTS * 64 <= 4 * BUF, "the combine fits the stages");
    __syncthreads();   // every wave is done with the stage buffers
    ACC* red = lds + wave * SLOTS * 64;
    for (int i = 0; i < WN; ++i) {
      for (int j = 0; j < WK; ++j)
        for (int r = 0; r < 4; ++r)
          red[((i * WK + j) * 4 + r) * 64 + lane] = acc[i][j][r];
      red[(WN * WK * 4 + i) * 64 + lane] = bs[i];
    }
    __syncthreads();
    for (int idx = tid; idx < SLOTS * 64; idx += kThreads) {
      const int slot = idx >> 6, ln = idx & 63;
      if (slot < WN * WK * 4) {
        ACC v = lds[idx];
        for (int w = 1; w < 4; ++w) v += lds[w * SLOTS * 64 + idx];
        int t = slot >> 2, r = slot & 3;
        int n = (t / WK) * 16 + M::row(ln, r);
        int k = (t % WK) * 16 + (ln & 15);
        if (n < N && k < K) outW[n * K + k] = v;
      } else if (ln < 16 && outB != nullptr) {
        // waves in order, the four lane groups in order within a wave
        ACC v = 0;
        for (int w = 0; w < 4; ++w)
          for (int q = 0; q < 4; ++q)
            v += lds[w * SLOTS * 64 + (slot << 6) + q * 16 + ln];
        int n = (slot - WN * WK * 4) * 16 + ln;
        if (n < N) outB[n] = v;
      }
    }
  }
}

// out = sum of the partials, in a fixed order of two levels: the chunks
// are cut into RG consecutive ranges (a function of the chunk count
// alone), a range is added in ascending chunk order, the RG range sums in
// ascending range order.  A block owns 32 consecutive outputs; thread
// (range, output) = (tid >> 5, tid & 31).  The first nk outputs are the
// weight gradient, the next n the bias gradient.
constexpr int RG = 8;

template <typename ACC>
__global__ __launch_bounds__(32 * RG) void wgrad_reduce_kernel(
    const ACC* __restrict__ partW, const ACC* __restrict__ partB,
    ACC* __restrict__ gW, ACC* __restrict__ gb, long chunks, int nk, int n) {
  __shared__ ACC part[RG][32];
  const int o = threadIdx.x & 31;
  const int r = threadIdx.x >> 5;
  const int idx = blockIdx.x * 32 + o;
  const ACC* src = nullptr;
  ACC* dst = nullptr;
  int stride = 0;
  if (idx < nk) {
    src = partW + idx; dst = gW + idx; stride = nk;
  } else if (partB != nullptr && idx < nk + n) {
    src = partB + (idx - nk); dst = gb + (idx - nk); stride = n;
  }
  const long per = (chunks + RG - 1) / RG;
  long c = r * per;
  const long c_end = c + per < chunks ? c + per : chunks;
  ACC s = 0;
  if (src != nullptr) {
    for (; c + 4 <= c_end; c += 4) {
      ACC v[4];
      for (int t = 0; t < 4; ++t) v[t] = src[(c + t) * stride];
      for (int t = 0; t < 4; ++t) s += v[t];
    }
    for (; c < c_end; ++c) s += src[c * stride];
  }
  part[r][o] = s;
  __syncthreads();
  if (r == 0 && dst != nullptr) {
    ACC t = part[0][o];
    for (int q = 1; q < RG; ++q) t += part[q][o];
    *dst = t;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// How the output tiles go to blocks and waves: a function of N and K.
struct Tiling {
  bool split;      // four tiles or fewer: the waves share the rows
  int wn, wk;      // tiles of a wave
  int npn, npk;    // panels of a launch
};

// t tiles along one side -> (panels, tiles of a wave): a panel is two
// waves wide and a wave at most four tiles
void side(int t, int& panels, int& w) {
  panels = (t + 7) / 8;
  w = (t + 2 * panels - 1) / (2 * panels);
}

Tiling tiling(long N, long K) {
  int tn = (int)(N + 15) / 16, tk = (int)(K + 15) / 16;
  Tiling t;
  t.split = tn * tk <= 4;
  if (t.split) {
    t.wn = tn; t.wk = tk; t.npn = t.npk = 1;
  } else {
    side(tn, t.npn, t.wn);
    side(tk, t.npk, t.wk);
  }
  return t;
}

struct Split {
  long chunks, rows;
};

// the split of E: a function of (E, N, K) alone
Split wgrad_split(long E, long N, long K) {
  if (E <= 0) return {0, kMinRows};
  Tiling t = tiling(N, K);
  long cap = std::max(kMinChunkCap, kBlocksTarget / (t.npn * t.npk));
  // chunks of kMinRows rows until there are `cap` of them, then `cap`
  // chunks that grow: the count never falls as E rises.  A chunk past
  // the end of E (rounding can leave some) writes zeros.
  long chunks = std::min(cap, (E + kMinRows - 1) / kMinRows);
  return {chunks, std::max(kMinRows, (E + chunks - 1) / chunks)};
}

void check_envelope(long E, long N, long K) {
  TORCH_CHECK(N >= 1 && K >= 1 && N <= kMaxWidth && K <= kMaxWidth &&
                  E >= 0 && E < (1L << 31),
              "linear_wgrad envelope: 1 <= N, K <= ", kMaxWidth,
              " and 0 <= E < 2^31; got E=", E, " N=", N, " K=", K);
}

template <typename T, int WN, int WK, bool SPLIT>
void launch_partial(const T* g, const T* x, at::opmath_type<T>* pw,
                    at::opmath_type<T>* pb, long E, int N, int K,
                    const Split& sp, const Tiling& t, hipStream_t stream) {
  using St = Stager<T>;
  using ACC = at::opmath_type<T>;
  // rows of a stage: the largest power of two whose span fits
  int R = 4;
  while (R < kMaxStageRows && 2 * R * std::max(N, K) <= St::CAP) R *= 2;
  size_t lds = 4 * (size_t)(St::CAP + kLdsPad) * sizeof(ACC);
  dim3 grid((unsigned)sp.chunks, (unsigned)(t.npn * t.npk));
  hipLaunchKernelGGL((wgrad_partial_kernel<T, WN, WK, SPLIT>), grid,
                     dim3(kThreads), lds, stream, g, x, pw, pb, E, N, K,
                     sp.rows, R, t.npk);
  check_launch("linear_wgrad");
}

template <typename T, int WN>
void pick_wk(const Tiling& t, const T* g, const T* x, at::opmath_type<T>* pw,
             at::opmath_type<T>* pb, long E, int N, int K, const Split& sp,
             hipStream_t stream) {
#define WGRAD_CASE(WK_)                                                      \
  case WK_:                                                                  \
    if constexpr (WN * WK_ <= 4) {                                           \
      if (t.split)                                                           \
        return launch_partial<T, WN, WK_, true>(g, x, pw, pb, E, N, K, sp,   \
                                                t, stream);                  \
    }                                                                        \
    return launch_partial<T, WN, WK_, false>(g, x, pw, pb, E, N, K, sp, t,   \
                                             stream);
  switch (t.wk) {
    WGRAD_CASE(1)
    WGRAD_CASE(2)
    WGRAD_CASE(3)
    WGRAD_CASE(4)
    default: TORCH_CHECK(false, "linear_wgrad: ", t.wk, " tiles a wave");
  }
#undef WGRAD_CASE
}

}  // namespace

long linear_wgrad_chunks(long E, long N, long K) {
  check_envelope(E, N, K);
  return wgrad_split(E, N, K).chunks;
}

long linear_wgrad_chunk_rows(long E, long N, long K) {
  check_envelope(E, N, K);
  return wgrad_split(E, N, K).rows;
}

// -> (gW [N, K], gb [N] or an empty tensor), in the accumulator dtype
std::vector<torch::Tensor> linear_wgrad(torch::Tensor g, torch::Tensor x,
                                        bool want_bias) {
  TORCH_CHECK(g.is_cuda() && x.is_cuda() && g.dim() == 2 && x.dim() == 2 &&
                  g.size(0) == x.size(0) &&
                  g.scalar_type() == x.scalar_type(),
              "linear_wgrad: g [E, N] and x [E, K] of one dtype on the device");
  const long E = g.size(0), N = g.size(1), K = x.size(1);
  check_envelope(E, N, K);
  g = g.contiguous();
  x = x.contiguous();
  std::vector<torch::Tensor> out;
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::ScalarType::Half, at::ScalarType::BFloat16, g.scalar_type(),
      "linear_wgrad", [&] {
        using ACC = at::opmath_type<scalar_t>;
        auto aopt = g.options().dtype(c10::CppTypeToScalarType<ACC>::value);
        if (E == 0) {
          out = {torch::zeros({N, K}, aopt),
                 torch::zeros({want_bias ? N : 0}, aopt)};
          return;
        }
        const Split sp = wgrad_split(E, N, K);
        const Tiling t = tiling(N, K);
        auto gW = torch::empty({N, K}, aopt);
        auto gb = torch::empty({want_bias ? N : 0}, aopt);
        auto partW = torch::empty({sp.chunks, N, K}, aopt);
        auto partB = torch::empty({want_bias ? sp.chunks : 0, N}, aopt);
        ACC* pb = want_bias ? partB.data_ptr<ACC>() : nullptr;
        auto stream = at::hip::getCurrentHIPStream().stream();
        const scalar_t* gp = g.data_ptr<scalar_t>();
        const scalar_t* xp = x.data_ptr<scalar_t>();
        ACC* pw = partW.data_ptr<ACC>();
        switch (t.wn) {
          case 1: pick_wk<scalar_t, 1>(t, gp, xp, pw, pb, E, N, K, sp, stream);
            break;
          case 2: pick_wk<scalar_t, 2>(t, gp, xp, pw, pb, E, N, K, sp, stream);
            break;
          case 3: pick_wk<scalar_t, 3>(t, gp, xp, pw, pb, E, N, K, sp, stream);
            break;
          case 4: pick_wk<scalar_t, 4>(t, gp, xp, pw, pb, E, N, K, sp, stream);
            break;
          default: TORCH_CHECK(false, "linear_wgrad: ", t.wn, " tiles a wave");
        }
        const int nk = (int)(N * K), nb = want_bias ? (int)N : 0;
        hipLaunchKernelGGL(wgrad_reduce_kernel<ACC>,
                           dim3((nk + nb + 31) / 32), dim3(32 * RG), 0, stream,
                           (const ACC*)pw, (const ACC*)pb, gW.data_ptr<ACC>(),
                           want_bias ? gb.data_ptr<ACC>() : nullptr,
                           sp.chunks, nk, (int)N);
        check_launch("linear_wgrad_reduce");
        out = {gW, gb};
      });
  return out;
}
