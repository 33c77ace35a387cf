// Graph-tiled radius neighbor enumeration, open + periodic, fp32/fp64
// (gfx950).
//
// Replaces the r1 fp32-only brute kernels and the CPU/numpy PBC path
// (science configs run fp64 and 1k+ atom periodic cells).
// Distances are computed in the POSITION dtype — no fp32 cast, so
// boundary-edge membership is deterministic for fp64 datasets.
//
// Tiling: one workgroup per (dst-block, graph); candidate j-atoms are
// staged through LDS in 256-atom tiles so each j position is read from
// HBM once per block instead of once per thread.  PBC loops the shift
// images (precomputed integer shifts x cell, passed as cartesian
// offsets) inside the j-tile loop.  count + fill two-pass for exact
// allocation and deterministic dst-major edge order.
//
// Reference behavior matched: hydragnn/preprocess (radius_graph /
// radius_graph_pbc with vesin), torch_cluster.radius contract.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

namespace {

constexpr int RB = 256;  // threads per block == j-tile size

template <typename T>
__global__ __launch_bounds__(RB) void radius_tiled_kernel(
    const T* __restrict__ pos,         // [N, 3]
    const long* __restrict__ graph_of, // [N]
    const long* __restrict__ gptr,     // [G+1]
    const T* __restrict__ shifts,      // [S, 3] cartesian (PBC) or null
    int S,                             // #images (1 with null shifts)
    long N, T r2, bool loop,
    const long* __restrict__ offs,     // write offsets [N] (fill) or null
    int* __restrict__ count,           // [N] (count pass)
    long* __restrict__ src_out, long* __restrict__ dst_out,
    T* __restrict__ dist_out, long* __restrict__ simg_out) {
  __shared__ T lx[RB], ly[RB], lz[RB];

  const long i = (long)blockIdx.x * RB + threadIdx.x;
  const bool active = i < N;
  long g = 0, lo = 0, hi = 0;
  T xi = 0, yi = 0, zi = 0;
  if (active) {
    g = graph_of[i];
    lo = gptr[g];
    hi = gptr[g + 1];
    xi = pos[i * 3];
    yi = pos[i * 3 + 1];
    zi = pos[i * 3 + 2];
  }
  // all threads in the block belong to dst atoms in a contiguous index
  // range; their graphs may differ at block boundaries, so tile over
  // the union range of the block
  __shared__ long blo, bhi;
  if (threadIdx.x == 0) { blo = (long)1e18; bhi = 0; }
  __syncthreads();
  if (active) {
    atomicMin((unsigned long long*)&blo, (unsigned long long)lo);
    atomicMax((unsigned long long*)&bhi, (unsigned long long)hi);
  }
  __syncthreads();

  int c = 0;
  long w = (active && offs != nullptr) ? offs[i] : 0;
  for (long t0 = blo; t0 < bhi; t0 += RB) {
    long j = t0 + threadIdx.x;
    if (j < bhi) {
      lx[threadIdx.x] = pos[j * 3];
      ly[threadIdx.x] = pos[j * 3 + 1];
      lz[threadIdx.x] = pos[j * 3 + 2];
    }
    __syncthreads();
    if (active) {
      long jlo = lo > t0 ? lo : t0;
      long jhi = hi < t0 + RB ? hi : t0 + RB;
      for (long j2 = jlo; j2 < jhi; ++j2) {
        int sj = (int)(j2 - t0);
        T xj = lx[sj], yj = ly[sj], zj = lz[sj];
        for (int s = 0; s < S; ++s) {
          T sx = 0, sy = 0, sz = 0;
          bool zero_shift = true;
          if (shifts != nullptr) {
            sx = shifts[s * 3];
            sy = shifts[s * 3 + 1];
            sz = shifts[s * 3 + 2];
            zero_shift = (sx == (T)0 && sy == (T)0 && sz == (T)0);
          }
          if (!loop && j2 == i && zero_shift) continue;
          T dx = xj + sx - xi, dy = yj + sy - yi, dz = zj + sz - zi;
          T d2 = dx * dx + dy * dy + dz * dz;
          if (d2 <= r2) {
            if (offs == nullptr) {
              ++c;
            } else {
              src_out[w] = j2;
              dst_out[w] = i;
              dist_out[w] = sqrt(d2);
              if (simg_out != nullptr) simg_out[w] = s;
              ++w;
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (active && offs == nullptr) count[i] = c;
}

}  // namespace

// (src, dst, dist[, shift_image]) with dst-major ordering.  shifts:
// optional [S, 3] cartesian image offsets (applied to the SRC atom:
// vec = pos[src] + shift - pos[dst]... see Python wrapper for the
// sign convention used by edge vectors).
std::vector<torch::Tensor> radius_pairs_t(torch::Tensor pos,
                                          torch::Tensor batch,
                                          torch::Tensor gptr, double r,
                                          bool loop,
                                          c10::optional<torch::Tensor> shifts) {
  TORCH_CHECK(pos.is_cuda() && pos.is_contiguous());
  TORCH_CHECK(pos.scalar_type() == at::ScalarType::Float ||
              pos.scalar_type() == at::ScalarType::Double,
              "radius_pairs_t: fp32/fp64 positions only");
  long N = pos.size(0);
  auto b = batch.contiguous();
  auto gp = gptr.contiguous();
  auto stream = at::hip::getCurrentHIPStream().stream();
  int S = 1;
  torch::Tensor sh;
  bool has_sh = shifts.has_value() && shifts->numel() > 0;
  if (has_sh) {
    sh = shifts->to(pos.scalar_type()).contiguous();
    S = (int)sh.size(0);
  }
  auto count = torch::zeros({N}, pos.options().dtype(torch::kInt));
  long blocks = (N + RB - 1) / RB;
  if (N == 0) blocks = 1;

  AT_DISPATCH_FLOATING_TYPES(pos.scalar_type(), "radius_pairs_t", [&] {
    hipLaunchKernelGGL((radius_tiled_kernel<scalar_t>), dim3(blocks),
                       dim3(RB), 0, stream, pos.data_ptr<scalar_t>(),
                       b.data_ptr<long>(), gp.data_ptr<long>(),
                       has_sh ? sh.data_ptr<scalar_t>() : nullptr, S, N,
                       (scalar_t)(r * r), loop, nullptr,
                       count.data_ptr<int>(), nullptr, nullptr, nullptr,
                       nullptr);
  });
  auto offs = torch::zeros({N}, pos.options().dtype(torch::kLong));
  auto csum = count.to(torch::kLong).cumsum(0);
  if (N > 1) offs.slice(0, 1, N).copy_(csum.slice(0, 0, N - 1));
  long E = N > 0 ? csum[-1].item<long>() : 0;
  auto src = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dst = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dist = torch::empty({E}, pos.options());
  auto simg = has_sh ? torch::empty({E}, pos.options().dtype(torch::kLong))
                     : torch::empty({0}, pos.options().dtype(torch::kLong));
  if (E > 0) {
    AT_DISPATCH_FLOATING_TYPES(pos.scalar_type(), "radius_pairs_t_f", [&] {
      hipLaunchKernelGGL((radius_tiled_kernel<scalar_t>), dim3(blocks),
                         dim3(RB), 0, stream, pos.data_ptr<scalar_t>(),
                         b.data_ptr<long>(), gp.data_ptr<long>(),
                         has_sh ? sh.data_ptr<scalar_t>() : nullptr, S,
                         N, (scalar_t)(r * r), loop,
                         offs.data_ptr<long>(), nullptr,
                         src.data_ptr<long>(), dst.data_ptr<long>(),
                         dist.data_ptr<scalar_t>(),
                         has_sh ? simg.data_ptr<long>() : nullptr);
    });
  }
  return {src, dst, dist, simg};
}

namespace {

// Cell-list pair enumeration for LARGE graphs (10k+ atoms, open
// boundary): atoms pre-sorted by cell id (host does the argsort),
// cells are cubes of edge slightly above r (the host states the margin
// that keeps every accepted pair at most one cell apart); each atom
// scans the 27 neighbor cells' contiguous atom ranges.
// O(N * 27 * atoms/cell) instead of O(N^2).
template <typename T>
__global__ __launch_bounds__(RB) void radius_cells_kernel(
    const T* __restrict__ pos,          // [N, 3] (original order)
    const long* __restrict__ order,     // [N] sorted-by-cell atom ids
    const long* __restrict__ cell_of,   // [N] cell id per SORTED slot
    const long* __restrict__ cell_start,// [C+1] ranges into sorted ids
    int ncx, int ncy, int ncz,
    long N, T r2, bool loop,
    const long* __restrict__ offs,      // fill pass or null
    int* __restrict__ count,
    long* __restrict__ src_out, long* __restrict__ dst_out,
    T* __restrict__ dist_out) {
  long s = (long)blockIdx.x * RB + threadIdx.x;   // sorted slot
  if (s >= N) return;
  long i = order[s];                               // original id
  T xi = pos[i * 3], yi = pos[i * 3 + 1], zi = pos[i * 3 + 2];
  long cid = cell_of[s];
  int cz = (int)(cid % ncz);
  int cy = (int)((cid / ncz) % ncy);
  int cx = (int)(cid / ((long)ncz * ncy));
  int c = 0;
  long w = (offs != nullptr) ? offs[s] : 0;
  for (int dx = -1; dx <= 1; ++dx) {
    int nx = cx + dx;
    if (nx < 0 || nx >= ncx) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      int ny = cy + dy;
      if (ny < 0 || ny >= ncy) continue;
      for (int dz = -1; dz <= 1; ++dz) {
        int nz = cz + dz;
        if (nz < 0 || nz >= ncz) continue;
        long nc = ((long)nx * ncy + ny) * ncz + nz;
        for (long t = cell_start[nc]; t < cell_start[nc + 1]; ++t) {
          long j = order[t];
          if (!loop && j == i) continue;
          T ddx = pos[j * 3] - xi, ddy = pos[j * 3 + 1] - yi,
            ddz = pos[j * 3 + 2] - zi;
          T d2 = ddx * ddx + ddy * ddy + ddz * ddz;
          if (d2 <= r2) {
            if (offs == nullptr) {
              ++c;
            } else {
              src_out[w] = j;
              dst_out[w] = i;
              dist_out[w] = sqrt(d2);
              ++w;
            }
          }
        }
      }
    }
  }
  if (offs == nullptr) count[s] = c;
}

}  // namespace

// Cell-list radius pairs for ONE large open-boundary graph.  Host
// wrapper (Python) supplies the cell sort; returns (src, dst, dist)
// ordered by SORTED slot (per-dst contiguous; dst order follows the
// cell sort, re-sorted dst-major in Python).
std::vector<torch::Tensor> radius_pairs_cells(
    torch::Tensor pos, torch::Tensor order, torch::Tensor cell_of,
    torch::Tensor cell_start, long ncx, long ncy, long ncz, double r,
    bool loop) {
  TORCH_CHECK(pos.is_cuda() && pos.is_contiguous());
  long N = pos.size(0);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto count = torch::zeros({N}, pos.options().dtype(torch::kInt));
  long blocks = (N + RB - 1) / RB;
  if (N == 0) blocks = 1;
  auto ord = order.contiguous();
  auto co = cell_of.contiguous();
  auto cs = cell_start.contiguous();
  AT_DISPATCH_FLOATING_TYPES(pos.scalar_type(), "radius_cells", [&] {
    hipLaunchKernelGGL((radius_cells_kernel<scalar_t>), dim3(blocks),
                       dim3(RB), 0, stream, pos.data_ptr<scalar_t>(),
                       ord.data_ptr<long>(), co.data_ptr<long>(),
                       cs.data_ptr<long>(), (int)ncx, (int)ncy,
                       (int)ncz, N, (scalar_t)(r * r), loop, nullptr,
                       count.data_ptr<int>(), nullptr, nullptr,
                       nullptr);
  });
  auto offs = torch::zeros({N}, pos.options().dtype(torch::kLong));
  auto csum = count.to(torch::kLong).cumsum(0);
  if (N > 1) offs.slice(0, 1, N).copy_(csum.slice(0, 0, N - 1));
  long E = N > 0 ? csum[-1].item<long>() : 0;
  auto src = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dst = torch::empty({E}, pos.options().dtype(torch::kLong));
  auto dist = torch::empty({E}, pos.options());
  if (E > 0) {
    AT_DISPATCH_FLOATING_TYPES(pos.scalar_type(), "radius_cells_f",
                               [&] {
      hipLaunchKernelGGL((radius_cells_kernel<scalar_t>), dim3(blocks),
                         dim3(RB), 0, stream, pos.data_ptr<scalar_t>(),
                         ord.data_ptr<long>(), co.data_ptr<long>(),
                         cs.data_ptr<long>(), (int)ncx, (int)ncy,
                         (int)ncz, N, (scalar_t)(r * r), loop,
                         offs.data_ptr<long>(), nullptr,
                         src.data_ptr<long>(), dst.data_ptr<long>(),
                         dist.data_ptr<scalar_t>());
    });
  }
  return {src, dst, dist};
}
