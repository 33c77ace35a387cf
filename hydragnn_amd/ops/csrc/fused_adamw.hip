// Fused AdamW over a flat parameter/gradient buffer (gfx950).
//
// The captured train step (train/captured.py) keeps every gradient as
// a view into ONE flat buffer; flattening the parameters the same way
// turns the optimizer into a single elementwise kernel instead of
// ~10 foreach launches — and because `step` is carried in a device
// tensor incremented by a stream-ordered prelude kernel, the whole
// update is hipGraph-capturable (the graph replays the optimizer too).
//
// Math is torch.optim.AdamW's (decoupled weight decay, bias
// correction, eps outside the root):
//   p *= 1 - lr*wd
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
//   p -= lr * (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps)
//
// Constants.  Every constant reaches the elementwise kernel as the
// single fp32 rounding of its double value:
//   - lr, b1, b2, eps, 1-b1, 1-b2 and 1-lr*wd are formed on the host in
//     double and passed as float;
//   - 1-b1^t and 1-b2^t are formed in double by the one-thread prelude
//     from the device step counter it has just incremented, and stored
//     as float in `bc` [2], which the elementwise kernel reads.
// Forming 1-b2 or 1-b2^t in fp32 from the fp32 beta costs 1e-5
// relative; rounded once the whole update stays within the dozen-ulp
// bound derived in tests/_exact_adamw.py.  Multiply, add, divide and
// sqrt are correctly rounded (no fast-math; __fsqrt_rn and IEEE
// division), so the bound is a plain count of roundings.
//
// Master reconciliation (bf16 variant).  The fp32 master is the
// authoritative weight only while it still rounds to the stored bf16
// parameter: element by element, if bf16(master[i]) and p[i] differ in
// any bit, p[i] was overwritten from outside (load_state_dict, a
// broadcast) and the step starts from float(p[i]) instead.  The test
// is part of the kernel, so it needs no host sync and survives capture.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace {

// step[0] += 1, then both bias corrections from the new count, in
// double, rounded once.
__global__ void adamw_prelude_kernel(float* __restrict__ step,
                                     float* __restrict__ bc,
                                     double beta1, double beta2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float t = step[0] + 1.0f;
    step[0] = t;
    bc[0] = (float)(1.0 - pow(beta1, (double)t));
    bc[1] = (float)(1.0 - pow(beta2, (double)t));
  }
}

struct AdamWConsts {
  float lr, beta1, beta2, eps;
  float one_m_beta1, one_m_beta2, decay;  // 1-b1, 1-b2, 1-lr*wd
};

AdamWConsts adamw_consts(double lr, double beta1, double beta2,
                         double eps, double wd) {
  AdamWConsts c;
  c.lr = (float)lr;
  c.beta1 = (float)beta1;
  c.beta2 = (float)beta2;
  c.eps = (float)eps;
  c.one_m_beta1 = (float)(1.0 - beta1);
  c.one_m_beta2 = (float)(1.0 - beta2);
  c.decay = (float)(1.0 - lr * wd);
  return c;
}

// One element: advances m and v in place, returns the new parameter.
__device__ __forceinline__ float adamw_update(
    float pi, float gi, float& mi, float& vi, float bc1, float bc2,
    const AdamWConsts& c) {
  pi = pi * c.decay;
  mi = c.beta1 * mi + c.one_m_beta1 * gi;
  vi = c.beta2 * vi + c.one_m_beta2 * gi * gi;
  float denom = __fsqrt_rn(vi / bc2) + c.eps;
  return pi - c.lr * (mi / bc1) / denom;
}

__global__ void fused_adamw_kernel(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v,
    const float* __restrict__ bc,  // [2], written by the prelude
    long n, AdamWConsts c) {
  const float bc1 = bc[0];
  const float bc2 = bc[1];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float mi = m[i], vi = v[i];
    float pi = adamw_update(p[i], g[i], mi, vi, bc1, bc2, c);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// Mixed-precision variant: bf16 working params/grads, fp32 master +
// moments (pure-bf16 compute with fp32 optimizer state).
__global__ void fused_adamw_bf16_kernel(
    __hip_bfloat16* __restrict__ p, const __hip_bfloat16* __restrict__ g,
    float* __restrict__ master, float* __restrict__ m,
    float* __restrict__ v, const float* __restrict__ bc,
    long n, AdamWConsts c) {
  const float bc1 = bc[0];
  const float bc2 = bc[1];
  const unsigned short* p_bits =
      reinterpret_cast<const unsigned short*>(p);
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    // master reconciliation, see the header
    float w = master[i];
    const unsigned short stored = p_bits[i];
    const __hip_bfloat16 rounded = __float2bfloat16(w);
    if (*reinterpret_cast<const unsigned short*>(&rounded) != stored)
      w = __uint_as_float((unsigned)stored << 16);
    float mi = m[i], vi = v[i];
    w = adamw_update(w, __bfloat162float(g[i]), mi, vi, bc1, bc2, c);
    m[i] = mi;
    v[i] = vi;
    master[i] = w;
    p[i] = __float2bfloat16(w);
  }
}

// Every operand check of both entry points; nothing is launched
// before it returns.
void check_operands(const torch::Tensor& p, at::ScalarType p_type,
                    const torch::Tensor& g,
                    const torch::Tensor* master, const torch::Tensor& m,
                    const torch::Tensor& v, const torch::Tensor& step,
                    const torch::Tensor& bc) {
  auto flat = [&](const torch::Tensor& t, at::ScalarType ty,
                  const char* name) {
    TORCH_CHECK(t.is_cuda(), "fused_adamw: ", name,
                " must be a device tensor");
    TORCH_CHECK(t.device() == p.device(), "fused_adamw: ", name,
                " is on another device than p");
    TORCH_CHECK(t.scalar_type() == ty, "fused_adamw: ", name,
                " has dtype ", t.scalar_type(), ", expected ", ty);
    TORCH_CHECK(t.is_contiguous(), "fused_adamw: ", name,
                " must be contiguous");
  };
  auto same_size = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.sizes() == p.sizes(), "fused_adamw: ", name,
                " has shape ", t.sizes(), ", p has ", p.sizes());
  };
  flat(p, p_type, "p");
  flat(g, p_type, "g");
  same_size(g, "g");
  if (master != nullptr) {
    flat(*master, at::ScalarType::Float, "master");
    same_size(*master, "master");
  }
  flat(m, at::ScalarType::Float, "m");
  same_size(m, "m");
  flat(v, at::ScalarType::Float, "v");
  same_size(v, "v");
  flat(step, at::ScalarType::Float, "step");
  TORCH_CHECK(step.numel() == 1,
              "fused_adamw: step must hold one element, has ",
              step.numel());
  flat(bc, at::ScalarType::Float, "bias_corr");
  TORCH_CHECK(bc.numel() == 2,
              "fused_adamw: bias_corr must hold two elements, has ",
              bc.numel());
}

constexpr int kBlock = 256;
constexpr long kMaxBlocks = 8192;

}  // namespace

void fused_adamw(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                 torch::Tensor v, torch::Tensor step, torch::Tensor bc,
                 double lr, double beta1, double beta2, double eps,
                 double wd) {
  check_operands(p, at::ScalarType::Float, g, nullptr, m, v, step, bc);
  long n = p.numel();
  if (n == 0) return;  // nothing to update: step and bc stay as they are
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(adamw_prelude_kernel, dim3(1), dim3(64), 0, stream,
                     step.data_ptr<float>(), bc.data_ptr<float>(),
                     beta1, beta2);
  long blocks = std::min((n + kBlock - 1) / kBlock, kMaxBlocks);
  hipLaunchKernelGGL(fused_adamw_kernel, dim3(blocks), dim3(kBlock), 0,
                     stream, p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     bc.data_ptr<float>(), n,
                     adamw_consts(lr, beta1, beta2, eps, wd));
}

void fused_adamw_bf16(torch::Tensor p, torch::Tensor g,
                      torch::Tensor master, torch::Tensor m,
                      torch::Tensor v, torch::Tensor step,
                      torch::Tensor bc, double lr, double beta1,
                      double beta2, double eps, double wd) {
  check_operands(p, at::ScalarType::BFloat16, g, &master, m, v, step,
                 bc);
  long n = p.numel();
  if (n == 0) return;  // nothing to update: step and bc stay as they are
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(adamw_prelude_kernel, dim3(1), dim3(64), 0, stream,
                     step.data_ptr<float>(), bc.data_ptr<float>(),
                     beta1, beta2);
  long blocks = std::min((n + kBlock - 1) / kBlock, kMaxBlocks);
  hipLaunchKernelGGL(
      fused_adamw_bf16_kernel, dim3(blocks), dim3(kBlock), 0, stream,
      reinterpret_cast<__hip_bfloat16*>(p.data_ptr()),
      reinterpret_cast<const __hip_bfloat16*>(g.data_ptr()),
      master.data_ptr<float>(), m.data_ptr<float>(),
      v.data_ptr<float>(), bc.data_ptr<float>(), n,
      adamw_consts(lr, beta1, beta2, eps, wd));
}
