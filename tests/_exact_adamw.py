"""Shared pieces of the FusedAdamW tests (test_fused_adamw.py on the CPU
fallback, test_gpu_fused_adamw.py on the HIP kernels): a float64
reference of one AdamW step that does not go through the ops, the
rounding-count bound an fp32 evaluation of that step has to meet, the
cases, and the checks, which work on whatever device their operands
live on.

Reference
---------
One step of AdamW as published (Loshchilov & Hutter, decoupled decay;
Kingma & Ba, bias correction, eps outside the root), which is what
torch.optim.AdamW computes (test_reference_matches_torch_adamw_fp64):

    P  = p (1 - lr wd)
    M  = b1 m + (1 - b1) g            V = b2 v + (1 - b2) g^2
    U  = lr (M / (1 - b1^t)) / (sqrt(V / (1 - b2^t)) + eps)
    p' = P - U

in float64 from the fp32 (bf16 for g in the bf16 variant) values of
p, g, m and v widened exactly; t is an integer and lr, b1, b2, eps, wd
are the Python doubles the user passed.

Bound
-----
u = 2^-24 is the unit roundoff of fp32 and gamma_k = k u / (1 - k u)
bounds a product of k factors (1 + d), |d| <= u.  The kernel evaluates
the formula above in fp32.  Each constant (lr, b1, b2, eps, 1 - b1,
1 - b2, 1 - lr wd, 1 - b1^t, 1 - b2^t) is the double value rounded
once: one factor.  Multiply, add, divide and sqrt are correctly
rounded: one factor each.  There is no fast-math, and a fused
multiply-add only removes a factor.  Every bound is relative to the sum
of the absolute values of the terms, never to a result that may cancel.

m:  fl(fl(b1 m) + fl((1-b1) g)).  Each product carries its constant and
    its multiply, the sum one more:
        |m_k - M| <= gamma_3 S,      S = |b1 m| + |(1 - b1) g|.
v:  fl(fl(b2 v) + fl(fl((1-b2) g) g)).  The second product carries a
    constant and two multiplies, the sum one more; every term is >= 0:
        |v_k - V| <= gamma_4 V.
U:  fl(fl(lr mh) / D_k), mh = fl(m_k / bc1), D_k = fl(sq + eps),
    sq = fl(sqrt(fl(v_k / bc2))).
      mh   = (m_k / (1 - b1^t)) (1 + th_2)          constant, divide
      v_k / bc2: V (1 + th_4) / (1 - b2^t), constant, divide: th_6;
      its root halves that, sqrt(1 + th_6) <= 1 + th_3, and rounds:
      sq = sqrt(V / (1 - b2^t)) (1 + th_4)
      D_k  = (sq + eps (1 + d)) (1 + d) = D (1 + th_5), both terms >= 0
      lr, its multiply and the last divide: three more.
    So U_k = lr (m_k / (1 - b1^t)) / D times ten factors, th_10, and
    m_k = M + e_m with |e_m| <= gamma_3 S, |M| <= S:
        |U_k - U| <= gamma_13 A,     A = lr S / ((1 - b1^t) D) >= |U|.
    A dozen u, as a count of the operations suggests.
p': fl(fl(p dk) - U_k).  fl(p dk) = P (1 + th_2), the difference rounds
    once more, which also multiplies the error of U_k by (1 + d):
        |p_k - p'| <= gamma_3 |P| + gamma_14 A.

The double evaluations (the constants before they are rounded, the
device's pow in 1 - b^t, this reference itself) are each good to a few
2^-53 of numbers that cancel by at most 1 - b >= 1e-3, below 2^-40
relative; ETA = 2^-38 is added to every gamma for them.  The magnitudes
of the cases (|g| in 1e-6 .. 1e3, lr >= 1e-3 or 0, eps >= 1e-8) keep
every fp32 intermediate either normal or exactly 0, so no absolute
term is needed.

An fp32 evaluation with exact constants measures under 6 u on the
update; forming 1 - b2 and 1 - b2^t in fp32 from the fp32 beta
measures 70 to 180 u.  The bound separates the two.  It is the count
above and is not tuned to what any implementation produces.

In the bf16 variant the bounds hold for master, m and v, and the stored
parameter is the round-to-nearest-even bf16 of the new master.
"""

from collections import namedtuple

import torch

F64 = torch.float64
U = 2.0 ** -24
ETA = 2.0 ** -38


def gamma(k):
    return k * U / (1.0 - k * U) + ETA


Hyper = namedtuple("Hyper", "t lr betas eps wd cold")
Step = namedtuple("Step", "decayed update p m v")
Bounds = namedtuple("Bounds", "p m v update")

# Every value the optimizer's hyperparameters take in the tests occurs
# in one of these: t, the betas, eps, wd, lr, and one cold start.
HYPERS = (
    Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, False),
    Hyper(2, 1e-3, (0.9, 0.95), 1e-3, 0.0, False),
    Hyper(10, 1e-3, (0.0, 0.999), 1e-8, 0.01, False),
    Hyper(1000, 1e-3, (0.9, 0.999), 1e-8, 0.0, False),
    Hyper(100000, 0.0, (0.9, 0.999), 1e-3, 0.01, False),
    Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True),
)


def reference_step(p, g, m, v, t, lr, betas, eps, wd):
    """One AdamW step in float64; see the module docstring."""
    assert isinstance(t, int) and t >= 1
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    b1, b2 = betas
    decayed = p * (1.0 - lr * wd)
    m_new = b1 * m + (1.0 - b1) * g
    v_new = b2 * v + (1.0 - b2) * g * g
    denom = (v_new / (1.0 - b2 ** t)).sqrt() + eps
    update = lr * (m_new / (1.0 - b1 ** t)) / denom
    return Step(decayed, update, decayed - update, m_new, v_new)


def bounds(p, g, m, v, t, lr, betas, eps, wd):
    """The absolute error an fp32 evaluation of the step may have, per
    element, for p', M, V and U; derived in the module docstring."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    b1, b2 = betas
    ref = reference_step(p, g, m, v, t, lr, betas, eps, wd)
    s = (b1 * m).abs() + ((1.0 - b1) * g).abs()
    denom = (ref.v / (1.0 - b2 ** t)).sqrt() + eps
    a = lr * s / ((1.0 - b1 ** t) * denom)
    return Bounds(p=gamma(3) * ref.decayed.abs() + gamma(14) * a,
                  m=gamma(3) * s,
                  v=gamma(4) * ref.v,
                  update=gamma(13) * a)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
Case = namedtuple("Case", "p g m v zero")
ZERO_EVERY = 7   # elements 0, 7, 14, ... have g = m = v = 0


def make_case(n, dtype, seed, cold=False):
    """CPU operands of one step.  |g| is log-uniform over 1e-6 .. 1e3
    with random sign (rounded to bf16 in the bf16 variant); m and v are
    warm and of the gradient's scale, m with either sign relative to g
    so that b1 m + (1 - b1) g also cancels, v >= 0; p is the fp32
    parameter (the master, in the bf16 variant).  Every ZERO_EVERY-th
    element has g = m = v = 0.  `cold`: m = v = 0 everywhere."""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 9.0 - 6.0)
    sign = torch.randint(0, 2, (n,), generator=gen).to(F64) * 2.0 - 1.0
    g = (mag * sign).float().to(dtype)
    g64 = g.to(F64)
    m = (g64 * (torch.rand(n, generator=gen, dtype=F64) * 3.0 - 1.5)).float()
    v = (g64 * g64 * (torch.rand(n, generator=gen, dtype=F64) * 1.75
                      + 0.25)).float()
    p = torch.randn(n, generator=gen, dtype=F64).float()
    zero = torch.zeros(n, dtype=torch.bool)
    zero[::ZERO_EVERY] = True
    g[zero] = 0
    m[zero] = 0
    v[zero] = 0
    if cold:
        m.zero_()
        v.zero_()
    return Case(p, g, m, v, zero)


def make_optimizer(case, h, dtype, device):
    """A FusedAdamW over one parameter tensor holding `case`, with the
    moments, the master, the gradient and the step counter (t - 1) set
    so that the next step() is step `h.t` of the case.  Returns the
    optimizer and the parameter."""
    from hydragnn_amd.ops.fused_adamw import FusedAdamW
    w = torch.nn.Parameter(case.p.to(dtype).to(device))
    opt = FusedAdamW([w], lr=h.lr, betas=h.betas, eps=h.eps,
                     weight_decay=h.wd)
    with torch.no_grad():
        if opt.master is not None:
            opt.master.copy_(case.p)     # rounds to the stored bf16
        opt.flat_grad.copy_(case.g)
        opt.exp_avg.copy_(case.m)
        opt.exp_avg_sq.copy_(case.v)
        opt.step_t.fill_(h.t - 1)
    return opt, w


def bits(x):
    """The tensor's bit pattern as integers of its element size."""
    return x.contiguous().view(
        {2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape \
        and bool(torch.equal(bits(a), bits(b)))


def check_within(got, ref, bound, what):
    """Every element of `got` lies within `bound` of `ref`."""
    err = (got.to(F64) - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                            torch.full_like(err, float("inf")))
        ratio = torch.where(bad, ratio, torch.zeros_like(ratio))
        i = int(ratio.argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {err.numel()} elements outside "
            f"the bound; worst at [{i}]: got {float(got[i])!r}, reference "
            f"{float(ref[i])!r}, error {float(err[i]):.3e} = "
            f"{float(ratio[i]):.2f} x bound "
            f"({float(bound[i] / U):.3e} u absolute)")


def check_step(before, after, h, what):
    """`before` and `after` are (p, g, m, v) with p the fp32 parameter
    (or master): every element of the new p, m and v within the bound
    of the float64 step from `before`; exact-zero elements exactly."""
    p, g, m, v = before
    p_k, m_k, v_k = after
    args = (int(h.t), h.lr, h.betas, h.eps, h.wd)
    ref = reference_step(p, g, m, v, *args)
    bnd = bounds(p, g, m, v, *args)
    check_within(m_k, ref.m, bnd.m, f"{what}: m")
    check_within(v_k, ref.v, bnd.v, f"{what}: v")
    check_within(p_k, ref.p, bnd.p, f"{what}: p")
    # g = m = v = 0: the moments stay 0, the update is exactly 0 and
    # the new parameter is the single fp32 rounding of p times the
    # fp32 decay constant (itself the double 1 - lr wd rounded once)
    zero = (g == 0) & (m == 0) & (v == 0)
    if bool(zero.any()):
        assert not bool(m_k[zero].any()) and not bool(v_k[zero].any()), \
            f"{what}: moments of exact-zero elements moved"
        decay = torch.tensor(1.0 - h.lr * h.wd, dtype=F64).float().to(F64)
        want = (p[zero].to(F64) * decay.to(p.device)).float()
        assert same_bits(p_k[zero], want), \
            f"{what}: exact-zero elements are not fl(p * decay)"
