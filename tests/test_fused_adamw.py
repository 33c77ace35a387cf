"""FusedAdamW (flat-buffer single-kernel AdamW) on the CPU: the
trajectory against torch.optim.AdamW, one step of the fallback against
the float64 reference and the rounding-count bound of _exact_adamw.py,
resume, master reconciliation, the view check and the errors.  The HIP
kernels are held to the same reference and bound in
tests/test_gpu_fused_adamw.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_adamw as X  # noqa: E402
from hydragnn_amd.ops.fused_adamw import FusedAdamW  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16)


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.SiLU(),
                               torch.nn.Linear(16, 3))


def test_fused_adamw_matches_torch_cpu():
    m1, m2 = _model(1), _model(1)
    m2.load_state_dict(m1.state_dict())
    o1 = torch.optim.AdamW(m1.parameters(), lr=3e-3, weight_decay=0.01)
    o2 = FusedAdamW(m2.parameters(), lr=3e-3, weight_decay=0.01)
    x = torch.randn(32, 6)
    y = torch.randn(32, 3)
    for i in range(10):
        o1.zero_grad()
        torch.nn.functional.mse_loss(m1(x), y).backward()
        o1.step()
        o2.zero_grad()
        torch.nn.functional.mse_loss(m2(x), y).backward()
        o2.step()
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.allclose(p1, p2, rtol=1e-5, atol=1e-6), \
            (p1 - p2).abs().max()


def test_fused_adamw_params_are_flat_views():
    m = _model(2)
    o = FusedAdamW(m.parameters(), lr=1e-3)
    base = o.flat_param
    for p in m.parameters():
        assert p.data.data_ptr() >= base.data_ptr()
        assert p.grad is not None and \
            p.grad.data_ptr() >= o.flat_grad.data_ptr()
    # zero_grad keeps the views alive
    o.zero_grad()
    for p in m.parameters():
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0


def test_reference_matches_torch_adamw_fp64():
    """The float64 reference is torch.optim.AdamW's definition: five
    chained steps on float64 parameters.  torch orders the same
    operations differently (lr / bc1 first, sqrt(v) / sqrt(bc2)), so
    each step may differ by a few float64 roundings of the terms of
    p' = P - U; 32 * 2^-53 * (|P| + |U|) per step taken so far is the
    tolerance, and 8 * 2^-53 relative per step for m and v (three
    roundings each)."""
    h = X.Hyper(None, 3e-3, (0.9, 0.999), 1e-8, 0.01, False)
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(301, generator=gen, dtype=X.F64)
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([w], lr=h.lr, betas=h.betas, eps=h.eps,
                            weight_decay=h.wd, foreach=False)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    eps64 = 2.0 ** -53
    for t in range(1, 6):
        g = torch.randn(301, generator=gen, dtype=X.F64) \
            * 10.0 ** (torch.rand(301, generator=gen, dtype=X.F64) * 6 - 4)
        w.grad = g.clone()
        opt.step()
        ref = X.reference_step(p, g, m, v, t, h.lr, h.betas, h.eps, h.wd)
        p, m, v = ref.p, ref.m, ref.v
        st = opt.state[w]
        tol = 32 * t * eps64 * (ref.decayed.abs() + ref.update.abs())
        assert bool(((w.detach() - p).abs() <= tol).all())
        assert bool(((st["exp_avg"] - m).abs()
                     <= 8 * t * eps64 * ((h.betas[0] * m).abs()
                                         + g.abs())).all())
        assert bool(((st["exp_avg_sq"] - v).abs()
                     <= 8 * t * eps64 * v).all())


def _one_tensor_optimizer(case, h, dtype, device="cpu"):
    return X.make_optimizer(case, h, dtype, device)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("ih", range(len(X.HYPERS)))
def test_fallback_step_within_bound(ih, dtype):
    """One step of the CPU fallback over the hyperparameter grid: every
    element of p (master), m and v within the derived bound of the
    float64 reference; the bf16 parameter is the rounded master."""
    h = X.HYPERS[ih]
    case = X.make_case(1031, dtype, seed=100 + ih, cold=h.cold)
    opt, w = _one_tensor_optimizer(case, h, dtype)
    before = (case.p, case.g, case.m, case.v)
    opt.step()
    work = opt.flat_param if opt.master is None else opt.master
    X.check_step(before, (work, opt.exp_avg, opt.exp_avg_sq), h,
                 f"fallback {dtype} {h}")
    assert float(opt.step_t) == h.t
    if opt.master is not None:
        assert X.same_bits(opt.flat_param, opt.master.bfloat16())
    assert w.data_ptr() == opt.flat_param.data_ptr()
    if h.lr == 0.0:
        # lr = 0: p bit-unchanged, the moments still advance
        assert X.same_bits(work, case.p)
        moved = ~case.zero
        assert bool((opt.exp_avg[moved] != case.m[moved]).any())
        assert bool((opt.exp_avg_sq[moved] != case.v[moved]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_zero_update_without_decay_leaves_p_unchanged(dtype):
    """wd = 0 and g = m = v = 0 everywhere: p is bit-unchanged."""
    h = X.Hyper(3, 1e-3, (0.9, 0.999), 1e-8, 0.0, False)
    case = X.make_case(257, dtype, seed=5)
    for x in (case.g, case.m, case.v):
        x.zero_()
    opt, _ = _one_tensor_optimizer(case, h, dtype)
    opt.step()
    work = opt.flat_param if opt.master is None else opt.master
    assert X.same_bits(work, case.p)
    assert not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())


def _data(seed, steps):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(8, 6, generator=gen),
             torch.randn(8, 3, generator=gen)) for _ in range(steps)]


def _train(model, opt, batches):
    dtype = next(model.parameters()).dtype
    for x, y in batches:
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x.to(dtype)).float(),
                                     y).backward()
        opt.step()


def _state(opt):
    return [opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_t] \
        + ([] if opt.master is None else [opt.master])


def _resume(dtype, save, load):
    """Six uninterrupted steps against three, a checkpoint into a fresh
    model and optimizer of another seed and lr, and three more."""
    batches = _data(21, 6)
    whole = _model(3).to(dtype)
    o_whole = FusedAdamW(whole.parameters(), lr=3e-3, weight_decay=0.02)
    _train(whole, o_whole, batches)

    first = _model(3).to(dtype)
    o_first = FusedAdamW(first.parameters(), lr=3e-3, weight_decay=0.02)
    _train(first, o_first, batches[:3])
    save(first, o_first)

    second = _model(17).to(dtype)
    o_second = FusedAdamW(second.parameters(), lr=0.5)
    load(second, o_second)
    assert o_second.param_groups[0]["lr"] == 3e-3
    assert o_second.param_groups[0]["weight_decay"] == 0.02
    assert float(o_second.step_t) == 3.0
    _train(second, o_second, batches[3:])
    for a, b in zip(_state(o_whole), _state(o_second)):
        assert X.same_bits(a, b)
    for a, b in zip(whole.parameters(), second.parameters()):
        assert X.same_bits(a.detach(), b.detach())


def test_fused_adamw_state_roundtrip(tmp_path):
    """Resume through torch.save / torch.load is bit-equal to the
    uninterrupted run: parameters, moments, step and master."""
    for dtype in DTYPES:
        path = tmp_path / f"ckpt_{dtype}.pt"

        def save(model, opt):
            torch.save({"model": model.state_dict(),
                        "opt": opt.state_dict()}, path)

        def load(model, opt):
            ckpt = torch.load(path)
            model.load_state_dict(ckpt["model"])
            opt.load_state_dict(ckpt["opt"])

        _resume(dtype, save, load)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_resume_through_save_model(tmp_path, dtype):
    from hydragnn_amd.utils.model.model import (load_existing_model,
                                                save_model)

    def save(model, opt):
        save_model(model, opt, "resume", path=str(tmp_path))

    def load(model, opt):
        load_existing_model(model, "resume", path=str(tmp_path),
                            optimizer=opt)

    _resume(dtype, save, load)


def test_stale_master_starts_from_loaded_weights():
    """Build the optimizer, load weights, step: the step starts from the
    loaded weights, not from the master copied at construction."""
    h = X.Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True)
    case = X.make_case(513, torch.bfloat16, seed=9, cold=True)
    opt, w = _one_tensor_optimizer(case, h, torch.bfloat16)
    gen = torch.Generator().manual_seed(10)
    loaded = (torch.randn(513, generator=gen) + 3.0).bfloat16()
    # half of the elements are overwritten, the others keep their master
    loaded[::2] = opt.flat_param[::2]
    holder = torch.nn.ParameterList([w])
    holder.load_state_dict({"0": loaded})
    assert w.data_ptr() == opt.flat_param.data_ptr()
    start = torch.where(X.bits(loaded) != X.bits(case.p.bfloat16()),
                        loaded.float(), case.p)
    assert bool((start != case.p).any()) and bool((start == case.p).any())
    opt.step()
    X.check_step((start, case.g, case.m, case.v),
                 (opt.master, opt.exp_avg, opt.exp_avg_sq), h,
                 "stale master")
    assert X.same_bits(opt.flat_param, opt.master.bfloat16())


def _ready(seed=6):
    m = _model(seed)
    o = FusedAdamW(m.parameters(), lr=1e-2)
    x = torch.randn(8, 6)
    return m, o, x


def _detach_by_model_zero_grad(m):
    m.zero_grad()


def _detach_by_grad_none(m):
    m[2].weight.grad = None


def _detach_by_data_clone(m):
    m[0].bias.data = m[0].bias.data.clone()


@pytest.mark.parametrize("detach", [_detach_by_model_zero_grad,
                                    _detach_by_grad_none,
                                    _detach_by_data_clone])
def test_detached_views_raise(detach):
    m, o, x = _ready()
    m(x).square().sum().backward()
    o.step()
    detach(m)
    m(x).square().sum().backward()
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(RuntimeError, match="zero_grad"):
        o.step()
    for a, p in zip(before, m.parameters()):
        assert X.same_bits(a, p.detach())


def test_optimizer_zero_grad_keeps_training():
    m, o, x = _ready()
    for _ in range(2):
        o.zero_grad(set_to_none=True)
        m(x).square().sum().backward()
        assert float(o.flat_grad.abs().max()) > 0
        before = o.flat_param.clone()
        o.step()
        assert bool((o.flat_param != before).any())


def test_scheduler_lr_reaches_each_step():
    """StepLR halves lr every second step; each step is within the
    bound of the reference at the scheduled lr."""
    h0 = X.Hyper(1, 4e-3, (0.9, 0.999), 1e-8, 0.01, True)
    case = X.make_case(257, torch.float32, seed=12, cold=True)
    opt, _ = _one_tensor_optimizer(case, h0, torch.float32)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    seen = []
    for t in range(1, 6):
        lr = 4e-3 * 0.5 ** ((t - 1) // 2)
        assert opt.param_groups[0]["lr"] == pytest.approx(lr, rel=1e-12)
        lr = opt.param_groups[0]["lr"]
        seen.append(lr)
        g = X.make_case(257, torch.float32, seed=30 + t).g
        opt.flat_grad.copy_(g)
        before = (opt.flat_param.clone(), g, opt.exp_avg.clone(),
                  opt.exp_avg_sq.clone())
        opt.step()
        sched.step()
        X.check_step(before,
                     (opt.flat_param, opt.exp_avg, opt.exp_avg_sq),
                     h0._replace(t=t, lr=lr), f"scheduled step {t}")
    assert len(set(seen)) == 3


def test_single_group_dict_and_group_errors():
    m = _model(7)
    o = FusedAdamW([{"params": list(m.parameters()), "lr": 2e-3,
                     "weight_decay": 0.0}], lr=1.0)
    assert o.param_groups[0]["lr"] == 2e-3
    assert o.param_groups[0]["weight_decay"] == 0.0
    assert o.param_groups[0]["betas"] == (0.9, 0.999)
    assert o.flat_param.numel() == sum(p.numel() for p in m.parameters())
    m(torch.randn(4, 6)).sum().backward()
    o.step()

    m = _model(7)
    with pytest.raises(ValueError, match="single group"):
        FusedAdamW([{"params": list(m[0].parameters())},
                    {"params": list(m[2].parameters()), "lr": 1e-4}])
    extra = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="cannot be added"):
        o.add_param_group({"params": [extra]})
    assert len(o.param_groups) == 1


def test_load_state_dict_rejects_foreign_state():
    m = _model(8)
    o = FusedAdamW(m.parameters(), lr=1e-3)
    m2 = _model(8)
    foreign = torch.optim.AdamW(m2.parameters(), lr=1e-3)
    m2(torch.randn(4, 6)).sum().backward()
    foreign.step()
    with pytest.raises(ValueError, match="'flat'"):
        o.load_state_dict(foreign.state_dict())
    assert float(o.step_t) == 0.0


def test_fused_adamw_bf16_master_mode_cpu():
    """bf16 params + fp32 master: trajectory tracks an fp32
    torch.optim.AdamW run within bf16 resolution."""
    m_ref = _model(4)
    m_bf = _model(4)
    m_bf.load_state_dict(m_ref.state_dict())
    m_bf = m_bf.to(torch.bfloat16)
    o_ref = torch.optim.AdamW(m_ref.parameters(), lr=3e-3,
                              weight_decay=0.01)
    o_bf = FusedAdamW(m_bf.parameters(), lr=3e-3, weight_decay=0.01)
    assert o_bf.master is not None
    x = torch.randn(32, 6)
    y = torch.randn(32, 3)
    for _ in range(8):
        o_ref.zero_grad()
        torch.nn.functional.mse_loss(m_ref(x), y).backward()
        o_ref.step()
        o_bf.zero_grad()
        torch.nn.functional.mse_loss(
            m_bf(x.bfloat16()).float(), y).backward()
        o_bf.step()
    for p1, p2 in zip(m_ref.parameters(), m_bf.parameters()):
        assert torch.allclose(p1, p2.float(), rtol=0.1, atol=0.05), \
            (p1 - p2.float()).abs().max()
