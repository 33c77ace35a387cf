"""The FusedAdamW HIP kernels (csrc/fused_adamw.hip) against the float64
AdamW step and the rounding-count bound of _exact_adamw.py: single
steps through the raw entry points across the block and grid edges and
the hyperparameter grid, with guard regions; consecutive steps on the
device-side counter; master reconciliation; run-to-run identity;
capture; no host sync; operand checks; learning-rate changes."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("requires MI355X GPU", allow_module_level=True)

import _exact_adamw as X  # noqa: E402
from hydragnn_amd.ops._extension import get_extension  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
DTYPES = (F32, BF16)
IDS = ("fp32", "bf16")

GRID = 8192 * 256        # elements of one grid-stride pass
NS = (1, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * GRID + 257)
GUARD = 64               # elements on either side of every operand
SENTINEL = -1234.5       # exact in fp32 and bf16

# every n meets both dtypes; every entry of HYPERS meets both dtypes
SINGLE = [(n, dt, X.HYPERS[(i + 3 * j) % len(X.HYPERS)])
          for i, n in enumerate(NS) for j, dt in enumerate(DTYPES)]


def _guarded(t, dtype=None):
    """`t` on the device as an interior slice of a larger allocation
    filled with SENTINEL; returns (allocation, slice)."""
    dtype = dtype or t.dtype
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=dtype,
                     device=DEV)
    view = buf[GUARD:GUARD + t.numel()]
    view.copy_(t)
    return buf, view


def _guards_intact(buf, what):
    want = torch.full((GUARD,), SENTINEL, dtype=buf.dtype, device=DEV)
    assert X.same_bits(buf[:GUARD], want), f"{what}: front guard written"
    assert X.same_bits(buf[-GUARD:], want), f"{what}: back guard written"


class Raw:
    """Operands of one raw call, each inside guards."""

    def __init__(self, case, h, dtype):
        self.h, self.dtype = h, dtype
        self.bufs = {}
        ops = {"g": case.g, "m": case.m, "v": case.v,
               "step": torch.tensor([float(h.t - 1)]),
               "bc": torch.tensor([-1.0, -1.0])}
        if dtype == BF16:
            ops["master"] = case.p
            ops["p"] = case.p.bfloat16()
        else:
            ops["p"] = case.p
        for k, t in ops.items():
            self.bufs[k], view = _guarded(t)
            setattr(self, k, view)

    def clone(self):
        other = object.__new__(Raw)
        other.h, other.dtype, other.bufs = self.h, self.dtype, {}
        for k, buf in self.bufs.items():
            other.bufs[k] = buf.clone()
            n = buf.numel() - 2 * GUARD
            setattr(other, k, other.bufs[k][GUARD:GUARD + n])
        return other

    def work(self):
        return self.master if self.dtype == BF16 else self.p

    def call(self, **over):
        ext = get_extension(required=True)
        a = {k: getattr(self, k) for k in self.bufs}
        a.update(over)
        h = self.h
        hyper = (h.lr, h.betas[0], h.betas[1], h.eps, h.wd)
        if self.dtype == BF16:
            ext.fused_adamw_bf16(a["p"], a["g"], a["master"], a["m"],
                                 a["v"], a["step"], a["bc"], *hyper)
        else:
            ext.fused_adamw(a["p"], a["g"], a["m"], a["v"], a["step"],
                            a["bc"], *hyper)


@pytest.mark.parametrize(
    "n,dtype,h", SINGLE,
    ids=[f"n{n}-{IDS[DTYPES.index(dt)]}-t{h.t}{'cold' if h.cold else ''}"
         for n, dt, h in SINGLE])
def test_single_step_within_bound(n, dtype, h):
    case = X.make_case(n, dtype, seed=n % 1000 + h.t % 97, cold=h.cold)
    raw = Raw(case, h, dtype)
    before = tuple(x.clone() for x in (raw.work(), raw.g, raw.m, raw.v))
    raw.call()
    what = f"n={n} {dtype} {h}"
    X.check_step(before, (raw.work(), raw.m, raw.v), h, what)
    for k, buf in raw.bufs.items():
        _guards_intact(buf, f"{what}: {k}")
    assert raw.step.tolist() == [float(h.t)]
    want_bc = torch.tensor([1.0 - b ** h.t for b in h.betas], dtype=X.F64)
    assert bool(((raw.bc.cpu().to(X.F64) - want_bc).abs()
                 <= X.gamma(1) * want_bc).all()), (raw.bc, want_bc)
    assert X.same_bits(raw.g, before[1])
    if dtype == BF16:
        # the stored parameter is the new master rounded to nearest even
        assert X.same_bits(raw.p, raw.master.bfloat16())
    if h.lr == 0.0:
        # lr = 0: p bit-unchanged while m and v still advance
        assert X.same_bits(raw.work(), before[0])
        moved = ~case.zero.to(DEV)
        assert bool((raw.v[moved] != before[3][moved]).any())
        assert bool((raw.m[moved] != before[2][moved]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_update_without_decay_leaves_p_unchanged(dtype):
    """wd = 0 and g = m = v = 0 everywhere: p is bit-unchanged."""
    h = X.Hyper(3, 1e-3, (0.9, 0.999), 1e-8, 0.0, False)
    case = X.make_case(1000, dtype, seed=5)
    for x in (case.g, case.m, case.v):
        x.zero_()
    raw = Raw(case, h, dtype)
    before = raw.work().clone()
    raw.call()
    assert X.same_bits(raw.work(), before)
    assert not bool(raw.m.any()) and not bool(raw.v.any())
    assert raw.step.tolist() == [3.0]


def _opt_state(opt):
    return [opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_t] \
        + ([] if opt.master is None else [opt.master])


def _step_and_check(opt, g, h, what):
    opt.flat_grad.copy_(g)
    work = opt.flat_param if opt.master is None else opt.master
    before = (work.clone(), opt.flat_grad.clone(), opt.exp_avg.clone(),
              opt.exp_avg_sq.clone())
    opt.step()
    X.check_step(before, (work, opt.exp_avg, opt.exp_avg_sq), h, what)
    assert opt.step_t.tolist() == [float(h.t)]
    if opt.master is not None:
        assert X.same_bits(opt.flat_param, opt.master.bfloat16())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_twenty_steps_on_the_device_counter(dtype):
    """t = 1 .. 20 with fresh gradients; each step against the reference
    restarted from the kernel's own state before that step."""
    h = X.Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True)
    opt, _ = X.make_optimizer(X.make_case(1543, dtype, 40, cold=True), h,
                              dtype, DEV)
    for t in range(1, 21):
        g = X.make_case(1543, dtype, seed=40 + t).g
        _step_and_check(opt, g, h._replace(t=t), f"{dtype} step {t}")


def test_stale_master_restarts_from_overwritten_parameters():
    h = X.Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True)
    case = X.make_case(GRID + 513, BF16, seed=9, cold=True)
    opt, w = X.make_optimizer(case, h, BF16, DEV)
    gen = torch.Generator().manual_seed(10)
    loaded = (torch.randn(case.p.numel(), generator=gen) + 3.0).bfloat16()
    loaded[::2] = case.p.bfloat16()[::2]     # these keep their master
    holder = torch.nn.ParameterList([w])
    holder.load_state_dict({"0": loaded})
    assert w.data_ptr() == opt.flat_param.data_ptr()
    start = torch.where(X.bits(loaded) != X.bits(case.p.bfloat16()),
                        loaded.float(), case.p).to(DEV)
    before = (start, opt.flat_grad.clone(), opt.exp_avg.clone(),
              opt.exp_avg_sq.clone())
    opt.step()
    X.check_step(before, (opt.master, opt.exp_avg, opt.exp_avg_sq), h,
                 "stale master")
    assert X.same_bits(opt.flat_param, opt.master.bfloat16())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_run_to_run_identity(dtype):
    h = X.HYPERS[0]
    raw = Raw(X.make_case(GRID + 1, dtype, seed=77), h, dtype)
    twin = raw.clone()
    raw.call()
    twin.call()
    for k in raw.bufs:
        assert X.same_bits(raw.bufs[k], twin.bufs[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_step_equals_eager(dtype):
    """opt.step() alone in a graph on one stream, five replays with
    flat_grad refilled in between, against an eager twin that took the
    same steps, warm-up included."""
    warm, replays, n = 3, 5, 5003
    h = X.Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True)
    case = X.make_case(n, dtype, seed=50, cold=True)
    cap, _ = X.make_optimizer(case, h, dtype, DEV)
    eager, _ = X.make_optimizer(case, h, dtype, DEV)
    grads = [X.make_case(n, dtype, seed=60 + i).g.to(DEV)
             for i in range(warm + replays)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for g in grads[:warm]:
            cap.flat_grad.copy_(g)
            cap.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step()
    for g in grads[warm:]:
        cap.flat_grad.copy_(g)
        graph.replay()
    for g in grads:
        eager.flat_grad.copy_(g)
        eager.step()
    torch.cuda.synchronize()
    assert cap.step_t.tolist() == [float(warm + replays)]
    for a, b in zip(_opt_state(cap), _opt_state(eager)):
        assert X.same_bits(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step_without_host_sync(dtype):
    h = X.HYPERS[0]
    opt, _ = X.make_optimizer(X.make_case(3001, dtype, seed=3), h, dtype,
                              DEV)
    opt.step()      # loads the extension
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.zero_grad()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert opt.step_t.tolist() == [float(h.t + 1)]


def _bad_operands(raw):
    """(name, overrides) of calls that must be rejected."""
    n = raw.p.numel()
    bad = []
    names = ["p", "g", "m", "v"] + (["master"] if raw.dtype == BF16 else [])
    for k in names:
        t = getattr(raw, k)
        bad.append((f"{k} on the host", {k: t.cpu()}))
        bad.append((f"{k} of another dtype", {k: t.double()}))
        bad.append((f"{k} strided",
                    {k: torch.zeros(2 * n, dtype=t.dtype,
                                    device=DEV)[::2]}))
        if k != "p":
            bad.append((f"{k} shorter", {k: t[:n - 1]}))
            bad.append((f"{k} longer",
                        {k: torch.zeros(n + 1, dtype=t.dtype,
                                        device=DEV)}))
    bad.append(("p shorter", {"p": raw.p[:n - 1]}))
    for k, size in (("step", 1), ("bc", 2)):
        t = getattr(raw, k)
        bad.append((f"{k} on the host", {k: t.cpu()}))
        bad.append((f"{k} of another dtype", {k: t.double()}))
        bad.append((f"{k} too long",
                    {k: torch.zeros(size + 1, device=DEV)}))
        bad.append((f"{k} empty", {k: torch.zeros(0, device=DEV)}))
    return bad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_operand_checks_reject_before_launch(dtype):
    """Every rejected call stops at a TORCH_CHECK of check_operands,
    which both entry points run before their first launch; nothing is
    written."""
    h = X.HYPERS[0]
    raw = Raw(X.make_case(96, dtype, seed=1), h, dtype)
    untouched = raw.clone()
    for name, over in _bad_operands(raw):
        with pytest.raises(RuntimeError, match="fused_adamw"):
            raw.call(**over)
            pytest.fail(f"accepted: {name}")
    torch.cuda.synchronize()
    for k in raw.bufs:
        assert X.same_bits(raw.bufs[k], untouched.bufs[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_buffers_touch_nothing(dtype):
    h = X.HYPERS[0]
    raw = Raw(X.make_case(0, dtype, seed=1), h, dtype)
    untouched = raw.clone()
    raw.call()
    torch.cuda.synchronize()
    for k in raw.bufs:
        assert X.same_bits(raw.bufs[k], untouched.bufs[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_learning_rate_change_reaches_the_next_step(dtype):
    h = X.Hyper(1, 1e-3, (0.9, 0.999), 1e-8, 0.01, True)
    opt, _ = X.make_optimizer(X.make_case(1543, dtype, 80, cold=True), h,
                              dtype, DEV)
    _step_and_check(opt, X.make_case(1543, dtype, seed=81).g, h,
                    "first lr")
    opt.param_groups[0]["lr"] = 2.5e-4
    _step_and_check(opt, X.make_case(1543, dtype, seed=82).g,
                    h._replace(t=2, lr=2.5e-4), "second lr")
