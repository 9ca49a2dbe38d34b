"""Where two Adam rules coincide, their kernels agree in every bit: the six Adam kernels are one dense and one
sparse walk under different element rules, and this is the property that makes the shared walk legitimate.  Options that are
active but neutral -- skip_nonfinite set over clean gradients, a constant schedule (factor exactly 1), no decay -- put the _opt
kernels on the rule of the plain ones: rtxn_adam_step_captured against rtxn_adam_step_opt on one rate buffer, and
rtxn_adam_step_sparse against rtxn_adam_step_sparse_opt.  test_gpu_optimizer.py holds one such step (fp32, aligned, no clearing),
test_gpu_ema.py the _ema kernels against the _opt ones and test_gpu_loss_scaler.py the device multiplier against the value.

n = 4099: 1024 quads and a 3-element tail, more than one block; offset 1 takes the all-scalar path.  Three steps, so the second
and third start from moments and update counts that are not zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, LR, LOSS_SCALE = 4_099, 3, 1e-2, 2.0


def _views(torch, n, offset, *dtypes):
    """zeroed tensors of n elements that start `offset` elements into their allocation (offset 1: no 16-byte alignment)"""
    return [torch.zeros(n + 8, dtype=dt, device="cuda")[offset:offset + n] for dt in dtypes]


def _bits(torch, x):
    return x.view({2: torch.int16, 4: torch.int32}[x.element_size()])


def _neutral_options(torch, api):
    factor = torch.zeros(1, device="cuda")
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    return api.optimizer_options(None, 0.0, True, factor, guard), factor, guard


def _gradients(half, sparse):
    """the gradients of the three steps.  sparse: about half the elements are exact zeros, a different half each step; quad 5 is
    all zero, quad 9 holds -0.0 beside non-zeros, quad 13 holds only +-0 (in fp16: words the 0x7fff7fff mask must let through),
    and the last tail element is zero"""
    rng = np.random.default_rng(31 + 2 * half + sparse)
    out = []
    for _ in range(STEPS):
        g = (rng.standard_normal(N) * 0.3).astype(np.float16 if half else np.float32)
        assert (g != 0).all()
        if sparse:
            g[rng.uniform(size=N) < 0.5] = 0
            g[20:24] = 0
            g[36:40] = np.array([-0.0, 0.25, -0.0, -0.5], g.dtype)
            g[52:56] = np.array([-0.0, 0.0, -0.0, -0.0], g.dtype)
            g[N - 1] = 0
            assert 0.4 < (g == 0).mean() < 0.6 and np.signbit(g[36]) and np.signbit(g[52])
        out.append(g)
    return out


class _State:
    def __init__(self, torch, offset, half):
        self.w, self.m, self.v, self.p, self.s = _views(torch, N, offset, torch.float32, torch.float32, torch.float32, torch.float16, torch.int32)
        self.g, = _views(torch, N, offset, torch.float16 if half else torch.float32)
        self.w.copy_(torch.from_numpy(np.random.default_rng(5).standard_normal(N).astype(np.float32)))
        self.p.copy_(self.w.half())

    def tensors(self):
        return {"master": self.w, "params": self.p, "m": self.m, "v": self.v, "param_steps": self.s, "grads": self.g}


def _run_pair(torch, grads, offset, step_a, step_b, before_step=lambda: None):
    """STEPS steps of the two calls side by side, from one start and on copies of one gradient; after every step every tensor of
    the two states -- the gradient buffer among them -- holds the same bits.  Returns the first state."""
    half = grads[0].dtype == np.float16
    a, b = _State(torch, offset, half), _State(torch, offset, half)
    start = a.w.clone()
    for t, g in enumerate(grads):
        before_step()
        for st, step in ((a, step_a), (b, step_b)):
            st.g.copy_(torch.from_numpy(g))
            step(st)
        for (k, x), y in zip(a.tensors().items(), b.tensors().values()):
            assert torch.equal(_bits(torch, x), _bits(torch, y)), (k, t + 1)
    assert bool(torch.isfinite(a.w).all()) and not torch.equal(a.w, start) and torch.equal(a.p, a.w.half())
    return a


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_dense_opt_kernel_under_neutral_options_is_the_captured_kernel(gpu, half_grads, offset, zero):
    torch = gpu
    from rtx_nerf_amd import api
    opt, factor_d, guard = _neutral_options(torch, api)
    step_d, rate_d = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    grads = _gradients(half_grads, False)
    a = _run_pair(torch, grads, offset,
                  lambda s: api.adam_step_captured(s.w, s.p, s.g, s.m, s.v, rate_d, loss_scale=LOSS_SCALE, zero_grads=zero),
                  lambda s: api.adam_step_opt(s.w, s.p, s.g, s.m, s.v, rate_d, opt, lr=LR, loss_scale=LOSS_SCALE, zero_grads=zero),
                  before_step=lambda: api.optimizer_rate(opt, step_d, rate_d, lr=LR))       # both read this step's rate from rate_d
    assert float(factor_d.item()) == 1.0 and guard.tolist() == [0, 0, 0, 0] and int(step_d.item()) == STEPS
    left = _bits(torch, a.g).cpu().numpy()
    assert (not left.any()) if zero else np.array_equal(left, grads[-1].view(left.dtype))
    assert not a.s.any()


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("half_grads", [False, True])
def test_sparse_opt_kernel_under_neutral_options_is_the_sparse_kernel(gpu, half_grads, offset, zero):
    torch = gpu
    from rtx_nerf_amd import api
    opt, factor_d, guard = _neutral_options(torch, api)
    step_d, rate_d = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    api.optimizer_rate(opt, step_d, rate_d, lr=LR)          # the factor (exactly 1) and a clear skip word
    assert float(factor_d.item()) == 1.0 and guard.tolist() == [0, 0, 0, 0]
    grads = _gradients(half_grads, True)
    a = _run_pair(torch, grads, offset,
                  lambda s: api.adam_step_sparse(s.w, s.p, s.g, s.m, s.v, s.s, lr=LR, eps=1e-15, loss_scale=LOSS_SCALE, zero_grads=zero),
                  lambda s: api.adam_step_sparse_opt(s.w, s.p, s.g, s.m, s.v, s.s, opt, lr=LR, eps=1e-15, loss_scale=LOSS_SCALE, zero_grads=zero))
    counts = a.s.cpu().numpy()
    assert np.array_equal(counts, sum((g != 0).astype(np.int32) for g in grads))
    assert not counts[20:24].any() and not counts[52:56].any() and counts[36] == 0 and counts[37] == STEPS
    left = _bits(torch, a.g).cpu().numpy()
    if not zero:
        assert np.array_equal(left, grads[-1].view(left.dtype))
    else:
        # what the walk passes over keeps its bits (the -0.0 of the +-0 quad); a quad it consumes is cleared whole, a scalar
        # element only where it is not zero
        assert left[52] != 0 and left[37] == 0 and left[39] == 0 and [left[36] == 0, left[38] == 0] == [offset == 0] * 2
        assert not (left & (0x7fff if half_grads else 0x7fffffff)).any()
