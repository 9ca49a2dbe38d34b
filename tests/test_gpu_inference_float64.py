"""The inference kernels against a float64 evaluation of the same network, layer by layer.

tests/test_gpu_parity.py compares the fused forward with the CPU oracle at atol 1e-2 behind a sigmoid: a 1 % scale error in
one layer of a bias-free ReLU net moves those outputs by about 1e-3 and passes.  Here the yardstick is float64
(tests/_mlp_float64.py: float64 products over the fp16 weights, fp16 only where the format stores a value), and the bar is
not a fixed number but the CPU oracle's OWN distance from float64 on the same inputs, computed in the test:

    rel_rms(kernel, f64) <= F * rel_rms(oracle, f64)        rel_max(kernel, f64) <= F * rel_max(oracle, f64)

The kernels and the oracle round at the same points; they differ by the order of the fp32 sums (the same error distribution)
and by the hardware sine with angle doubling, which test_encoder_error_per_octave bounds at 1 fp16 ulp in under 2 % of the
features.  F started at 3; profiles/r09/inference_float64_anchor.txt holds the ratio measured for every case.  The median is
1.2 and the pre-encoded kernel (no encoder in its path) stays below 1.3, but two one-layer 64-wide cases reach 3.96 and 4.40:
there the oracle differs from float64 in 2 to 36 of 19,792 outputs (one fp16 flip each), so its error is a small-count
statistic, while the encoder's 1-ulp feature differences reach the output through a single layer with nothing to average
them (the kernel: 20 to 170 flips).  Every other case is below 2.7, and no rel_max ratio exceeds 2.  F = 1.5 x 4.40 = 6.6.
F <= 8 is a hard condition: tests/test_mlp_float64_reference.py shows on the CPU that the oracle's error is at most 5e-4 and a
1/64 scale error of any one layer is 1.56e-2, so at F = 8 every negative control below still fails the bar by a factor of
about 4 or more.  A kernel that needs F > 8 is a finding, not a bar to widen.

Negative controls use the kernel's output as it is (nothing else runs on the GPU): against the float64 reference with layer
l scaled by 1 + 1/64 (1 + 1/16 behind the sigmoid) the SAME bar must fail, for every layer of every case.
"""
import numpy as np
import pytest

import _mlp_float64 as F64

pytestmark = pytest.mark.gpu

F_BAR = 6.6              # see the module docstring and profiles/r09/inference_float64_anchor.txt
N = F64.N_BASE
DEPTHS = list(range(1, 9))
LIN, SIG = 0, 1
CASES = [(1, LIN), (3, LIN), (1, SIG)]    # (gain, activation).  Sigmoid at gain 1 only: at gain 3 a deep net's logits reach 1e3 and the
#                                           sigmoid amplifies their rounding noise into 0 / 1 flips -- useless as a bar


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_the_factor_is_within_its_hard_limit():
    assert 3.0 <= F_BAR <= 8.0


def _anchor(tag, got, orc, ref_of, n_layers, control_scale, capsys):
    """got, orc: fp16 [n][C] of the kernel and the oracle; ref_of(scale_layer) -> fp16 [n][C] of the float64 reference."""
    ref = ref_of(None)
    assert np.isfinite(got.astype(np.float32)).all(), tag
    own_rms, own_max = F64.rel_rms(orc, ref), F64.rel_max(orc, ref)
    k_rms, k_max = F64.rel_rms(got, ref), F64.rel_max(got, ref)
    assert own_rms > 0 and own_max > 0, f"{tag}: the oracle equals float64 bit for bit; the case carries no yardstick"
    equal = float((got.view(np.uint16) == ref.view(np.uint16)).mean())
    line = (f"[f64 anchor] {tag}: kernel/oracle rel_rms {k_rms:.3e}/{own_rms:.3e} = {k_rms / own_rms:.2f}  "
            f"rel_max {k_max:.3e}/{own_max:.3e} = {k_max / own_max:.2f}  bit-equal to f64 {100 * equal:.2f} % "
            f"(oracle {100 * float((orc.view(np.uint16) == ref.view(np.uint16)).mean()):.2f} %)")
    with capsys.disabled():
        print("\n" + line)
    assert k_rms <= F_BAR * own_rms, line
    assert k_max <= F_BAR * own_max, line
    for l in range(n_layers):
        d = F64.rel_rms(got, ref_of((l, control_scale)))
        assert d > F_BAR * own_rms, f"{tag}: layer {l} x {control_scale} passes the bar ({d:.3e} <= {F_BAR} x {own_rms:.3e})"


@pytest.mark.parametrize("gain,act", CASES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,ndf", F64.VARIANTS)
def test_forward_against_float64(gpu, oracle, capsys, W, ndf, depth, gain, act):
    """rtxn_mlp_forward, all 16 outputs of 1,237 samples (3 resp. 5 tiles, the last one partial)."""
    torch = gpu
    from rtx_nerf_amd import api
    cfg = oracle.mlp_cfg(n_neurons=W, n_hidden_layers=depth, n_dir_freqs=ndf, output_activation=act)
    E = oracle.mlp_enc_padded(cfg)
    params = F64.gained_params(W, depth, E, seed=W + depth, gain=gain)
    x = F64.base_inputs(N, seed=depth)
    net = api.Network(n_neurons=W, n_hidden_layers=depth, n_dir_freqs=ndf, output_activation=act)
    net.set_params(_dev(torch, params))
    got = net.forward(_dev(torch, x)).cpu().numpy()
    orc = oracle.mlp_forward(cfg, params, x)

    def ref_of(scale_layer):
        r = F64.forward(params, W, depth, inputs=x, n_dir_freqs=ndf, sigmoid=act == SIG, scale_layer=scale_layer)
        assert r.max_hidden < 3e4 and r.max_output < 3e4
        return r.out
    _anchor(f"forward {depth} x {W}, {ndf} octaves, gain {gain}, {'sigmoid' if act else 'linear'}", got, orc, ref_of, depth + 1,
            1 + 1 / 16 if act == SIG else 1 + 1 / 64, capsys)


@pytest.mark.parametrize("gain", [1, 3])
@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("depth", DEPTHS)
def test_pre_encoded_forward_against_float64(gpu, oracle, capsys, depth, E, gain):
    """rtxn_mlp_train_forward_outputs (mlp_enc_fwd16_kernel) on random fp16 features: no encoder in the path."""
    torch = gpu
    from rtx_nerf_amd import api
    params = F64.gained_params(64, depth, E, seed=E + depth, gain=gain)
    feat = np.random.default_rng(E * 10 + depth).uniform(-1, 1, (N, E)).astype(np.float16)
    net = api.Network(n_neurons=64, n_hidden_layers=depth, n_encoded_features=E, output_activation=api.ACT_NONE)
    net.set_params(_dev(torch, params))
    encT = torch.zeros((E, api.padded_samples(N)), dtype=torch.float16, device="cuda")
    encT[:, :N] = _dev(torch, feat).t()
    got = net.train_forward_outputs(encT, N).cpu().numpy()
    orc = oracle.mlpe_forward(64, depth, 0, params, feat)[1]

    def ref_of(scale_layer):
        r = F64.forward(params, 64, depth, features=feat, scale_layer=scale_layer)
        assert r.max_hidden < 3e4 and r.max_output < 3e4
        return r.out
    _anchor(f"train_forward_outputs {depth} x 64, E = {E}, gain {gain}, linear", got, orc, ref_of, depth + 1, 1 + 1 / 64, capsys)


@pytest.mark.parametrize("W,depth", [(128, 3), (256, 1)])
def test_positions_outside_the_cube_against_float64(gpu, oracle, capsys, W, depth):
    """The C ABI accepts any position (the encoder keeps v_fract for it): |x| up to 100, view angles up to +-20, against the
    float64 encoding of the same fp32 inputs, at the same bar."""
    torch = gpu
    from rtx_nerf_amd import api
    cfg = oracle.mlp_cfg(n_neurons=W, n_hidden_layers=depth, output_activation=0)
    E = oracle.mlp_enc_padded(cfg)
    params = F64.gained_params(W, depth, E, seed=W + depth)
    rng = np.random.default_rng(W)
    x = np.concatenate([rng.uniform(-100, 100, (N, 3)), rng.uniform(-20, 20, (N, 2))], axis=1).astype(np.float32)
    x[:8, :3] = [[100, -100, 99.999], [1, -1, 1.5], [-1.5, 37.25, -64], [2, -2, 3], [1e-3, 50.5, -50.5], [7, 11, 13], [-99.5, 0, 0.5],
                 [63.999, -31.001, 15.5]]
    net = api.Network(n_neurons=W, n_hidden_layers=depth, output_activation=api.ACT_NONE)
    net.set_params(_dev(torch, params))
    got = net.forward(_dev(torch, x)).cpu().numpy()
    orc = oracle.mlp_forward(cfg, params, x)
    _anchor(f"forward {depth} x {W}, |x| <= 100, angles <= 20", got, orc,
            lambda sl: F64.forward(params, W, depth, inputs=x, scale_layer=sl).out, depth + 1, 1 + 1 / 64, capsys)


def _ulp16(v):
    """Spacing of fp16 at |v| (float64 array), 2^-24 below the smallest normal."""
    return np.spacing(np.abs(v).astype(np.float16)).astype(np.float64)


@pytest.mark.parametrize("W,depth", [(128, 2), (128, 8), (256, 2)])
def test_sigmoid_epilogue_over_the_whole_logit_range(gpu, W, depth):
    """Two nets on the same weights, one without activation, one with the sigmoid; the output layer scaled so that |z| reaches
    100.  In each output form (half[n][16], float4 radiance, compact half4) the sigmoid output is finite, inside [0, 1], and
    equals the float64 sigmoid of the linear net's fp16 logit to 1 fp16 ulp + 2e-4.  The 2e-4 covers the logit's own fp16
    rounding: |dz| <= 2^-11 |z| moves the sigmoid by at most |z| s'(z) 2^-11 <= 0.224 * 4.9e-4 = 1.1e-4, and by nothing
    where it saturates."""
    torch = gpu
    from rtx_nerf_amd import api
    E = F64.enc_padded(10, 12)
    params = F64.gained_params(W, depth, E, seed=W + depth).astype(np.float32)
    x = F64.base_inputs(N, seed=3)
    zmax = F64.forward(params.astype(np.float16), W, depth, inputs=x).max_output
    params[-16 * W:] *= np.float32(100.0 / zmax)
    params = params.astype(np.float16)
    assert 95 < F64.forward(params, W, depth, inputs=x).max_output < 105
    rng = np.random.default_rng(5)
    P = 39
    start, end = (_dev(torch, rng.uniform(-1, 1, (P, 3)).astype(np.float32)) for _ in range(2))
    view = _dev(torch, np.stack([rng.uniform(0, 3.1416, P), rng.uniform(-3.1416, 3.1416, P)], axis=1).astype(np.float32))
    total = torch.tensor([P], dtype=torch.int32, device="cuda")
    forms = {}
    for act in (api.ACT_NONE, api.ACT_SIGMOID):
        net = api.Network(n_neurons=W, n_hidden_layers=depth, output_activation=act)
        net.set_params(_dev(torch, params))
        x_d = _dev(torch, x)
        rad = torch.zeros((P * 32, 4), device="cuda")
        half = torch.zeros((P * 32, 4), dtype=torch.float16, device="cuda")
        net.forward_segments(start, end, view, total, P, rad)
        net.forward_segments_compact(start, end, view, total, P, half)
        forms[act] = {"half16": net.forward(x_d), "radiance": net.forward_radiance(x_d), "segments float4": rad, "compact half4": half}
    for name in forms[api.ACT_NONE]:
        z = forms[api.ACT_NONE][name].cpu().numpy().astype(np.float64)
        y = forms[api.ACT_SIGMOID][name].cpu().numpy().astype(np.float64)
        assert np.isfinite(z).all() and np.abs(z).max() > 30, name
        assert np.isfinite(y).all() and y.min() >= 0.0 and y.max() <= 1.0, name
        assert y.min() < 1e-3 and y.max() > 0.999, name                        # both saturated ends are exercised
        want = 1.0 / (1.0 + np.exp(-z))
        tol = np.minimum(_ulp16(want), _ulp16(y)) + 2e-4
        worst = np.abs(y - want) - tol
        i = np.unravel_index(np.argmax(worst), worst.shape)
        assert worst[i] <= 0, f"{name}: z = {z[i]}, sigmoid {y[i]} vs float64 {want[i]} (tolerance {tol[i]:.3e})"
