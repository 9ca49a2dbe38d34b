"""The float64 restatement of the inference MLP (tests/_mlp_float64.py) against the CPU oracle -- no GPU.

tests/test_gpu_inference_float64.py holds the kernels to F times the oracle's own distance from float64, F <= 8, and needs
every one-layer scale error of 1/64 to break that bar.  Both halves are checkable here: the oracle sits within 5e-4 of
float64 (relative RMS; measured 1.3e-5 for 1 x 128 up to 2.9e-4 for 8 x 256), a 1/64 scale of any single layer sits 1.56e-2
away -- ReLU without biases is positively homogeneous, so the scale passes straight through to the output -- and nothing
leaves the fp16 range, so the comparison is between finite numbers.
"""
import numpy as np
import pytest

import _mlp_float64 as F64

N = F64.N_BASE


@pytest.mark.parametrize("gain", [1, 3])
@pytest.mark.parametrize("depth", [1, 2, 4, 8])
@pytest.mark.parametrize("W", [64, 128, 256])
def test_oracle_sits_on_the_float64_reference(oracle, W, depth, gain, capsys):
    cfg = oracle.mlp_cfg(n_neurons=W, n_hidden_layers=depth, n_dir_freqs=12, output_activation=0)
    E = oracle.mlp_enc_padded(cfg)
    assert E == F64.enc_padded(10, 12)
    params = F64.gained_params(W, depth, E, seed=W + depth, gain=gain)
    x = F64.base_inputs(N, seed=depth)
    orc = oracle.mlp_forward(cfg, params, x)
    ref = F64.forward(params, W, depth, inputs=x, n_dir_freqs=12)
    assert ref.out.shape == orc.shape == (N, 16)
    # nothing overflows fp16 on the way (gain 3, depth 8: output RMS about 1.2e3)
    assert ref.max_hidden < 3e4 and ref.max_output < 3e4, (ref.max_hidden, ref.max_output)
    assert np.isfinite(orc.astype(np.float32)).all() and np.isfinite(ref.out.astype(np.float32)).all()
    own = F64.rel_rms(orc, ref.out)
    lines = [f"{depth} x {W} gain {gain}: oracle vs float64 rel rms {own:.2e} rel max {F64.rel_max(orc, ref.out):.2e}, "
             f"output rms {F64.rms(ref.out):.3g}, max hidden {ref.max_hidden:.3g}"]
    assert own <= 5e-4, lines[0]
    # the encoder of the restatement is the oracle's: same features, bit for bit
    np.testing.assert_array_equal(F64.freq_encode(x[:64], 10, 12), oracle.encode_freq(cfg, x[:64]))
    ctl = []
    for l in range(depth + 1):
        off = F64.forward(params, W, depth, inputs=x, n_dir_freqs=12, scale_layer=(l, 1 + 1 / 64))
        ctl.append(F64.rel_rms(off.out, orc))
        assert ctl[-1] >= 1.5e-2, f"{lines[0]}\n  layer {l} x (1 + 1/64): rel rms {ctl[-1]:.2e}"
    with capsys.disabled():
        print("\n" + lines[0] + f"; one layer x (1 + 1/64): {min(ctl):.2e} .. {max(ctl):.2e}")


def test_restatement_reads_the_tcnn_layout_and_applies_its_controls():
    """Hand-checkable: a 1 x 64 net on pre-encoded features whose weights select single features; scale_layer scales one layer
    only; the sigmoid is applied to the float64 logit, not to its fp16 rounding."""
    W, E = 64, 32
    p = np.zeros(W * E + 16 * W, np.float16)
    w0, wo = p[:W * E].reshape(W, E), p[W * E:].reshape(16, W)
    w0[3, 5] = 2.0          # hidden 3 = 2 * feature 5
    w0[7, 9] = -1.0         # hidden 7 = relu(-feature 9)
    wo[0, 3] = 1.0
    wo[1, 7] = 1.0
    wo[2, 3] = 0.5
    feat = np.zeros((2, E), np.float16)
    feat[0, 5], feat[0, 9] = 0.75, 0.5
    feat[1, 5], feat[1, 9] = -0.25, -1.5
    r = F64.forward(p, W, 1, features=feat)
    np.testing.assert_array_equal(r.out[:, :3].astype(np.float32), [[1.5, 0.0, 0.75], [0.0, 1.5, 0.0]])
    assert r.max_hidden == 1.5 and r.max_output == 1.5
    r0 = F64.forward(p, W, 1, features=feat, scale_layer=(0, 2.0))
    r1 = F64.forward(p, W, 1, features=feat, scale_layer=(1, 2.0))
    np.testing.assert_array_equal(r0.out, r1.out)
    np.testing.assert_array_equal(r0.out.astype(np.float32), 2 * r.out.astype(np.float32))
    s = F64.forward(p, W, 1, features=feat, sigmoid=True)
    np.testing.assert_array_equal(s.out[0, :2], np.array([1 / (1 + np.exp(-1.5)), 0.5]).astype(np.float16))
    assert F64.rel_rms([1.0, 1.0], [1.0, 2.0]) == pytest.approx(np.sqrt(0.5) / np.sqrt(2.5))
    assert F64.rel_max([1.0, 1.0], [1.0, 2.0]) == 0.5
