"""A float64 restatement of the inference MLP (plain numpy; a helper module, not a conftest), and the metrics the float64
anchors are stated in.

The network is the one rtxn_mlp_forward evaluates: Composite-Frequency encoding (or pre-encoded fp16 features), fp16 weights
without biases in the tcnn layout ([W][E], (n_hidden - 1) x [W][W], [16][W], row-major [out][in]), ReLU hidden layers whose
activations are STORED in fp16, a 16-row output layer, an optional sigmoid, fp16 output.  Everything between the roundings
the format forces (encoded features, hidden activations, the output) is float64 here: the matrix products, the sine, the
sigmoid.  The kernels and the CPU oracle round at the same points and accumulate in fp32; their distance from this module is
their arithmetic error, and the oracle's is the yardstick the kernels are held to.
"""
from collections import namedtuple

import numpy as np

from rtx_nerf_amd import scenes

Result = namedtuple("Result", "out max_hidden max_output")   # out: fp16 [n][16]; maxima taken BEFORE the fp16 roundings


def enc_padded(n_pos_freqs=10, n_dir_freqs=12, n_pos_dims=3, n_dir_dims=2):
    return (2 * (n_pos_dims * n_pos_freqs + n_dir_dims * n_dir_freqs) + 15) // 16 * 16


def freq_encode(x, n_pos_freqs=10, n_dir_freqs=12, n_pos_dims=3, n_dir_dims=2):
    """float32 [n][5] -> fp16 [n][enc_padded]: feature k of a part is sin(pi * 2^f * x_dim + (k & 1) * pi / 2) with
    dim = k / (2F), f = (k / 2) % F, the sine taken in double on the exact product, rounded to fp16; padded with ones."""
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, n_pos_dims + n_dir_dims)
    cols = []
    for off, nd, F in ((0, n_pos_dims, n_pos_freqs), (n_pos_dims, n_dir_dims, n_dir_freqs)):
        for k in range(2 * nd * F):
            dim, f = k // (2 * F), (k // 2) % F
            cols.append(np.sin(np.pi * np.ldexp(x[:, off + dim], f) + (k & 1) * (np.pi / 2)))
    enc = np.ones((x.shape[0], enc_padded(n_pos_freqs, n_dir_freqs, n_pos_dims, n_dir_dims)), np.float64)
    enc[:, :len(cols)] = np.stack(cols, axis=1)
    return enc.astype(np.float32).astype(np.float16)            # through fp32, as orc_freq_encode's rh((float)sin(arg))


def layers_of(params, W, n_hidden, E):
    """The n_hidden + 1 weight matrices ([out][in], float64 views of the fp16 values) of a tcnn-layout parameter vector."""
    p = np.asarray(params, np.float16).astype(np.float64)
    assert p.size == W * E + (n_hidden - 1) * W * W + 16 * W
    mats, off = [], 0
    for rows, cols in [(W, E)] + [(W, W)] * (n_hidden - 1) + [(16, W)]:
        mats.append(p[off:off + rows * cols].reshape(rows, cols))
        off += rows * cols
    return mats


def forward(params, W, n_hidden, *, inputs=None, features=None, n_pos_freqs=10, n_dir_freqs=12, sigmoid=False, scale_layer=None):
    """inputs: float32 [n][5] (encoded here), or features: fp16 [n][E] (pre-encoded).  scale_layer = (l, s): layer l's weights
    (0 .. n_hidden, the last being the output layer) times s -- the negative controls.  Returns Result."""
    assert (inputs is None) != (features is None)
    a = (freq_encode(inputs, n_pos_freqs, n_dir_freqs) if features is None else np.asarray(features, np.float16)).astype(np.float64)
    mats = layers_of(params, W, n_hidden, a.shape[1])
    if scale_layer is not None:
        l, s = scale_layer
        mats[l] = mats[l] * float(s)
    max_hidden = 0.0
    for m in mats[:-1]:
        h = np.maximum(a @ m.T, 0.0)
        max_hidden = max(max_hidden, float(h.max()))
        a = h.astype(np.float16).astype(np.float64)              # the activations are stored in fp16
    z = a @ mats[-1].T
    y = 1.0 / (1.0 + np.exp(-z)) if sigmoid else z
    with np.errstate(over="ignore"):
        out = y.astype(np.float16)
    return Result(out, max_hidden, float(np.abs(z).max()))


# ---------------------------------------------------------------------------------------------------- metrics
def _f64(a):
    return np.asarray(a).astype(np.float64)


def rms(a):
    return float(np.sqrt(np.mean(np.square(_f64(a)))))


def rel_rms(a, ref):
    """rms(a - ref) / rms(ref)"""
    return rms(_f64(a) - _f64(ref)) / rms(ref)


def rel_max(a, ref):
    """max |a - ref| / max |ref|"""
    return float(np.abs(_f64(a) - _f64(ref)).max() / np.abs(_f64(ref)).max())


# ---------------------------------------------------------------------------------------------------- the shared cases
N_BASE = 1237            # 1237 mod 16, 64, 512 = 5, 21, 213: base-set copies land on every column, wave and tile offset
VARIANTS = [(128, 12), (64, 12), (128, 4), (64, 4), (256, 12)]   # (width, direction octaves) of the five built kernels


def base_inputs(n=N_BASE, seed=0):
    """Positions in [-1, 1]^3, view angles theta in [0, pi], phi in [-pi, pi]: float32 [n][5]."""
    rng = np.random.default_rng(1000 + seed)
    return np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 3.1416, (n, 1)), rng.uniform(-3.1416, 3.1416, (n, 1))],
                          axis=1).astype(np.float32)


def gained_params(W, n_hidden, E, seed, gain=1):
    """Xavier-uniform weights times `gain` in every layer, fp16."""
    p = scenes.xavier_params_fp16(W, n_hidden, E, seed=seed).astype(np.float32)
    return (p * np.float32(gain)).astype(np.float16)
