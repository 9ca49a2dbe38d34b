"""The sizes of the training workspaces, pinned (no GPU: a model handle and the *_workspace_bytes entries are host code).

train.hip lays both MLP training workspaces out in one host struct (TrainWs) that the size entries, the forward and the
backward launchers all read; the literals below were recorded from the library as it was BEFORE that struct existed, when
each of the six places spelled the arithmetic out by hand, so a slip in the struct shows here as a size that moved.
n_samples straddles the 256-sample tile (0, 1, 256 | 257: a second tile holding one sample), capacities straddle the 16-byte
padding of the live-segment flags."""
import ctypes as C

import pytest

# (n_neurons, n_hidden_layers) -> {n_samples: (rtxn_mlp_train_workspace_bytes, rtxn_mlp_train_lean_workspace_bytes)}
# (the lean path is built for the 8 x 128 model only: 0 for the other)
MLP_WORKSPACE_BYTES = {
    (64, 4): {0: (0, 0), 1: (286736, 0), 256: (286736, 0), 257: (573456, 0), 4096: (4587536, 0)},
    (128, 8): {0: (0, 0), 1: (1089552, 565264), 256: (1089552, 565264), 257: (2179088, 1130512), 4096: (17432592, 9043984)},
}
LIVE_WORKSPACE_BYTES = {0: 16, 1: 36, 15: 92, 16: 96, 17: 116}


@pytest.mark.parametrize("width,layers", sorted(MLP_WORKSPACE_BYTES))
def test_mlp_training_workspace_sizes_are_pinned(width, layers):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    cfg = _lib.MlpConfig(3, 10, 2, 12, width, layers, 4, 1)
    h = C.c_void_p()
    assert lib.rtxn_mlp_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert lib.rtxn_mlp_train_lean_supported(h) == int((width, layers) == (128, 8))
        got = {n: (lib.rtxn_mlp_train_workspace_bytes(h, n), lib.rtxn_mlp_train_lean_workspace_bytes(h, n))
               for n in MLP_WORKSPACE_BYTES[(width, layers)]}
        assert got == MLP_WORKSPACE_BYTES[(width, layers)]
        assert lib.rtxn_mlp_train_workspace_bytes(h, -1) == 0 and lib.rtxn_mlp_train_lean_workspace_bytes(h, -1) == 0
        assert lib.rtxn_mlp_train_workspace_bytes(None, 256) == 0 and lib.rtxn_mlp_train_lean_workspace_bytes(None, 256) == 0
    finally:
        assert lib.rtxn_mlp_destroy(h) == 0


def test_live_segment_workspace_sizes_are_pinned():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert {c: lib.rtxn_live_segments_workspace_bytes(c) for c in LIVE_WORKSPACE_BYTES} == LIVE_WORKSPACE_BYTES
    assert lib.rtxn_live_segments_workspace_bytes(-1) == 0
