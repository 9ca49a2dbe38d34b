"""CPU-side checks of the weight EMA at the C-ABI boundary (rtxn_weight_ema and the entry points that take it):
symbols and bindings, the structs' layout against the C compiler, the one rule every surface checks before any device is
touched, the Trainer (which raises before allocating), and the host twins of the device arithmetic against the float64
recurrence."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_weight_ema_check", "rtxn_ema_catch_up", "rtxn_ema_correction", "rtxn_optimizer_rate_ema", "rtxn_loss_scaler_step_ema",
               "rtxn_adam_step_ema", "rtxn_adam_step_sparse_ema", "rtxn_ema_weights", "rtxn_train_step_ema")
P = C.c_void_p(4096)           # a fake device pointer: never launched from here
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


def test_ema_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    for n in ("weight_ema", "ema_catch_up", "ema_correction", "optimizer_rate_ema", "loss_scaler_step_ema", "adam_step_ema",
              "adam_step_sparse_ema", "ema_weights"):
        assert callable(getattr(api, n))
    assert "ema" in inspect.signature(api.train_step).parameters
    from rtx_nerf_amd.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["ema_decay"].default is None
    assert inspect.signature(Trainer.render_pipeline).parameters["weights"].default == "live"
    for n in ("ema_parameters", "sync_ema"):
        assert callable(getattr(Trainer, n))
    assert isinstance(Trainer.ema_updates, property)
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("name,T,fields,want", [
    ("rtxn_weight_ema", "WeightEma", ["decay", "state", "mlp_ema", "table_ema", "table_stamps"], [40, 0, 8, 16, 24, 32]),
    ("rtxn_ema_state", "EmaState", ["updates", "correction", "reserved"], [16, 0, 4, 8])])
def test_struct_layouts_match_the_header_and_the_c_compiler(tmp_path, name, T, fields, want):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = [re.findall(r"([A-Za-z_]\w*)\s*(?:\[\d+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    T = getattr(_lib, T)
    assert declared == [f[0] for f in T._fields_] == fields
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(fields) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == got == want


# ---- the rule ---------------------------------------------------------------------------------------------------------------
_REJECTED = [0.0, 1.0, -0.1, float("nan"), float("inf")]


def _ema(_lib, decay=0.9, state=P, mlp=P, table=P, stamps=P):
    e = _lib.WeightEma()
    e.decay, e.state, e.mlp_ema, e.table_ema, e.table_stamps = decay, state, mlp, table, stamps
    return e


def _options(_lib, skip_nonfinite=0, lr_factor=P, guard=None):
    o = _lib.OptimizerOptions()
    o.schedule.ratio = 1.0
    o.skip_nonfinite, o.lr_factor, o.guard = skip_nonfinite, lr_factor, guard
    return o


def _surfaces(_lib, ema, opt=None):
    """(name, return code, message) of every entry point that takes the struct, on otherwise empty arguments: an accepted struct
    fails later, on the arguments' own checks or for want of a device"""
    lib = _lib.lib()
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type = 1, 3
    e, o = C.byref(ema), C.byref(opt if opt is not None else _options(_lib))
    return [("rtxn_weight_ema_check", lib.rtxn_weight_ema_check(e), lib.rtxn_last_error()),
            ("rtxn_optimizer_rate_ema", lib.rtxn_optimizer_rate_ema(o, e, None, 1, 1e-3, 1e-2, 0.9, 0.999, None, None, None), lib.rtxn_last_error()),
            ("rtxn_adam_step_ema", lib.rtxn_adam_step_ema(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-8, 1.0, o, None, e, P, None),
             lib.rtxn_last_error()),
            ("rtxn_adam_step_sparse_ema", lib.rtxn_adam_step_sparse_ema(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-15, 1.0, o, None, e, P, P, None),
             lib.rtxn_last_error()),
            ("rtxn_ema_weights", lib.rtxn_ema_weights(-1, P, P, P, ema.state, ema.decay, P, None, None), lib.rtxn_last_error()),
            ("rtxn_train_step_ema", lib.rtxn_train_step_ema(C.byref(args), None, None, None, None, o, None, e, None), lib.rtxn_last_error())]


@pytest.mark.parametrize("decay", _REJECTED)
def test_every_surface_refuses_a_decay_outside_the_open_interval(decay):
    """RTXN_ERR_INVALID (1) and a message naming the field and the entry point, with or without a GPU"""
    from rtx_nerf_amd import _lib, api
    for name, rc, msg in _surfaces(_lib, _ema(_lib, decay)):
        assert rc == 1 and b"decay" in msg and (name.encode() in msg or name == "rtxn_train_step_ema"), (name, rc, msg)
    with pytest.raises(_lib.RtxnError, match="decay"):
        api.weight_ema(decay)
    lib = _lib.lib()
    assert lib.rtxn_ema_correction(decay, 3) == -1.0 and b"rtxn_ema_correction: decay" in lib.rtxn_last_error()
    assert np.isnan(lib.rtxn_ema_catch_up(1.0, 2.0, 3, decay)) and b"rtxn_ema_catch_up: decay" in lib.rtxn_last_error()
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(16, None, encoding="freq", device="cpu", ema_decay=decay)


def test_a_valid_struct_reaches_the_arguments_own_checks_and_null_the_calls_without_it():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    assert lib.rtxn_weight_ema_check(None) == 0                   # NULL is valid: no EMA
    for d in (0.5, 0.9, 0.9999, float(np.nextafter(F(1), F(0))), 1e-30):
        assert lib.rtxn_weight_ema_check(C.byref(_ema(_lib, d, None, None, None, None))) == 0
    got = {name: (rc, msg) for name, rc, msg in _surfaces(_lib, _ema(_lib))}
    assert got["rtxn_weight_ema_check"][0] == 0
    assert got["rtxn_optimizer_rate_ema"][0] == 1 and b"rtxn_optimizer_rate_ema: step" in got["rtxn_optimizer_rate_ema"][1]
    assert got["rtxn_adam_step_ema"][0] == 1 and b"rtxn_adam_step_ema: n = -1" in got["rtxn_adam_step_ema"][1]
    assert got["rtxn_adam_step_sparse_ema"][0] == 1 and b"rtxn_adam_step_sparse_ema: n = -1" in got["rtxn_adam_step_sparse_ema"][1]
    assert got["rtxn_ema_weights"][0] == 1 and b"rtxn_ema_weights: n = -1" in got["rtxn_ema_weights"][1]
    assert got["rtxn_train_step_ema"][0] == 1 and b"batch.mlp is NULL" in got["rtxn_train_step_ema"][1]
    # the state words: needed by everything that launches, not by the rule alone
    for name, rc, msg in _surfaces(_lib, _ema(_lib, state=None))[1:]:
        assert rc == 1 and b"state" in msg and name.encode() in msg, (name, rc, msg)
    # the rate comes from the rate kernel: options with lr_factor, switched on or not; the guard is not implied
    for opt in (_options(_lib, lr_factor=None),):
        for name, rc, msg in _surfaces(_lib, _ema(_lib), opt):
            if name not in ("rtxn_weight_ema_check", "rtxn_ema_weights"):
                assert rc == 1 and name.encode() in msg and b"lr_factor" in msg, (name, msg)
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type = 1, 3
    assert lib.rtxn_train_step_ema(C.byref(args), None, None, None, None, None, None, C.byref(_ema(_lib)), None) == 1
    assert b"rtxn_train_step_ema" in lib.rtxn_last_error() and b"lr_factor" in lib.rtxn_last_error()
    for name, rc, msg in _surfaces(_lib, _ema(_lib), _options(_lib, skip_nonfinite=1, guard=None)):
        if name in ("rtxn_adam_step_ema", "rtxn_adam_step_sparse_ema", "rtxn_train_step_ema"):
            assert rc == 1 and b"guard" in msg, (name, msg)
    # NULL ema: the calls that existed before the struct, under their own names
    o = C.byref(_options(_lib, skip_nonfinite=1, guard=P))
    assert lib.rtxn_train_step_ema(None, None, None, None, None, None, None, None, None) == 1
    assert b"rtxn_train_step_reg: NULL arguments" in lib.rtxn_last_error()
    assert lib.rtxn_adam_step_ema(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-8, 1.0, o, None, None, None, None) == 1
    assert b"rtxn_adam_step_opt: n = -1" in lib.rtxn_last_error()
    assert lib.rtxn_adam_step_sparse_ema(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-15, 1.0, o, None, None, None, None, None) == 1
    assert b"rtxn_adam_step_sparse_opt: n = -1" in lib.rtxn_last_error()
    assert lib.rtxn_optimizer_rate_ema(o, None, None, 1, 1e-3, 1e-2, 0.9, 0.999, None, None, None) == 1
    assert b"rtxn_optimizer_rate_ema: step" in lib.rtxn_last_error()
    # the sparse rule keeps the average lazily: no stamps, no call
    assert lib.rtxn_train_step_ema(C.byref(args), None, None, None, None, o, None, C.byref(_ema(_lib, mlp=None)), None) == 1
    assert b"mlp_ema" in lib.rtxn_last_error()


# ---- the host twins against float64 -------------------------------------------------------------------------------------------
def _recurrence64(s, w, gap, d, cap=400_000):
    """`gap` steps of s = d s + (1 - d) w in float64 over a constant w, for arrays of cases at once (d: the floats the library
    holds, widened).  Iterated, not the closed form: the closed form is what is under test.  The cases are sorted by gap and each
    leaves the loop at its own step; past `cap` steps nothing moves any more (0.9999^400000 < 1e-17), so the loop ends there."""
    order = np.argsort(gap, kind="stable")
    S, W, D, G = s[order].astype(np.float64), w[order].astype(np.float64), d[order].astype(np.float64), gap[order]
    first = int(np.searchsorted(G, 1))
    for k in range(1, int(min(G[-1], cap)) + 1):
        S[first:] = D[first:] * S[first:] + (1.0 - D[first:]) * W[first:]
        first = int(np.searchsorted(G, k + 1))
        if first == len(G):
            break
    out = np.empty_like(S)
    out[order] = S
    return out


def test_catch_up_agrees_with_the_float64_recurrence():
    """2 000 random (s, w, gap, d), gap 0 .. 10^6: within 2^-22 (|s| + |w|) of `gap` steps of the float64 recurrence -- the catch-up
    commits one multiply-add and one exp2, and is a contraction."""
    from rtx_nerf_amd import api
    rng = np.random.default_rng(20260)
    n = 2000
    d = rng.choice(np.array([0.5, 0.9, 0.99, 0.9999], dtype=F), n)
    top = rng.choice([4, 100, 10_000, 1_000_001], n)                    # every decade of gaps, the small ones as often as the large
    gap = np.minimum(rng.integers(0, top), 1_000_000)
    gap[:8] = [0, 1, 2, 1_000_000, 999_999, 0, 3, 65_536]
    s = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, n)).astype(F)
    w = (rng.normal(size=n) * 10.0 ** rng.integers(-4, 2, n)).astype(F)
    want = _recurrence64(s, w, gap, d)
    got = np.array([api.ema_catch_up(s[k], w[k], gap[k], d[k]) for k in range(n)], dtype=F)
    assert (gap == 0).sum() >= 2 and (gap > 100_000).sum() > 100
    assert got[gap == 0].tobytes() == s[gap == 0].tobytes()            # gap == 0 returns s bit for bit
    err = np.abs(got.astype(np.float64) - want)
    bar = 2.0 ** -22 * (np.abs(s.astype(np.float64)) + np.abs(w.astype(np.float64)))
    print(f"rtxn_ema_catch_up: worst error / bar = {(err / bar).max():.3f}")
    k = int(np.argmax(err / bar))
    assert (err <= bar).all(), (s[k], w[k], gap[k], d[k], got[k], want[k])


def test_gap_zero_returns_s_bit_for_bit():
    """w + 1 (s - w) is not s in fp32: the host twin must skip the line, as the kernel does"""
    from rtx_nerf_amd import api
    rng = np.random.default_rng(7)
    differs = 0
    for _ in range(500):
        s, w = F(rng.normal()), F(rng.normal() * 1e3)
        assert F(api.ema_catch_up(s, w, 0, 0.99)).tobytes() == s.tobytes()
        differs += F(w + F(s - w)).tobytes() != s.tobytes()
    assert differs > 0                                     # the evaluated form would have been caught by this very data
    for s in (F(-0.0), F(np.inf), F(1e-45)):
        assert F(api.ema_catch_up(s, 1.0, 0, 0.5)).tobytes() == s.tobytes()


def test_correction_is_the_float64_debias_factor_rounded_once():
    """correction(0) = 1: the read-out at u = 0 is the weight itself, and 1 is the factor that says so; u >= 1: (float)(1 / (1 -
    d^u)) with d widened from the float the library holds"""
    from rtx_nerf_amd import api
    assert api.ema_correction(0.9, 0) == 1.0 and api.ema_correction(0.9999, 0) == 1.0
    for d in (0.5, 0.9, 0.99, 0.9999):
        for u in (1, 2, 3, 10, 59, 60, 1000, 200_000, 4_000_000_000):
            want = F(1.0 / (1.0 - np.float64(F(d)) ** np.float64(u)))
            got = F(api.ema_correction(d, u))
            assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1, (d, u, got, want)
        assert api.ema_correction(d, 4_000_000_000) == 1.0
    assert F(api.ema_correction(0.5, 1)).tobytes() == F(2.0).tobytes()


def test_trainer_refuses_a_decay_that_is_no_number_before_allocating():
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(16, None, encoding="freq", device="cpu", ema_decay="0.9x")
