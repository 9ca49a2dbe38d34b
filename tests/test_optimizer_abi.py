"""CPU-side checks of the optimizer options at the C-ABI boundary (rtxn_lr_schedule, rtxn_optimizer_options and the entry points
that take them): the host restatement of the schedule against a float64 numpy one, symbols and bindings, the structs'
layout against the C compiler, and the rules every surface checks before any device is touched -- the Adam entry points, the
one-call step and the Trainer (which raises before allocating)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtxn_lr_schedule_factor", "rtxn_optimizer_options_check", "rtxn_optimizer_rate", "rtxn_check_gradients",
               "rtxn_adam_step_opt", "rtxn_adam_step_sparse_opt", "rtxn_train_step_opt")
CONSTANT, EXPONENTIAL, COSINE = 0, 1, 2
P = C.c_void_p(4096)           # a fake device pointer: never launched from here
WARMUP, START, STEPS = 40, 100, 600


def _header():
    return open(os.path.join(ROOT, "include", "rtxn.h")).read()


# ---- the definition, restated (include/rtxn.h, "optimizer options") ----------------------------------------------------
def factor64(kind, t, warmup_steps=0, decay_start=0, decay_steps=1, ratio=1.0, staircase=False):
    """factor(t) in float64; the ratio is the float32 the struct holds"""
    warm = min(1.0, t / warmup_steps) if warmup_steps > 0 else 1.0
    x = max(0, t - decay_start) / decay_steps
    if staircase:
        x = np.floor(x)
    r = float(np.float32(ratio))
    dec = 1.0 if kind == CONSTANT else r ** x if kind == EXPONENTIAL else r + (1.0 - r) * (1.0 + np.cos(np.pi * min(x, 1.0))) / 2.0
    return warm * dec


def steps_of(warmup=WARMUP, start=START, steps=STEPS):
    """the issue's list: around the warm-up's end, around the decay's start, its middle, its end, one beyond, and 70 000"""
    return [1, warmup - 1, warmup, warmup + 1, start, start + 1, start + steps // 2, start + steps, start + steps + 1, 70_000]


def within_one_ulp(got, want64):
    want = np.float32(want64)
    return abs(np.float32(got) - want) <= np.spacing(want)


SCHEDULES = [dict(kind=CONSTANT, warmup_steps=WARMUP), dict(kind=EXPONENTIAL, warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.1),
             dict(kind=EXPONENTIAL, warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.33, staircase=True),
             dict(kind=EXPONENTIAL, decay_steps=250000, ratio=0.1), dict(kind=COSINE, warmup_steps=WARMUP, decay_start=START, decay_steps=STEPS, ratio=0.1),
             dict(kind=COSINE, decay_steps=STEPS, ratio=1.0)]


def _schedule(_lib, kind=CONSTANT, warmup_steps=0, decay_start=0, decay_steps=0, ratio=1.0, staircase=False):
    s = _lib.LrSchedule()
    s.kind, s.warmup_steps, s.decay_start, s.decay_steps, s.ratio, s.staircase = kind, warmup_steps, decay_start, decay_steps, ratio, int(staircase)
    return s


@pytest.mark.parametrize("kw", SCHEDULES)
def test_host_schedule_factor_matches_the_float64_restatement(kw):
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    s = _schedule(_lib, **kw)
    for t in steps_of():
        got = lib.rtxn_lr_schedule_factor(C.byref(s), t)
        want = factor64(t=t, **{"decay_steps": 1, **kw})
        print(f"{kw} t={t}: {got!r} want {want!r}")
        assert within_one_ulp(got, want), (kw, t, got, want)
    # the shape of it: warm-up rises to 1, the decay never rises
    f = [lib.rtxn_lr_schedule_factor(C.byref(s), t) for t in range(1, START + STEPS + 50)]
    if kw.get("warmup_steps"):
        assert f[0] == np.float32(1.0 / WARMUP) and all(a < b for a, b in zip(f[:WARMUP - 1], f[1:WARMUP]))
    assert all(a >= b for a, b in zip(f[WARMUP:], f[WARMUP + 1:]))


def test_constant_without_warmup_is_exactly_one():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    s = _schedule(_lib)
    for t in steps_of():
        assert lib.rtxn_lr_schedule_factor(C.byref(s), t) == 1.0
        assert api.lr_schedule_factor("constant", t) == 1.0


def test_presets_and_python_forms():
    from rtx_nerf_amd import _lib, api
    n = api.lr_schedule("nerf")
    assert (n.kind, n.decay_start, n.decay_steps, n.staircase) == (EXPONENTIAL, 0, 250000, 0) and n.ratio == np.float32(0.1)
    g = api.lr_schedule("instant_ngp", warmup_steps=5)
    assert (g.kind, g.warmup_steps, g.decay_start, g.decay_steps, g.staircase) == (EXPONENTIAL, 5, 20000, 10000, 1) and g.ratio == np.float32(0.33)
    assert api.lr_schedule_factor("instant_ngp", 29_999) == 1.0 and api.lr_schedule_factor("instant_ngp", 30_000) == float(np.float32(0.33))
    assert within_one_ulp(api.lr_schedule_factor("nerf", 250_000), float(np.float32(0.1)))
    d = api.lr_schedule(dict(kind="cosine", decay_steps=9, ratio=0.5))
    assert isinstance(d, _lib.LrSchedule) and (d.kind, d.decay_steps) == (COSINE, 9) and api.lr_schedule(d) is d
    with pytest.raises(ValueError, match="kind 'linear'"):
        api.lr_schedule("linear")
    with pytest.raises(_lib.RtxnError, match="step = 0"):
        api.lr_schedule_factor("nerf", 0)


def test_optimizer_symbols_are_declared_exported_and_bound():
    from rtx_nerf_amd import _lib, api
    lib = _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding"
        assert hasattr(lib, n), f"{n} not exported by librtxn.so"
        assert re.search(rf"\b{n}\s*\(", _header()), f"{n} not declared in include/rtxn.h"
    for n in ("lr_schedule", "lr_schedule_factor", "optimizer_options", "optimizer_options_check", "optimizer_rate", "check_gradients",
              "adam_step_opt", "adam_step_sparse_opt"):
        assert callable(getattr(api, n))
    import inspect
    assert "optimizer" in inspect.signature(api.train_step).parameters
    assert lib.rtxn_version() == 100


@pytest.mark.parametrize("name,T,fields,want", [
    ("rtxn_lr_schedule", "LrSchedule", ["kind", "warmup_steps", "decay_start", "decay_steps", "ratio", "staircase"], [24, 0, 4, 8, 12, 16, 20]),
    ("rtxn_optimizer_options", "OptimizerOptions", ["schedule", "weight_decay", "skip_nonfinite", "lr_factor", "guard"], [48, 0, 24, 28, 32, 40]),
    ("rtxn_grad_buffer", "GradBuffer", ["data", "count", "is_fp16"], [24, 0, 8, 16])])
def test_struct_layouts_match_the_header_and_the_c_compiler(tmp_path, name, T, fields, want):
    from rtx_nerf_amd import _lib
    src = _header()
    body = src[src.index(f"typedef struct {name} {{"):src.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    declared = [re.findall(r"([A-Za-z_]\w*)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    T = getattr(_lib, T)
    assert declared == [f[0] for f in T._fields_] == fields
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtxn.h"\nint main(void) { printf("' + "%zu " * (len(fields) + 1) + '\\n", '
                 f"sizeof({name}), " + ", ".join(f"offsetof({name}, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT}/include", str(c), "-o", str(exe)])
    got = [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == got == want


# ---- the rules -------------------------------------------------------------------------------------------------------------
# (schedule fields, weight_decay) -> the field the message names
_REJECTED = [(dict(kind=EXPONENTIAL, decay_steps=10, ratio=0.0), 0.0, b"schedule.ratio"),
             (dict(kind=EXPONENTIAL, decay_steps=10, ratio=1.5), 0.0, b"schedule.ratio"),
             (dict(kind=COSINE, decay_steps=10, ratio=-0.1), 0.0, b"schedule.ratio"),
             (dict(kind=CONSTANT, ratio=float("nan")), 0.0, b"schedule.ratio"),
             (dict(kind=EXPONENTIAL, decay_steps=0, ratio=0.5), 0.0, b"schedule.decay_steps"),
             (dict(kind=COSINE, decay_steps=-3, ratio=0.5), 0.0, b"schedule.decay_steps"),
             (dict(kind=CONSTANT, warmup_steps=-1), 0.0, b"schedule.warmup_steps"),
             (dict(kind=EXPONENTIAL, decay_start=-1, decay_steps=10, ratio=0.5), 0.0, b"schedule.decay_start"),
             (dict(kind=COSINE, decay_steps=10, ratio=0.5, staircase=True), 0.0, b"schedule.staircase"),
             (dict(kind=CONSTANT, staircase=True), 0.0, b"schedule.staircase"),
             (dict(kind=7), 0.0, b"schedule.kind"),
             (dict(), -0.01, b"opt->weight_decay"), (dict(), float("nan"), b"opt->weight_decay"), (dict(), float("inf"), b"opt->weight_decay")]


def _options(_lib, sched=None, weight_decay=0.0, skip_nonfinite=0, lr_factor=P, guard=P):
    o = _lib.OptimizerOptions()
    o.schedule = _schedule(_lib, **(sched or {}))
    o.weight_decay, o.skip_nonfinite, o.lr_factor, o.guard = weight_decay, skip_nonfinite, lr_factor, guard
    return o


def _surfaces(_lib, opt):
    """(name, return code, message) of every entry point that takes the struct, on otherwise empty arguments: an accepted struct
    fails later, on the arguments' own checks or for want of a device"""
    lib = _lib.lib()
    args = _lib.TrainStepArgs()
    args.batch.vr_mode, args.batch.sample_type = 1, 3
    o = C.byref(opt) if opt is not None else None
    return [("rtxn_optimizer_options_check", lib.rtxn_optimizer_options_check(o), lib.rtxn_last_error()),
            ("rtxn_adam_step_opt", lib.rtxn_adam_step_opt(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-8, 1.0, o, None), lib.rtxn_last_error()),
            ("rtxn_adam_step_sparse_opt", lib.rtxn_adam_step_sparse_opt(-1, P, P, P, 0, P, P, P, 1e-3, 0.9, 0.999, 1e-15, 1.0, o, None),
             lib.rtxn_last_error()),
            ("rtxn_train_step_opt", lib.rtxn_train_step_opt(C.byref(args), None, None, None, None, o, None), lib.rtxn_last_error()),
            ("rtxn_optimizer_rate", lib.rtxn_optimizer_rate(o, None, 1, 1e-3, 1e-2, 0.9, 0.999, None, None, None), lib.rtxn_last_error())]


@pytest.mark.parametrize("sched,wd,word", _REJECTED)
def test_every_surface_rejects_bad_options_before_touching_a_device(sched, wd, word):
    """RTXN_ERR_INVALID (1) and a message naming the field and the entry point, with or without a GPU"""
    from rtx_nerf_amd import _lib
    for name, rc, msg in _surfaces(_lib, _options(_lib, sched, wd)):
        assert rc == 1 and word in msg and name.encode() in msg, (name, rc, msg)
    if b"schedule" in word:
        s = _schedule(_lib, **sched)
        assert _lib.lib().rtxn_lr_schedule_factor(C.byref(s), 1) == -1.0 and word in _lib.lib().rtxn_last_error()


def test_active_options_need_their_device_words():
    from rtx_nerf_amd import _lib
    for opt, word in ((_options(_lib, weight_decay=0.1, lr_factor=None), b"opt->lr_factor"),
                      (_options(_lib, skip_nonfinite=1, guard=None), b"opt->guard"),
                      (_options(_lib, dict(kind=CONSTANT, warmup_steps=3), lr_factor=None), b"opt->lr_factor")):
        for name, rc, msg in _surfaces(_lib, opt)[1:]:
            assert rc == 1 and word in msg and name.encode() in msg, (name, rc, msg)
        assert _surfaces(_lib, opt)[0][1] == 0           # the rules without the pointers: what the Trainer asks before it allocates


def test_valid_options_reach_the_arguments_own_checks_and_inactive_ones_the_old_entry_points():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    active = _options(_lib, dict(kind=EXPONENTIAL, decay_steps=10, ratio=0.5, staircase=True), 0.1, 1)
    got = {name: (rc, msg) for name, rc, msg in _surfaces(_lib, active)}
    assert got["rtxn_optimizer_options_check"][0] == 0
    assert got["rtxn_adam_step_opt"][0] == 1 and b"rtxn_adam_step_opt: n = -1" in got["rtxn_adam_step_opt"][1]
    assert got["rtxn_adam_step_sparse_opt"][0] == 1 and b"rtxn_adam_step_sparse_opt: n = -1" in got["rtxn_adam_step_sparse_opt"][1]
    assert got["rtxn_train_step_opt"][0] == 1 and b"rtxn_train_step: batch.mlp is NULL" in got["rtxn_train_step_opt"][1]
    assert got["rtxn_optimizer_rate"][0] == 1 and b"rtxn_optimizer_rate: step" in got["rtxn_optimizer_rate"][1]
    # NULL, or a CONSTANT schedule with nothing else: the calls that existed before the struct, under their own names
    for opt in (None, _options(_lib), _options(_lib, lr_factor=None, guard=None)):
        got = {name: (rc, msg) for name, rc, msg in _surfaces(_lib, opt)}
        assert got["rtxn_optimizer_options_check"][0] == 0
        assert got["rtxn_adam_step_opt"][0] == 1 and b"rtxn_adam_step_captured: n = -1" in got["rtxn_adam_step_opt"][1]
        assert got["rtxn_adam_step_sparse_opt"][0] == 1 and b"rtxn_adam_step_sparse: n = -1" in got["rtxn_adam_step_sparse_opt"][1]
        assert got["rtxn_train_step_opt"][0] == 1 and b"rtxn_train_step: batch.mlp is NULL" in got["rtxn_train_step_opt"][1]
    assert lib.rtxn_train_step_opt(None, None, None, None, None, C.byref(active), None) == 1 and b"rtxn_train_step_opt: NULL arguments" in lib.rtxn_last_error()
    assert lib.rtxn_train_step_opt(None, None, None, None, None, None, None) == 1 and b"rtxn_train_step_reg: NULL arguments" in lib.rtxn_last_error()
    assert lib.rtxn_adam_step_opt(4, P, P, P, 8, P, P, P, 1e-3, 0.9, 0.999, 1e-8, 1.0, C.byref(active), None) == 1 and b"grad_flags" in lib.rtxn_last_error()


def test_check_gradients_rejects_bad_lists_before_touching_a_device():
    from rtx_nerf_amd import _lib
    lib = _lib.lib()
    bufs = (_lib.GradBuffer * 5)()
    assert lib.rtxn_check_gradients(bufs, 5, P, None) == 1 and b"n_buffers = 5" in lib.rtxn_last_error()
    assert lib.rtxn_check_gradients(bufs, 1, None, None) == 1 and b"NULL flag" in lib.rtxn_last_error()
    bufs[0].data, bufs[0].count, bufs[0].is_fp16 = None, 3, 0
    assert lib.rtxn_check_gradients(bufs, 1, P, None) == 1 and b"buffers[0].data" in lib.rtxn_last_error()
    bufs[0].data, bufs[0].count = 4098, 3                  # a float buffer on a 2-byte boundary
    assert lib.rtxn_check_gradients(bufs, 1, P, None) == 1 and b"buffers[0].data" in lib.rtxn_last_error()
    bufs[0].count = -1
    assert lib.rtxn_check_gradients(bufs, 1, P, None) == 1 and b"buffers[0].count" in lib.rtxn_last_error()


@pytest.mark.parametrize("kw,word", [(dict(lr_schedule=dict(kind="exponential", decay_steps=10, ratio=0.0)), "schedule.ratio"),
                                     (dict(lr_schedule=dict(kind="exponential", decay_steps=10, ratio=1.5)), "schedule.ratio"),
                                     (dict(lr_schedule=dict(kind="exponential", ratio=0.5)), "schedule.decay_steps"),
                                     (dict(lr_schedule=dict(kind="cosine", decay_steps=0, ratio=0.5)), "schedule.decay_steps"),
                                     (dict(lr_schedule=dict(warmup_steps=-2)), "schedule.warmup_steps"),
                                     (dict(lr_schedule=dict(kind="cosine", decay_start=-1, decay_steps=5, ratio=0.5)), "schedule.decay_start"),
                                     (dict(lr_schedule=dict(kind="cosine", decay_steps=5, ratio=0.5, staircase=True)), "schedule.staircase"),
                                     (dict(lr_schedule="linear"), "kind 'linear'"),
                                     (dict(weight_decay=-1.0), "opt->weight_decay"), (dict(weight_decay=float("nan")), "opt->weight_decay"),
                                     (dict(weight_decay=float("inf")), "opt->weight_decay")])
def test_trainer_refuses_bad_optimizer_options_before_allocating(kw, word):
    from rtx_nerf_amd.train import Trainer
    with pytest.raises(ValueError, match=re.escape(word)):
        Trainer(16, None, encoding="freq", device="cpu", **kw)
