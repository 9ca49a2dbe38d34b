"""The float64 reference of the depth term (tests/_depth_float64.py), checked on the CPU before any GPU test leans
on it: the restatement against the chain rule through the full Jacobian (no suffix sums, no prefix identities); the fp32
restatement of the kernels' formulation within the derived bound, for both schedules and the three kinds; and that the term is
visible through the fp16 radiance gradients at the weight and loss scale the GPU tests use.  No GPU, no torch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compositor_float64 as c64  # noqa: E402
import _depth_float64 as d64  # noqa: E402

LS, LAMBDA_Z = 128.0, 1.0          # the GPU tests' (tests/test_gpu_depth.py)
SCHEDULES = {32: "pair", 7: "one"}


def pixel_gradients(b, z, kind="l2"):
    """the fp16 pixel gradients a kernel would hand on for an L2 colour loss without a background: half(LS 2 (p - t) / (3 B))"""
    pix = np.zeros((b.B, 3))
    for r, s in enumerate(c64.ray_slices(b)):
        if s.stop > s.start:
            pix[r] = c64.composite_ray(b.rad[s, :3].astype(np.float64), b.rad[s, 3].astype(np.float64), b.step[s].astype(np.float64)).col
    return (LS * 2 * (pix - b.tgt[:, :3]) / (3 * b.B)).astype(np.float16).astype(np.float64)


_RES = {}


def result(K, kind):
    if (K, kind) not in _RES:
        b, z = d64.batch(K)
        g = pixel_gradients(b, z)
        kz = d64.k_factor(LS, LAMBDA_Z, b.B)
        _RES[(K, kind)] = (b, z, g, kz, d64.gradients(b, z, g, SCHEDULES[K], kind, kz))
    return _RES[(K, kind)]


def test_the_batch_is_what_the_issue_asks_for():
    for K in (32, 7):
        b, z = d64.batch(K)
        assert b.B == d64.N_RAYS and set(b.nh.tolist()) == set(d64.SEGMENTS)
        none = ~d64.valid(z)
        assert 0.2 < none.mean() < 0.3 and (z[none] < 0).sum() == 1 and np.isnan(z).sum() == 1 and (z == 0).sum() >= 60


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("kind", d64.KINDS)
def test_restatement_is_the_chain_rule_through_the_full_jacobian(kind, K):
    b, z, g, kz, res = result(K, kind)
    want = d64.closed_form_sigma_gradient(b, z, g, kind, kz)
    scale = np.abs(want).max()
    assert scale > 1e-3
    np.testing.assert_allclose(res.ref[:, 3], want, rtol=1e-9, atol=1e-12 * scale)


def test_restatement_with_every_other_term_active():
    """Huber colour gradients are just numbers here; the alpha gradient, a background and the regulariser's k enter G"""
    b, z = d64.batch(7)
    rng = np.random.default_rng(5)
    g = rng.uniform(-0.05, 0.05, (b.B, 3)).astype(np.float16).astype(np.float64)
    gA = rng.uniform(-0.05, 0.05, b.B).astype(np.float16).astype(np.float64)
    bg = np.tile(np.array([0.9, 0.25, 1.0]), (b.B, 1))
    kz, kd = d64.k_factor(LS, LAMBDA_Z, b.B), d64.k_factor(LS, 10.0, b.B)
    res = d64.gradients(b, z, g, "one", "huber", kz, bg=bg, gA=gA, reg_k=kd)
    want = d64.closed_form_sigma_gradient(b, z, g, "huber", kz, bg=bg, gA=gA, reg_k=kd)
    np.testing.assert_allclose(res.ref[:, 3], want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


def test_a_ray_without_a_target_gets_nothing():
    b, z, g, kz, res = result(32, "l2")
    none = ~d64.valid(z)
    assert np.all(res.gD[none] == 0.0) and np.all(res.lz[none] == 0.0)
    per_sample = np.repeat(none, b.nh.astype(np.int64) * b.K)
    assert np.all(res.depth_part[per_sample] == 0.0) and np.abs(res.depth_part[~per_sample]).max() > 1e-3


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("kind", d64.KINDS)
def test_fp32_restatement_of_the_kernels_lies_within_the_bound(kind, K):
    b, z, g, kz, res = result(K, kind)
    got, D32, l32 = d64.emulate(b, z, g, SCHEDULES[K], kind, kz)
    table = c64.check_elements(f"depth {kind} K={K}", got, res.ref, res.bound, b)
    print("\n".join(c64.table_lines(f"depth {kind} K={K} fp32 restatement", table)))
    assert np.all(np.abs(D32 - res.D) <= res.dD + 1e-300), (np.abs(D32 - res.D) / np.maximum(res.dD, 1e-300)).max()
    assert np.all(np.abs(l32 - res.lz) <= d64.loss_bar(kind, res, z) + 1e-300)


@pytest.mark.parametrize("K", [32, 7])
@pytest.mark.parametrize("kind", d64.KINDS)
def test_the_term_is_visible_through_fp16_at_loss_scale_128(kind, K):
    """lambda_z = 1 at loss scale 128 over 301 rays: the depth addend alone moves the majority of the non-zero sigma-gradients on
    rays with a target by more than their bound, so a kernel without the term cannot pass the GPU comparison.  The shares of the
    float64 reference: K = 32: L2 0.841, L1 0.999, Huber (|l'| <= 0.1) 0.679; K = 7: 0.990, 1.000, 0.981 -- the term does not drown
    in fp16 at 128, so the loss scale stays there."""
    b, z, g, kz, res = result(K, kind)
    share = d64.moved_share(res, z, b)
    print(f"depth {kind} K={K}: the depth addend moves {share:.3f} of the non-zero sigma-gradients on rays with a target by more than the bound")
    assert share > 0.5
