"""numpy-only float64 restatement of rtxn_image_metrics' record (include/rtxn.h): mse, psnr and the Wang et al. 2004 SSIM (11 x 11
Gaussian window, sigma 1.5, K1 0.01, K2 0.03, L 1, valid windows, mean over windows and channels).  The TARGET is formed in float32
exactly as the kernel forms it (u8 -> (float)v / 255.0f, RGBA over a background with one fused multiply-add) and then promoted, so
a comparison against the kernel measures the metric and not the target."""
import numpy as np

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
C1, C2 = K1 * K1, K2 * K2


def window():
    """the 11 normalised Gaussian weights, float64"""
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def target_f32(images, image, background=None):
    """frame `image` of images [N, H, W, C] (uint8 or float32, C = 3 | 4) as the kernel reads it: float32 [H, W, 3]"""
    f = np.asarray(images)[image]
    if f.dtype == np.uint8:
        f = f.astype(np.float32) / np.float32(255.0)
    else:
        f = f.astype(np.float32, copy=False)
    if f.shape[-1] == 3:
        return f
    bg = np.asarray(background, dtype=np.float32).reshape(1, 1, 3)
    a = f[..., 3:4]
    tail = (np.float32(1.0) - a) * bg                                          # float32 product, rounded once
    # fmaf(a, rgb, tail): the product is exact in float64, one rounding of the sum to float64 and one to float32
    return (a.astype(np.float64) * f[..., :3].astype(np.float64) + tail.astype(np.float64)).astype(np.float32)


def _filter_valid(x, w):
    """[H, W, ...] -> [H - 10, W - 10, ...]: the separable window, rows then columns, valid positions only"""
    H, W = x.shape[:2]
    h = sum(w[k] * x[:, k:k + W - WIN + 1] for k in range(WIN))
    return sum(w[k] * h[k:k + H - WIN + 1] for k in range(WIN))


def ssim_map(x, y):
    """per-window, per-channel SSIM of two float64 [H, W, 3] images: [H - 10, W - 10, 3]"""
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), window()
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError("ssim needs frames of at least 11 x 11")
    mx, my = _filter_valid(x, w), _filter_valid(y, w)
    # second moments about a global shift s (the images' mean): variances and the covariance are shift-invariant, and
    # E[(x - s)^2] - (mx - s)^2 cancels far fewer float64 digits on a bright flat image than E[x^2] - mx^2
    s = 0.5 * (x.mean() + y.mean())
    xs, ys = x - s, y - s
    mxs, mys = mx - s, my - s
    vx = _filter_valid(xs * xs, w) - mxs * mxs
    vy = _filter_valid(ys * ys, w) - mys * mys
    cxy = _filter_valid(xs * ys, w) - mxs * mys
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim(x, y):
    return float(ssim_map(x, y).mean())


def ssim_direct(x, y):
    """the same mean by a direct 2-D window loop with central moments (sum w (x - mx)^2): the definition, slowly"""
    x, y, w = np.asarray(x, np.float64), np.asarray(y, np.float64), window()
    w2 = np.outer(w, w)[:, :, None]
    H, W = x.shape[:2]
    total = 0.0
    for i in range(H - WIN + 1):
        for j in range(W - WIN + 1):
            px, py = x[i:i + WIN, j:j + WIN], y[i:i + WIN, j:j + WIN]
            mx, my = (w2 * px).sum((0, 1)), (w2 * py).sum((0, 1))
            dx, dy = px - mx, py - my
            vx, vy, cxy = (w2 * dx * dx).sum((0, 1)), (w2 * dy * dy).sum((0, 1)), (w2 * dx * dy).sum((0, 1))
            total += (((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))).sum()
    return total / (3.0 * (H - WIN + 1) * (W - WIN + 1))


def mse_psnr(pred, target):
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    mse = float((d * d).mean())
    return mse, float(10.0 * np.log10(1.0 / max(mse, 1e-12)))


def record(pred, images, image, background=None, with_ssim=True, clamp=False):
    """(mse, psnr, ssim) of pred (float32 [H, W, 3] or [H*W, 3]) against frame `image`; ssim is NaN without with_ssim"""
    t = target_f32(images, image, background)
    p = np.asarray(pred, np.float32).reshape(t.shape)
    if clamp:
        p = np.clip(p, np.float32(0.0), np.float32(1.0))
    mse, psnr = mse_psnr(p, t)
    return mse, psnr, (ssim(p, t) if with_ssim else float("nan"))
