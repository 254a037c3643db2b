"""numpy restatement of the clipped SGD step (csrc/loss_opt.hip: rd_grad_sumsq + rd_sgd_step_clip), in float64 on the fp32 inputs:

    S          = sum of g[i]^2 over every gradient                       (float64; the square of an fp32 value is exact there)
    total_norm = grad_scale * sqrt(S)
    coef       = float32(min(1, max_norm / (total_norm + 1e-6)))         (torch.clamp(max=1): a NaN stays a NaN); max_norm <= 0 or None: 1
    s          = float32(grad_scale) * coef                              (one fp32 product)
    d = wd * p + s * g;   buf = momentum * buf + d;   p = p - lr * buf   (float64, the hyper-parameters at their fp32 values)

which is torch.nn.utils.clip_grad_norm_(parameters, max_norm) followed by torch.optim.SGD's step on gradients that grad_scale
averages.  skip_nonfinite: a non-finite S leaves p and buf as they are.  Not the kernels' order of operations: the tests bound the
distance by counting fp32 roundings."""
import numpy as np


def _f32(v):
    return float(np.float32(v))


def sumsq(grads):
    """float64 sum of squares over a list of arrays (or one array)"""
    if isinstance(grads, np.ndarray):
        grads = [grads]
    return float(sum(np.square(np.asarray(g, dtype=np.float64)).sum() for g in grads))


def total_norm(grads, grad_scale=1.0):
    with np.errstate(invalid="ignore"):
        return _f32(grad_scale) * float(np.sqrt(sumsq(grads)))


def clip_coef(norm, max_norm):
    """the fp32 coefficient as a Python float"""
    if max_norm is None or not max_norm > 0.0:
        return 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.float64(max_norm) / (np.float64(norm) + 1e-6)
        return float(np.float32(1.0 if r > 1.0 else r))


def scale(grad_scale, coef):
    """s = grad_scale * coef in fp32"""
    with np.errstate(invalid="ignore"):
        return float(np.float32(grad_scale) * np.float32(coef))


def sgd_update(p, g, buf, lr, momentum, wd, s):
    """one tensor: returns (p, buf, d) in float64; s is the fp32 gradient scale as a Python float"""
    p, g, buf = (np.asarray(a, dtype=np.float64) for a in (p, g, buf))
    with np.errstate(invalid="ignore", over="ignore"):
        d = _f32(wd) * p + s * g
        buf = _f32(momentum) * buf + d
        p = p - _f32(lr) * buf
    return p, buf, d


def step(params, grads, bufs, lr, momentum, wd, grad_scale=1.0, max_norm=None, skip_nonfinite=False):
    """Lists of arrays in, (params, bufs, ds, stats) out; stats = dict(total_norm, clip_coef, skipped)."""
    norm = total_norm(grads, grad_scale)
    coef = clip_coef(norm, max_norm)
    skipped = bool(skip_nonfinite) and not np.isfinite(norm)
    stats = dict(total_norm=norm, clip_coef=coef, skipped=skipped)
    if skipped:
        f64 = lambda xs: [np.asarray(a, dtype=np.float64) for a in xs]      # noqa: E731
        return f64(params), f64(bufs), None, stats
    s = scale(grad_scale, coef)
    out = [sgd_update(p, g, b, lr, momentum, wd, s) for p, g, b in zip(params, grads, bufs)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], stats
