"""Two restatements of the Adam / AdamW step of csrc/adam.hip (rd_adam_prepare + rd_adam_step), and the measurement of the bars.

1. numpy float32, operation for operation (step_f32), with the float64 arithmetic of the state block (new_block, prepare): the launches
   must reproduce it bit for bit.  The block's layout is include/radar_depth_hip.h's.

       prepare (float64; skipped: only word 8 is written):
           t += 1;  b1t *= beta1;  b2t *= beta2
           s = f32(grad_scale) * f32(coef)           step_size = f32(lr / (1 - b1t))     bc2s = f32(sqrt(1 - b2t))
           decay = f32(1 - lr * wd)                  omb1 = f32(1 - beta1)               omb2 = f32(1 - beta2)
       step (float32, every operation rounded on its own):
           g = s * grad
           adam,  wd != 0:  g = g + wd * p           adamw, wd != 0:  p = p * decay
           m = m + omb1 * (g - m);   v = beta2 * v + (omb2 * g) * g;   d = sqrt(v) / bc2s + eps;   p = p - step_size * (m / d)

2. float64 (step_f64): the same formulas from the same fp32 state and the same fp32 scalars, every operation in float64, with the
   magnitudes entering each output's last operation:  |m0| + |g|,   |v0| + g^2,   |p0| + step_size |m| / d.  errors() divides the
   distance to it by those (normalising by the result alone means nothing where m cancels).

measure_bars(): one step of torch.optim.Adam and torch.optim.AdamW on the CPU in fp32 against (2): the reference's own error.  The bars
of the kernels are twice those (an equally valid order of operations)."""
import functools

import numpy as np

BLOCK_WORDS = 20
(W_LR, W_BETA1, W_BETA2, W_EPS, W_WD, W_T, W_B1T, W_B2T, W_SKIP, W_S, W_WDF, W_DECAY, W_OMB1, W_BETA2F, W_OMB2, W_BC2S, W_EPSF,
 W_STEP) = range(18)
MODES = {"adam": 0, "adamw": 1}
F = np.float32


def new_block(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, t=0):
    """a state at step t: the products by t multiplications, as a restored checkpoint forms them"""
    b = np.zeros(BLOCK_WORDS, dtype=np.float64)
    b[W_LR], b[W_BETA1], b[W_BETA2], b[W_EPS], b[W_WD] = lr, betas[0], betas[1], eps, weight_decay
    b[W_B1T] = b[W_B2T] = 1.0
    for _ in range(int(t)):
        b[W_T] += 1.0
        b[W_B1T] *= b[W_BETA1]
        b[W_B2T] *= b[W_BETA2]
    return b


def prepare(block, grad_scale=1.0, coef=1.0, skip=False):
    """rd_adam_prepare on the block, in place.  coef: the fp32 clip coefficient as a Python float (grad_clip_ref.clip_coef)."""
    block[W_SKIP] = 1.0 if skip else 0.0
    if skip:
        return block
    lr, b1, b2, eps, wd = (np.float64(block[i]) for i in (W_LR, W_BETA1, W_BETA2, W_EPS, W_WD))
    with np.errstate(all="ignore"):
        block[W_T] += 1.0
        block[W_B1T] *= b1
        block[W_B2T] *= b2
        block[W_S] = F(grad_scale) * F(coef)
        block[W_WDF] = F(wd)
        block[W_DECAY] = F(1.0 - lr * wd)
        block[W_OMB1] = F(1.0 - b1)
        block[W_BETA2F] = F(b2)
        block[W_OMB2] = F(1.0 - b2)
        block[W_BC2S] = F(np.sqrt(1.0 - block[W_B2T]))
        block[W_EPSF] = F(eps)
        block[W_STEP] = F(lr / (1.0 - block[W_B1T]))
    return block


def _scalars(block, dtype):
    return [dtype(block[i]) for i in (W_S, W_WDF, W_DECAY, W_OMB1, W_BETA2F, W_OMB2, W_BC2S, W_EPSF, W_STEP)]


def step_f32(p, grad, m, v, block, mode):
    """rd_adam_step: (p, m, v) as new float32 arrays"""
    assert mode in MODES
    p, grad, m, v = (np.array(a, dtype=F) for a in (p, grad, m, v))
    if block[W_SKIP] != 0.0:
        return p, m, v
    s, wd, decay, omb1, beta2, omb2, bc2s, eps, step = _scalars(block, F)
    with np.errstate(all="ignore"):
        g = s * grad
        if wd != 0:
            if mode == "adam":
                g = g + wd * p
            else:
                p = p * decay
        m = m + omb1 * (g - m)
        v = beta2 * v + (omb2 * g) * g
        d = np.sqrt(v) / bc2s + eps
        p = p - step * (m / d)
    assert p.dtype == F and m.dtype == F and v.dtype == F
    return p, m, v


def step_f64(p, grad, m, v, block, mode):
    """the same formulas in float64 from the same fp32 state: dict(p, m, v, the normalisers np_, nm, nv, and the intermediate g, d)"""
    assert mode in MODES
    p0, grad, m0, v0 = (np.asarray(a, dtype=F).astype(np.float64) for a in (p, grad, m, v))
    s, wd, decay, omb1, beta2, omb2, bc2s, eps, step = _scalars(block, np.float64)
    with np.errstate(all="ignore"):
        g = s * grad
        p = p0
        if wd != 0:
            if mode == "adam":
                g = g + wd * p
            else:
                p = p * decay
        m = m0 + omb1 * (g - m0)
        v = beta2 * v0 + (omb2 * g) * g
        d = np.sqrt(v) / bc2s + eps
        upd = step * (m / d)
        return dict(p=p - upd, m=m, v=v, nm=np.abs(m0) + np.abs(g), nv=np.abs(v0) + g * g, np_=np.abs(p0) + np.abs(upd), g=g, d=d)


def errors(got_p, got_m, got_v, ref):
    """worst normalised distances (p, m, v) of fp32 results to step_f64's; elements whose reference is not finite are left out"""
    out = []
    with np.errstate(all="ignore"):
        for got, key, norm in ((got_p, "p", "np_"), (got_m, "m", "nm"), (got_v, "v", "nv")):
            e = np.abs(np.asarray(got, dtype=np.float64) - ref[key]) / ref[norm]
            e = e[np.isfinite(ref[key]) & (ref[norm] > 0)]
            out.append(float(e.max()) if e.size else 0.0)
    return tuple(out)


def random_state(n, seed, t):
    """fp32 p, grad, m, v: gradient magnitudes log-uniform over 1e-6 .. 1e2, m and v of the gradients' scale, both signs"""
    r = np.random.RandomState(seed)
    sign = lambda: np.where(r.rand(n) < 0.5, -1.0, 1.0)      # noqa: E731
    mag = 10.0 ** r.uniform(-6.0, 2.0, n)
    grad = (sign() * mag).astype(F)
    p = (sign() * r.uniform(0.25, 2.0, n)).astype(F)
    m = (sign() * mag * r.uniform(0.05, 2.0, n)).astype(F)
    v = (mag * mag * r.uniform(0.05, 2.0, n)).astype(F)
    return p, grad, m, v


HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
BAR_CASES = [(mode, t, wd) for mode in ("adam", "adamw") for t in (0, 1000) for wd in (0.0, 1e-2)]


def torch_one_step(p, grad, m, v, mode, t, wd, lr=HP["lr"], betas=HP["betas"], eps=HP["eps"]):
    """one step of torch.optim.Adam / AdamW on the CPU in fp32 from the given state at step count t"""
    import torch
    tp = torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=F)))
    cls = torch.optim.Adam if mode == "adam" else torch.optim.AdamW
    opt = cls([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False, fused=False)
    opt.state[tp] = {"step": torch.tensor(float(t)), "exp_avg": torch.from_numpy(np.array(m, dtype=F)),
                     "exp_avg_sq": torch.from_numpy(np.array(v, dtype=F))}
    tp.grad = torch.from_numpy(np.array(grad, dtype=F))
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == t + 1
    return tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()


BAR_SAMPLES = 4194309


@functools.lru_cache(maxsize=None)
def measure_bars(n=BAR_SAMPLES):
    """(rows, worst): per case of BAR_CASES the errors (p, m, v) of torch's fp32 step and of the restatement against float64; worst =
    torch's worst (p, m, v) over the cases: the reference's own error.  A worst value is a maximum over a sample and grows with it (from
    2e4 to 4e6 elements: m from 0.77 to 0.96 x 2^-24), so every case takes as many elements as the largest kernel test evaluates; a
    maximum over fewer would hold the kernels to a bar the reference itself misses on the test's own sample.  About 14 s, once."""
    rows = []
    for k, (mode, t, wd) in enumerate(BAR_CASES):
        p, grad, m, v = random_state(n, 100 + k, t)
        blk = prepare(new_block(weight_decay=wd, t=t, **HP))
        ref = step_f64(p, grad, m, v, blk, mode)
        rows.append(((mode, t, wd), errors(*torch_one_step(p, grad, m, v, mode, t, wd), ref), errors(*step_f32(p, grad, m, v, blk, mode), ref)))
    worst = tuple(max(r[1][i] for r in rows) for i in range(3))
    return rows, worst


def bars():
    """the kernels' bars (p, m, v): twice the reference's own fp32 error"""
    return tuple(2.0 * w for w in measure_bars()[1])
