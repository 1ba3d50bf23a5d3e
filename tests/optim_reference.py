"""Float64 restatement of the optimizer update of csrc/optim.hip: clip_grad_norm_ folded into one AdamW step.
numpy only, no torch, no project imports: it is what tests/test_gpu_optim_edges.py holds the kernels against and
what tests/test_optim_reference_host.py holds against torch.optim.AdamW.  Not a test module.

Every hyper-parameter is taken at its float32 value and widened (the kernels receive floats, so 1 - beta is exact
here as it is there); tensors are widened from the fp32 inputs.

Non-finite norm, as adamw_state_k and step_meter_k (csrc/meter.hip) compute it with c = max_norm / (norm *
grad_scale + 1e-6) and coef = grad_scale * (c < 1 ? c : 1):
    sumsq = inf  ->  c = 0, the coefficient is 0 (moments decay, no gradient enters);
    sumsq = NaN  ->  c = NaN, `c < 1` is false, the coefficient stays at grad_scale (the step is NOT clipped).
torch.nn.utils.clip_grad_norm_ multiplies every gradient by the NaN coefficient instead; the training runner stops
on the meter's flag before such a step matters."""
import numpy as np

U = 2.0 ** -24            # unit of the bounds: half an fp32 ulp of 1
FLOOR = 2.0 ** -126       # smallest normal fp32: a result flushed to zero stays within it


def w32(x):
    """x at its float32 value, as float64."""
    return np.float64(np.float32(x))


def wide(a):
    """fp32 inputs widened; a float64 array passes through (a state carried over several reference steps)."""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.astype(np.float64)


def clip_coef(sumsq, grad_scale, max_norm):
    """What every gradient element is multiplied by: grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale +
    1e-6)); max_norm <= 0 switches clipping off (sumsq is then ignored).  sumsq is the fp64 sum of squares of the
    UNSCALED gradients."""
    gs, mx = w32(grad_scale), w32(max_norm)
    if not mx > 0.0:
        return gs
    s = np.float64(sumsq)
    if np.isnan(s):
        return gs                                   # rule: `c < 1` is false for NaN
    if np.isinf(s):
        return gs * 0.0                             # rule: c = max_norm / inf = 0
    c = mx / (np.sqrt(s) * gs + w32(1e-6))
    return gs * (c if c < 1.0 else 1.0)


def adamw_step(p, g, m, v, coef, t, lr, lr_factor, weight_decay, beta1, beta2, eps):
    """Step number t (>= 1) of torch.optim.AdamW on gradients g * coef.  Returns p', m', v' and the scales Sp, Sm,
    Sv of the bounds |got - ref| <= C * 2^-24 * S + 2^-126: sums of the absolute values of what each result is
    added up from, so none of them shrinks when the terms cancel (Sp is built on Sm, not on |m'|)."""
    p, g, m, v = wide(p), wide(g), wide(m), wide(v)
    coef = np.float64(coef)
    b1, b2, eps = w32(beta1), w32(beta2), w32(eps)
    lr = w32(lr) * w32(lr_factor)
    t = np.float64(t)
    bc1 = 1.0 - np.power(b1, t)
    bc2_sqrt = np.sqrt(1.0 - np.power(b2, t))
    gc = g * coef
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + (1.0 - b2) * gc * gc
    denom = np.sqrt(v1) / bc2_sqrt + eps
    p1 = p * (1.0 - lr * w32(weight_decay)) - (lr / bc1) * (m1 / denom)
    Sm = np.abs(b1 * m) + np.abs((1.0 - b1) * gc)
    Sv = b2 * v + (1.0 - b2) * gc * gc
    Sp = np.abs(p) + (lr / bc1) * Sm / denom
    return p1, m1, v1, Sp, Sm, Sv


def error_ratio(got, ref, S):
    """max over elements of (|got - ref| - 2^-126) / (2^-24 * S), 0 where the difference is within the floor; inf
    for a non-finite result or a miss on an element whose scale is 0."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    S = np.asarray(S, np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        excess = np.abs(got - ref) - FLOOR
        r = np.where(excess <= 0.0, 0.0, excess / (U * S))
    r = np.where(np.isfinite(got), r, np.inf)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())
