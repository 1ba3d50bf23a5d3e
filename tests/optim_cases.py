"""Inputs of the optimizer-kernel edge tests (tests/test_gpu_optim_edges.py), a numpy float32 transcription of the
kernels' expression order, and the constants of the bounds.  Not a test module; numpy only.

The bounds: |got - ref64| <= C * 2^-24 * S + 2^-126 per element of p', m', v', with the scales Sp, Sm, Sv of
tests/optim_reference.py.  Each C is the smallest power of two at or above TWICE the worst ratio of the float32
transcription below against the reference, measured on the CPU over sweep() (tests/test_optim_reference_host.py
re-measures it in every run); the factor covers a differently rounded clip coefficient / bias correction and a
division or square root that is not correctly rounded.  The kernels are built with -ffp-contract=off, so their
expression order is the transcription's.
#              fp32 transcription (CPU)   kernels (MI355X)
C_P = 16.0     # 6.07                     7.05
C_M = 8.0      # 3.61                     3.95
C_V = 16.0     # 6.31                     6.92
"""
import numpy as np

import optim_reference as ref

C_P = 16.0
C_M = 8.0
C_V = 16.0

f32 = np.float32
BETA1, BETA2, EPS = f32(0.9), f32(0.999), f32(1e-8)
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]      # finite, negative, not a value any update makes

T_VALUES = (0, 1, 9, 99_999, 2 ** 31 + 5)        # completed steps BEFORE the launch (the state's t)
LR_FACTORS = (1.0, 0.1)
GRAD_SCALES = (1.0, 0.5, 0.125)


def adamw_inputs(n, seed, fresh=False):
    """p, g, m, v (fp32) for n elements.  Element i belongs to class i % 7 (7 is odd: every class meets every
    lane of a float4):
        0, 4, 6  ordinary          1  g == 0          2  p == 0
        3  m opposite in sign to g, of comparable size (m' cancels)          5  v == 0 with m != 0
    (v != 0 in classes 0 and 4: the lone element of n = 1 and the scalar tails of n = 5 and n = 1 048 577 can tell
    beta1 from beta2.)  |g| is log-uniform over 1e-6 .. 1e3 per element.  ``fresh``: m = v = 0 (the state before
    the first step)."""
    rng = np.random.default_rng(seed)
    cls = np.arange(n) % 7
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = (sign * 10.0 ** rng.uniform(-6.0, 3.0, n)).astype(f32)
    g[cls == 1] = 0.0
    p = rng.standard_normal(n).astype(f32)
    p[cls == 2] = 0.0
    if fresh:
        return p, g, np.zeros(n, f32), np.zeros(n, f32)
    mag = 10.0 ** rng.uniform(-6.0, 1.0, n)
    m = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * mag).astype(f32)
    opp = cls == 3
    # (1 - beta1) g coef against beta1 m: a ninth of g is where they cancel exactly at coef = 1
    m[opp] = (-g[opp].astype(np.float64) * rng.uniform(0.02, 0.5, int(opp.sum()))).astype(f32)
    v = ((np.abs(m.astype(np.float64)) * 10.0 ** rng.uniform(-1.0, 1.0, n)) ** 2).astype(f32)
    v[cls == 5] = 0.0
    assert np.all(m[cls == 5] != 0.0)
    return p, g, m, v


def kernel_fp32(p, g, m, v, sumsq, t, lr, lr_factor, weight_decay, max_norm, grad_scale,
                beta1=BETA1, beta2=BETA2, eps=EPS):
    """adamw_state_k, term by term, in numpy float32 (t: the step being taken, >= 1)."""
    one = f32(1.0)
    b1, b2, eps = f32(beta1), f32(beta2), f32(eps)
    coef = f32(grad_scale)
    if f32(max_norm) > 0:
        with np.errstate(invalid="ignore", over="ignore"):
            norm = f32(np.sqrt(np.float64(sumsq)))
            c = f32(max_norm) / f32(norm * f32(grad_scale) + f32(1e-6))
        coef = f32(coef * (c if c < one else one))
    lr_ = f32(f32(lr) * f32(lr_factor))
    decay = f32(one - f32(lr_ * f32(weight_decay)))
    step = f32(lr_ / f32(1.0 - np.power(np.float64(b1), np.float64(t))))
    bc2 = f32(np.sqrt(1.0 - np.power(np.float64(b2), np.float64(t))))
    gc = (g * coef).astype(f32)
    p1 = (p * decay).astype(f32)
    m1 = ((b1 * m).astype(f32) + ((one - b1) * gc).astype(f32)).astype(f32)
    v1 = ((b2 * v).astype(f32) + (((one - b2) * gc).astype(f32) * gc).astype(f32)).astype(f32)
    q = (m1 / ((np.sqrt(v1).astype(f32) / bc2).astype(f32) + eps).astype(f32)).astype(f32)
    p1 = (p1 - (step * q).astype(f32)).astype(f32)
    return p1, m1, v1


def step_ratios(got, before, sumsq, t, lr, lr_factor, weight_decay, max_norm, grad_scale, coef=None):
    """Worst error ratio of one step's (p', m', v') ``got`` against the fp64 reference started from ``before`` =
    (p, g, m, v), the fp32 state the step itself started from."""
    p, g, m, v = before
    if coef is None:
        coef = ref.clip_coef(sumsq, grad_scale, max_norm)
    p1, m1, v1, Sp, Sm, Sv = ref.adamw_step(p, g, m, v, coef, t, lr, lr_factor, weight_decay, BETA1, BETA2, EPS)
    return (ref.error_ratio(got[0], p1, Sp), ref.error_ratio(got[1], m1, Sm), ref.error_ratio(got[2], v1, Sv))


def sweep():
    """(name, kwargs of kernel_fp32 / step_ratios, (p, g, m, v)) over every device-state value the GPU tests use:
    each t, lr factor and grad scale, clipped (the gradients' own norm against max_norm = 10) and unclipped."""
    out = []
    seed = 0
    for t0 in T_VALUES:
        for lrf in LR_FACTORS:
            for gs in GRAD_SCALES:
                for clipped in (True, False):
                    for lr, wd in ((0.008, 0.01), (0.0004, 0.02)):
                        seed += 1
                        x = adamw_inputs(4099, seed, fresh=(t0 == 0))
                        sumsq = float((x[1].astype(np.float64) ** 2).sum()) if clipped else 4.0
                        kw = dict(sumsq=sumsq, t=t0 + 1, lr=lr, lr_factor=lrf, weight_decay=wd, max_norm=10.0,
                                  grad_scale=gs)
                        out.append(("t%d_f%g_s%g_%s_lr%g" % (t0, lrf, gs, "clip" if clipped else "free", lr), kw, x))
    return out
