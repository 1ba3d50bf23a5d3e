"""tests/optim_reference.py (float64, numpy) against clip_grad_norm_ + torch.optim.AdamW on float64 parameters,
and the float32 transcription of the kernels' expression order (tests/optim_cases.py) against the reference: the
premise of the constants C_P / C_M / C_V that tests/test_gpu_optim_edges.py holds the kernels to.  No GPU."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_reference as ref

GROUPS = ((0.008, 0.01), (0.0004, 0.02))          # (lr, weight decay) as the fp32 numbers the kernels receive
MAX_NORM = 10.0


def _w(x):
    return float(np.float32(x))


@pytest.mark.parametrize("steps", [1, 2, 10])
def test_reference_matches_torch_adamw_in_float64(steps):
    """Two groups with their own lr and weight decay, clipped (odd steps: large gradients) and unclipped steps, the
    lr factor dropping to 0.1 in the middle: parameters AND both moments to 1e-12 relative."""
    sizes = (37, 11)
    rng = np.random.default_rng(steps)
    p = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    m = [np.zeros(n, np.float32) for n in sizes]
    v = [np.zeros(n, np.float32) for n in sizes]
    tp = [torch.from_numpy(x.astype(np.float64)).requires_grad_() for x in p]
    opt = torch.optim.AdamW([dict(params=[tp[i]], lr=_w(lr), weight_decay=_w(wd)) for i, (lr, wd) in enumerate(GROUPS)],
                            betas=(_w(oc.BETA1), _w(oc.BETA2)), eps=_w(oc.EPS))
    # the reference's own float64 state is carried across the steps
    state = [[x.astype(np.float64) for x in (p[i], m[i], v[i])] for i in range(2)]
    lrf = 1.0
    clipped_steps = 0
    for it in range(steps):
        if it == steps // 2 and steps > 1:
            lrf = _w(0.1)
            for grp, (lr, _) in zip(opt.param_groups, GROUPS):
                grp["lr"] = _w(lr) * lrf
        scale = 30.0 if it % 2 == 0 else 0.01
        g = [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]
        for i in range(2):
            tp[i].grad = torch.from_numpy(g[i].astype(np.float64))
        norm = torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
        opt.step()
        sumsq = sum(float((x.astype(np.float64) ** 2).sum()) for x in g)
        assert float(norm) == pytest.approx(np.sqrt(sumsq), rel=1e-14)
        coef = ref.clip_coef(sumsq, 1.0, MAX_NORM)
        clipped_steps += coef < 1.0
        assert (coef < 1.0) == (it % 2 == 0)
        for i, (lr, wd) in enumerate(GROUPS):
            p1, m1, v1, Sp, Sm, Sv = ref.adamw_step(state[i][0], g[i], state[i][1], state[i][2], coef, it + 1, lr, lrf, wd,
                                                    oc.BETA1, oc.BETA2, oc.EPS)
            assert np.all(Sp >= np.abs(p1) * (1 - 1e-12)) and np.all(Sm >= np.abs(m1)) and np.all(Sv == v1)
            state[i] = [p1, m1, v1]
    assert clipped_steps >= 1 and (steps == 1 or clipped_steps < steps)
    for i in range(2):
        st = opt.state[tp[i]]
        for name, got, want in (("p", state[i][0], tp[i].detach().numpy()), ("m", state[i][1], st["exp_avg"].numpy()),
                                ("v", state[i][2], st["exp_avg_sq"].numpy())):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg="group %d %s" % (i, name))
        assert float(st["step"]) == steps


def test_reference_takes_hyperparameters_at_their_float32_value():
    p, g, m, v = oc.adamw_inputs(64, 1)
    a = ref.adamw_step(p, g, m, v, 1.0, 3, 0.008, 0.1, 0.01, 0.9, 0.999, 1e-8)
    b = ref.adamw_step(p, g, m, v, 1.0, 3, _w(0.008), _w(0.1), _w(0.01), _w(0.9), _w(0.999), _w(1e-8))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_clip_coefficient_rules():
    assert ref.clip_coef(4.0, 1.0, 10.0) == 1.0                                  # norm 2 < 10
    assert ref.clip_coef(4.0, 0.5, 10.0) == 0.5
    assert ref.clip_coef(1e4, 1.0, 10.0) == pytest.approx(10.0 / (100.0 + _w(1e-6)), rel=1e-15)
    assert ref.clip_coef(1e4, 0.125, 10.0) == pytest.approx(0.125 * 10.0 / (12.5 + _w(1e-6)), rel=1e-15)
    assert ref.clip_coef(0.0, 0.5, 10.0) == 0.5
    assert ref.clip_coef(float("inf"), 0.5, 10.0) == 0.0                         # c = 0
    assert ref.clip_coef(float("nan"), 0.5, 10.0) == 0.5                         # `c < 1` false: not clipped
    for stale in (1e9, float("inf"), float("nan")):
        assert ref.clip_coef(stale, 0.5, 0.0) == 0.5                             # max_norm = 0: sumsq is ignored
    # torch, for the record: a NaN norm poisons every gradient
    x = torch.tensor([float("nan"), 1.0], dtype=torch.float64, requires_grad=True)
    x.grad = x.detach().clone()
    torch.nn.utils.clip_grad_norm_([x], 10.0)
    assert bool(torch.isnan(x.grad).all())


def test_case_generator_holds_what_the_gpu_tests_rely_on():
    for n in (7, 1025):
        p, g, m, v = oc.adamw_inputs(n, n)
        assert (g == 0).any() and (p == 0).any()
        assert ((m * g) < 0).sum() >= max(1, n // 7)
        assert ((v == 0) & (m != 0)).any()
    p, g, m, v = oc.adamw_inputs(100_000, 3)
    mag = np.abs(g[g != 0])
    assert mag.min() < 2e-6 and mag.max() > 5e2 and 0.1 < (g == 0).mean() < 0.2
    # cancelling moments: a bound built on |m'| instead of Sm would be orders of magnitude tighter there
    _, m1, _, _, Sm, _ = ref.adamw_step(p, g, m, v, 1.0, 10, 0.008, 1.0, 0.01, oc.BETA1, oc.BETA2, oc.EPS)
    assert (Sm[m1 != 0] / np.abs(m1[m1 != 0])).max() > 1e3
    p, g, m, v = oc.adamw_inputs(64, 1, fresh=True)
    assert not m.any() and not v.any()


def test_fp32_transcription_sets_the_constants():
    """What the kernels' own expression order costs in float32 on the CPU, in units of 2^-24 * S, over every
    device-state value of the GPU tests (oc.sweep: 120 draws of 4099 elements).  Each constant is the smallest
    power of two at or above twice this figure, so the transcription has to stay within half of each - and above
    a quarter, or the constant is looser than its rule."""
    worst = [0.0, 0.0, 0.0]
    where = [None, None, None]
    for name, kw, x in oc.sweep():
        r = oc.step_ratios(oc.kernel_fp32(*x, **kw), x, **kw)
        for i in range(3):
            if r[i] > worst[i]:
                worst[i], where[i] = r[i], name
    print("fp32 transcription, units of 2^-24 * S: p %.2f (%s)  m %.2f (%s)  v %.2f (%s)"
          % (worst[0], where[0], worst[1], where[1], worst[2], where[2]))
    for w, C in zip(worst, (oc.C_P, oc.C_M, oc.C_V)):
        assert C / 4 < w <= C / 2, (worst, where)


def test_bound_on_the_cancelling_moment_needs_Sm():
    """p = 0 and m opposite to g: |m'| nearly cancels, the fp32 result misses a bound built on |m'| by orders of
    magnitude and sits inside the one built on Sm."""
    n = 4096
    rng = np.random.default_rng(5)
    g = (10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    m = (-(g.astype(np.float64) / 9.0) * (1 + rng.uniform(-1e-6, 1e-6, n))).astype(np.float32)
    v = (m.astype(np.float64) ** 2).astype(np.float32)
    p = np.zeros(n, np.float32)
    kw = dict(sumsq=0.0, t=10, lr=0.008, lr_factor=1.0, weight_decay=0.01, max_norm=0.0, grad_scale=1.0)
    got = oc.kernel_fp32(p, g, m, v, **kw)
    rp, rm, rv = oc.step_ratios(got, (p, g, m, v), **kw)
    assert rp <= oc.C_P / 2 and rm <= oc.C_M / 2 and rv <= oc.C_V / 2
    p1, m1, v1, Sp, Sm, Sv = ref.adamw_step(p, g, m, v, 1.0, 10, 0.008, 1.0, 0.01, oc.BETA1, oc.BETA2, oc.EPS)
    naive = (_w(0.008) / (1 - _w(0.9) ** 10)) * np.abs(m1) / (np.sqrt(v1) / np.sqrt(1 - _w(0.999) ** 10) + _w(1e-8))
    assert ref.error_ratio(got[0], p1, naive) > 1e3
