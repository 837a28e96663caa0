"""tests/adam_ref.py checks itself: the float64 reference is torch.optim.Adam, its distance from torch's double-hyperparameter
semantics is the derived one, a float32 evaluation in plain operation order stays inside every bound, and the cancelling
1 - powf(b, t) form of the bias corrections does not.  No GPU, no library call."""
import numpy as np
import pytest
import torch

from tests import adam_ref as R

KW = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
T_SWEEP = (1, 2, 3, 5, 10, 100, 1000, 10 ** 4, 10 ** 5)


def test_spec_hyperparameters_are_the_ones_used_here():
    from oracle import colvo_spec as S
    assert S.ADAM_KW == dict(lr=KW["lr"], betas=(KW["b1"], KW["b2"]), eps=KW["eps"], weight_decay=0.0)


def test_reference_with_double_hyperparameters_is_torch_adam_in_float64():
    from oracle import colvo_spec as S
    rng = np.random.default_rng(3)
    n = 1000
    p = rng.standard_normal(n)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], **S.ADAM_KW)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** (t - 3)
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        r = R.adam_step_f64(p, g, m, v, t, gscale=1.0, f32_hyper=False, **KW)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[pt]
        # relative to the size of what is summed: m' is a sum of two terms of either sign, which torch adds in another order
        # (lerp), so where they cancel the two float64 results differ by roundings of the TERMS, not of the small sum
        for got, want, scale in ((p, pt.detach().numpy(), np.abs(p)), (m, st["exp_avg"].numpy(), np.abs(r["a"]) + np.abs(r["b"])),
                                 (v, st["exp_avg_sq"].numpy(), v)):
            rel = np.max(np.abs(got - want) / np.maximum(scale, 1e-300))
            assert rel < 1e-14, (t, rel)


def test_distance_between_float_and_double_hyperparameters_is_the_derived_one():
    """float32(0.999) is off by 1.29e-8, which is 1.29e-5 = 216 U of 1 - b2: of 1 - b2^t at small t, and of the (1 - b2) gi^2
    term of v' at every t.  Either moves the step by half of that, 108 U = 6.4e-6 (where both act they pull in opposite
    directions: at t = 1 with v = 0 they cancel); float32(0.9) is off by 2.4e-7 of 1 - b1, lr and eps by less than U.  Below
    1e-5 relative in the update at every t -- relative to the update's magnitude ss (|b1 m| + |(1 - b1) gi|) / den: where the two
    terms of m' cancel, |upd| itself is no scale (the 2.4e-7 of one TERM is then anything of the sum)."""
    assert abs(float(np.float32(0.999)) - 0.999) == pytest.approx(1.29e-8, rel=0.01)
    p, g, m, v = R.make_state(20000, seed=5)
    worst = {}
    for t in T_SWEEP:
        a = R.adam_step_f64(p, g, m, v, t, gscale=1.0, **KW)
        b = R.adam_step_f64(p, g, m, v, t, gscale=1.0, f32_hyper=False, **KW)
        scale = b["ss"] * (np.abs(b["a"]) + np.abs(b["b"])) / b["den"]
        worst[t] = float(np.max(np.abs(a["upd"] - b["upd"]) / scale))
    print("relative distance of the update, float32 vs double hyperparameters:", {t: f"{w:.3e}" for t, w in worst.items()})
    assert max(worst.values()) < 1e-5, worst
    assert max(worst.values()) > 3e-6, worst            # (it IS the 108 U effect, not nothing)


def _ratios(coef, t, gscale, p_zero, seed, n=200_000):
    p, g, m, v = R.make_state(n, seed, p_zero=p_zero)
    R.plant_specials(p, g, m, v, gscale)
    if p_zero:
        p[:] = 0
    ref = R.adam_step_f64(p, g, m, v, t, gscale=gscale, **KW)
    p1, m1, v1, upd = R.adam_emulate_f32(p, g, m, v, t, gscale=gscale, coef=coef, **KW)
    return R.worst_ratios(dict(p=p1, m=m1, v=v1, upd=upd), ref, R.adam_bounds(ref))


@pytest.mark.parametrize("p_zero", [False, True])
def test_float32_emulation_stays_inside_every_bound(p_zero):
    worst = dict(p=0.0, m=0.0, v=0.0, upd=0.0)
    for t in (1, 2, 7, 1000, 100000):
        for gscale in (1.0, 0.125, 1.0 / 3.0):
            r = _ratios("expm1", t, gscale, p_zero, seed=1000 * t % 9973 + int(gscale * 64))
            for k in worst:
                worst[k] = max(worst[k], r[k][0])
    print(f"float32 emulation, p {'zero' if p_zero else 'normal'}: worst ratios", {k: f"{x:.3f}" for k, x in worst.items()})
    assert all(x <= 1.0 for x in worst.values()), worst
    assert worst["m"] > 0.3 and worst["v"] > 0.3, worst        # (the bounds are the right size, not vacuous)


def test_the_cancelling_pow_form_of_the_coefficients_exceeds_the_update_bound():
    r = _ratios("pow", 2, 1.0, True, seed=11)
    print("powf-form coefficients at t = 2, p = 0:", {k: f"{x[0]:.3f}" for k, x in r.items()})
    assert r["m"][0] <= 1.0 and r["v"][0] <= 1.0
    assert r["upd"][0] > 1.0 and r["p"][0] > 1.0, r


def test_the_pow_form_stays_inside_the_bound_that_carries_pow_through_the_cancellation():
    """What tests/test_adam_exact_gpu.py holds the kernels to: coef_allowance_pow in place of the fixed coefficient allowance."""
    worst = 0.0
    for t in (1, 2, 3, 5, 7, 1000, 100000):
        p, g, m, v = R.make_state(50_000, seed=70 + t % 13, p_zero=True)
        ref = R.adam_step_f64(p, g, m, v, t, gscale=0.125, **KW)
        p1, m1, v1, upd = R.adam_emulate_f32(p, g, m, v, t, gscale=0.125, coef="pow", **KW)
        r = R.worst_ratios(dict(p=p1, m=m1, v=v1, upd=upd), ref, R.adam_bounds(ref, coef_u=R.coef_allowance_pow(t, KW["b1"], KW["b2"])))
        worst = max(worst, max(x[0] for x in r.values()))
    assert worst <= 1.0, worst
    assert R.coef_allowance_pow(2, KW["b1"], KW["b2"]) == pytest.approx(16 * (0.81 / 0.19 + 0.998 / 0.002) + 3, rel=1e-2)
    assert R.coef_allowance_pow(10 ** 5, KW["b1"], KW["b2"]) == pytest.approx(3.0, abs=1e-9)


def test_zero_bounds_pin_the_bits():
    p, g, m, v = (np.array(x, np.float32) for x in ([1.5, -0.0], [0, 0], [0, 0], [0, 0]))
    ref = R.adam_step_f64(p, g, m, v, 3, gscale=0.125, **KW)
    bp, bm, bv, bu = R.adam_bounds(ref)
    assert not bm.any() and not bv.any() and not bu.any() and bp[1] == 0
    same = R.worst_ratios(dict(p=p.copy(), m=m.copy(), v=v.copy()), ref, (bp, bm, bv, bu))
    assert same["m"][0] == 0 and same["v"][0] == 0 and same["p"][0] == 0
    flipped = R.worst_ratios(dict(p=np.array([1.5, 0.0], np.float32), m=m, v=v), ref, (bp, bm, bv, bu))
    assert flipped["p"][0] == np.inf                    # +0 where -0 is due


def test_operand_copies_layout():
    co, ci = 3, 2
    w = torch.arange(64 + co * 9 * ci, dtype=torch.float32)
    (fwd, bwd), = R.operand_copies(w, [(64, co, ci)], torch.bfloat16)
    assert fwd.dtype == torch.bfloat16 and fwd.shape == (co, 9, ci) and bwd.shape == (ci, 9, co)
    m = w[64:].view(co, 9, ci)
    for o in range(co):
        for k in range(9):
            for c in range(ci):
                assert bwd[c, 8 - k, o] == m[o, k, c].to(torch.bfloat16) == fwd[o, k, c]
