"""The Adam update of include/colvo.h (a8) in float64, and how far a float32 evaluation of it may lie from that.

Nothing here touches a GPU: tests/test_adam_ref_cpu.py holds this file to torch.optim.Adam in float64 and to a float32 emulation
of the kernel's arithmetic; tests/test_adam_exact_gpu.py holds csrc/adam.hip's k_adam, k_adam_multi and k_adam_pack to it.

adam_step_f64  the operation the kernel is asked to do: float64 arithmetic on the float32 state and on the float32-ROUNDED
               hyperparameters that the C ABI carries (float lr, beta1, beta2, eps, grad_scale).
adam_bounds    per-element bounds on |float32 result - adam_step_f64| that hold for every evaluation order, with or without
               fused multiply-add.  Derived below from the operation count, never from what a kernel returned.
adam_emulate_f32  the kernel's arithmetic in NumPy float32, plain operation order (the bounds' self-check).
operand_copies what the forward / transposed operand copies must hold given a parameter arena.
"""
import numpy as np

U = 2.0 ** -24            # unit round-off of float32: one rounding to nearest moves a normal result by at most U, relatively
TINY = 2.0 ** -126        # smallest normal float32: the absolute allowance for a kernel that flushes subnormal results to zero


def _f32(x) -> float:
    return float(np.float32(x))


def _gamma(k: float) -> float:
    """k roundings in a row: (1 + U)^k - 1 <= k U / (1 - k U) (Higham's gamma_k) -- the first-order k U made rigorous."""
    return k * U / (1.0 - k * U)


def bias_corrections(t, b1, b2):
    """(1 - b1^t, 1 - b2^t) in float64 without cancellation."""
    t = float(t)
    return -np.expm1(t * np.log(b1)), -np.expm1(t * np.log(b2))


def adam_step_f64(p, g, m, v, t, lr, b1, b2, eps, gscale, f32_hyper=True):
    """One Adam step (torch.optim.Adam semantics, no weight decay) in float64.

        gi = g gscale;  m' = b1 m + (1 - b1) gi;  v' = b2 v + (1 - b2) gi^2
        p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

    f32_hyper: lr, b1, b2, eps and gscale are rounded to float32 first, as the C ABI does (False: taken as the doubles they are --
    torch's semantics, used only to measure the distance between the two).  t is the 1-based step number.
    -> dict(p, m, v: the new state; gi, a = b1 m, b = (1 - b1) gi, upd = p - p', den, ss = lr / (1 - b1^t), rs = 1 / sqrt(1 - b2^t))."""
    if f32_hyper:
        lr, b1, b2, eps, gscale = (_f32(x) for x in (lr, b1, b2, eps, gscale))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    gi = g * gscale
    a, b = b1 * m, (1.0 - b1) * gi
    m1 = a + b
    v1 = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = bias_corrections(t, b1, b2)
    ss, rs = lr / bc1, 1.0 / np.sqrt(bc2)
    den = np.sqrt(v1) * rs + eps
    upd = ss * (m1 / den)
    return dict(p=p - upd, m=m1, v=v1, gi=gi, a=a, b=b, upd=upd, den=den, ss=ss, rs=rs)


# relative allowances of the update m' / den * ss, in units of U (see adam_bounds)
UPD_OWN_U = 7.5
COEF_U = 22.5


def coef_allowance_pow(t, b1, b2):
    """The coefficient allowance, in units of U and in place of COEF_U, for a kernel that computes the bias corrections as
    1 - powf(b, t) -- what csrc/adam.hip's adam_coef does.  pow is held to the OpenCL limit of 16 ulp; 1 - b^t is an exact
    subtraction (Sterbenz, b^t >= 1/2) or absorbs it, so a relative error e of b^t becomes e b^t / (1 - b^t) of the correction:
    16 U b^t / (1 - b^t) per coefficient.  Plus the three roundings behind the corrections (lr / bc1; sqrt and 1 / of bc2), 3 U,
    which that figure does not count and which are all that is left once b^t has vanished.  At t = 1, b2 = 0.999 this is
    16 000 U = 9.5e-4 of the step: the early step sizes are only that well specified by this form."""
    bc1, bc2 = bias_corrections(t, _f32(b1), _f32(b2))
    return 16.0 * ((1.0 - bc1) / bc1 + (1.0 - bc2) / bc2) + 3.0


def adam_bounds(ref, coef_u=COEF_U):
    """Per-element bounds (bp, bm, bv, bu) on |float32 kernel - ref| for ref = adam_step_f64(...) of float32 state.

    Every float32 operation (+, *, /, sqrt: correctly rounded) multiplies its exact result by (1 + d), |d| <= U; k of them in a row
    by at most 1 + gamma_k, gamma_k = k U / (1 - k U).  A fused multiply-add only removes roundings.

    bm = gamma_3 (|b1 m| + |(1 - b1) gi|) + TINY.   gi = fl(g gscale) is one rounding; (1 - b1) is EXACT in float32 for b1 in
        [0.5, 1] (Sterbenz); (1 - b1) gi a second rounding, the sum a third, which also acts on b1 m (itself one rounding, two in
        all).  Three on the worse term, for either association.  (The issue's constant; re-derived: the same.)
    bv = gamma_5 v' + TINY.   gi^2 carries gi's rounding twice, its two products two more, the sum a fifth; b2 v two.  Every term
        is non-negative, so 5 on the sum.  (The same.)
    bu = |upd| (UPD_OWN_U + coef_u) U + ss bm / den + |upd| (sqrt(v') rs / den) bv / (2 v').
        The second term is m's error carried through the quotient, the third is v's through the square root (half its relative
        error) weighted by the share of sqrt(v') rs in the denominator.
        UPD_OWN_U: sqrt, x rs, + eps, /, x step_size are five roundings, 5 U.  The issue allows 7.5 U, counting v's half share
        (2.5 U) here as well as in the third term; the larger figure is kept, as the issue asks.
        coef_u: the two coefficients step_size = lr / bc1 and rs = 1 / sqrt(bc2), bc = -expm1(t log b).  log and expm1 are held
        to the OpenCL limit of 3 ulp each; an ulp is up to 2 U relative (just above a power of two), so 6 U each -- the issue
        counted an ulp as U and arrived at 12.5 U.  x = t log(b): 6 U + the product's U = 7 U, which expm1 passes on with the
        factor |x| e^x / (1 - e^x) <= 1; expm1's own 6 U: bc is good to 13 U.  step_size: + the division, 14 U.  rs: half of 13 U
        + sqrt + division, 8.5 U.  Together 22.5 U, the larger figure, kept.  ((float)t is exact below 2^24.)  A kernel that
        computes the corrections as 1 - powf(b, t) is given coef_allowance_pow(t, b1, b2) instead.
    bp = U (|p'| + bu) + bu: the final subtraction rounds a difference that is at most |p'| + bu in magnitude.
    TINY is added only where the quantity has a non-zero term: a sum of exact zeros is exactly zero in any arithmetic, so an
    element with g = m = v = 0 has bm = bv = bu = 0 and must come back bit-equal.  (Second-order terms: gamma_k covers them for
    m and v; in bu they are below 1e-6 of the bound.)"""
    absab = np.abs(ref["a"]) + np.abs(ref["b"])
    bm = _gamma(3) * absab + np.where(absab > 0, TINY, 0.0)
    v1 = ref["v"]
    bv = _gamma(5) * v1 + np.where(v1 > 0, TINY, 0.0)
    aupd = np.abs(ref["upd"])
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(v1 > 0, np.sqrt(v1) * ref["rs"] / ref["den"] * bv / (2.0 * v1), 0.0)
        bu = aupd * (UPD_OWN_U + coef_u) * U + ref["ss"] * bm / ref["den"] + aupd * share
    bu = np.where(absab > 0, bu + TINY, 0.0)
    bp = U * (np.abs(ref["p"]) + bu) + bu
    return bp, bm, bv, bu


def adam_emulate_f32(p, g, m, v, t, lr, b1, b2, eps, gscale, coef="expm1"):
    """adam_one of csrc/adam.hip in NumPy float32, plain operation order, no fused multiply-add.  coef: 'expm1' -- the
    coefficients as -expm1f(t logf(b)); 'pow' -- as 1 - powf(b, t), the cancelling form.  -> (p', m', v', upd) float32."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, gscale, one, tf = f(lr), f(b1), f(b2), f(eps), f(gscale), f(1), f(t)
    if coef == "expm1":
        bc1, bc2 = f(-np.expm1(f(tf * np.log(b1)))), f(-np.expm1(f(tf * np.log(b2))))
    elif coef == "pow":
        bc1, bc2 = f(one - np.power(b1, tf)), f(one - np.power(b2, tf))
    else:
        raise ValueError(coef)
    ss, rs = f(lr / bc1), f(one / np.sqrt(bc2))
    gi = g * gscale
    m1 = b1 * m + (one - b1) * gi
    v1 = b2 * v + (one - b2) * gi * gi
    upd = ss * (m1 / (np.sqrt(v1) * rs + eps))
    p1 = p - upd
    assert all(x.dtype == f for x in (m1, v1, upd, p1))
    return p1, m1, v1, upd


def worst_ratios(got, ref, bounds):
    """{quantity: (worst |got - ref| / bound, its index)} for got = dict(p, m, v[, upd]) of float32 arrays; an element whose bound
    is zero counts 0 when bit-equal to the (float32-representable) reference and inf otherwise."""
    bp, bm, bv, bu = bounds
    out = {}
    for key, bound in (("p", bp), ("m", bm), ("v", bv), ("upd", bu)):
        if key not in got:
            continue
        x = np.asarray(got[key])
        assert x.dtype == np.float32, (key, x.dtype)
        err = np.abs(x.astype(np.float64) - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        # a zero bound also pins the sign of a zero
        same_bits = x.view(np.uint32) == ref[key].astype(np.float32).view(np.uint32)
        r = np.where((bound == 0) & ~same_bits, np.inf, r)
        assert not np.isnan(r).any(), key
        i = int(np.argmax(r)) if r.size else 0
        out[key] = (float(r[i]) if r.size else 0.0, i)
    return out


def make_state(n, seed, p_zero=False, g_lo=1e-8, g_hi=1e3):
    """float32 (p, g, m, v) of n elements: g, m = normal x 10^U(-8, 3), |g| clamped to [g_lo, g_hi]; v = |normal| x 10^U(-16, 6);
    p normal (or all zero).  Everything normal and finite."""
    rng = np.random.default_rng(seed)
    f = np.float32
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)
    g = (np.where(g < 0, -1.0, 1.0) * np.clip(np.abs(g), g_lo, g_hi)).astype(f)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)).astype(f)
    v = (np.abs(rng.standard_normal(n)) * 10.0 ** rng.uniform(-16, 6, n)).astype(f)
    v = np.maximum(v, f(1e-30))
    p = np.zeros(n, f) if p_zero else rng.standard_normal(n).astype(f)
    return p, g, m, v


# float32(0.9) = 15099494 / 2^24 and 1 - float32(0.9) = 1677722 / 2^24: m = 838861 s and gi = -7549747 s make b1 m + (1 - b1) gi
# vanish EXACTLY (both integers fit 24 bits; the products fit a double)
CANCEL_M, CANCEL_G = 838861.0, -7549747.0


def plant_specials(p, g, m, v, gscale=1.0):
    """Overwrite the first elements (as many as fit) with the special cases, in place; -> how many were planted.
      0  g = m = v = 0, p = 1.5      (p, m, v must come back bit-unchanged)
      1  g = m = v = 0, p = -0.0
      2  p = +0, 3  p = -0           (ordinary g, m, v)
      4  m and gi cancelling exactly for beta1 = float32(0.9) when g gscale is exact (gscale a power of two), nearly otherwise
      5  |g| = 1e-8,  6  |g| = 1e3   (the ends of the gradient range)"""
    f = np.float32
    rows = [
        (1.5, 0.0, 0.0, 0.0), (-0.0, 0.0, 0.0, 0.0),
        (0.0, 0.37, -0.011, 2.5e-4), (-0.0, -3.0e-3, 4.0e-4, 1.0e-7),
        (0.25, CANCEL_G * 2.0 ** -20 / gscale, CANCEL_M * 2.0 ** -20, 0.5),
        (-0.7, 1e-8, 2.0e-9, 1.0e-16), (0.9, -1e3, 40.0, 3.0e5),
    ]
    k = min(len(rows), len(p))
    for i in range(k):
        p[i], g[i], m[i], v[i] = (f(x) for x in rows[i])
    return k


def operand_copies(p_new, layers, dtype):
    """What the operand buffers must hold for the parameter arena p_new (1-D float32 torch tensor on the CPU).
    layers: (w_off, Cout, Cin) of each 3x3 layer, weights [Cout][9][Cin] at element w_off.  dtype: torch.float32 or torch.bfloat16
    (torch's cast: round to nearest even).  -> [(fwd [Cout, 9, Cin], bwd [Cin, 9, Cout])]: fwd the cast, bwd the taps flipped and
    the channel axes exchanged, as in test_pack_weights_multi_matches_permute."""
    out = []
    for w_off, co, ci in layers:
        w = p_new[w_off:w_off + co * 9 * ci].view(co, 9, ci)
        out.append((w.to(dtype), w.flip(1).permute(2, 1, 0).contiguous().to(dtype)))
    return out
