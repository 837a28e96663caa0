"""No GPU, no HIP: the plain C++ part of coivo_amd/csrc/gauss_newton.h -- the damped Cholesky solve and the closed-form rotation that
k_refine_solve and k_register_solve run on one thread -- compiled with g++ (tests/cpp/gn_solve.cpp) and held to the NumPy replicas:
`solve_damped` bit for bit against tests/refine_ref.py `solve` and tests/register_ref.py's use of `cholesky_solve`, refusals included
(only + - * / sqrt are involved, so equality is the condition, not a tolerance); `rot_exp` against `se3_exp`, bit for bit where no
library function is called and within a bound derived from the operation count elsewhere."""
import os
import subprocess

import numpy as np
import pytest

from tests import refine_ref as R
from tests import register_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gn_solve.cpp")
U = 2.0 ** -53                                   # one rounding, relative; one ulp of a library function is 2 U


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gn") / "gn_solve"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _floats(line):
    return np.array([float.fromhex(t) for t in line.split()])


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- solve_damped --------------------------------------------------------------------------------------------------------------- #
DAMPINGS = (1e-6, 0.0, 1e-9)


def _systems():
    """200 seeded systems J^T J, J^T r of a 40 x 8 Gaussian J with column scales 10^U(-3, 3); every 17th with a zero column."""
    rng = np.random.default_rng(20)
    out = []
    for i in range(200):
        J = rng.standard_normal((40, 8)) * 10.0 ** rng.uniform(-3, 3, 8)
        if i % 17 == 0:
            J[:, int(rng.integers(0, 6))] = 0.0
        r = rng.standard_normal(40)
        out.append((J.T @ J, J.T @ r, DAMPINGS[i % 3]))
    return out


def _sums(Hm, g, LD):
    return np.array([Hm[k, l] for k in range(LD) for l in range(k, LD)] + list(g[:LD]))


def _register_solve(sums, n, damping):
    """tests/register_ref.py `step` up to its solution: the same four lines."""
    Hm = G.normal_matrix(sums)[:n, :n].copy()
    for k in range(n):
        Hm[k, k] = Hm[k, k] + damping * Hm[k, k]
    return R.cholesky_solve(Hm, sums[28:28 + n])


@pytest.mark.parametrize("LD,n", [(8, 6), (8, 8), (7, 6), (7, 7)])
def test_solve_damped_equals_the_replica_bit_for_bit(harness, LD, n):
    systems = _systems()
    sums = [_sums(Hm, g, LD) for Hm, g, _ in systems]
    got = harness([f"solve {LD} {n} {float(d).hex()} {_hex(s)}" for s, (_, _, d) in zip(sums, systems)])
    refused = mismatches = 0
    for line, s, (_, _, d) in zip(got, sums, systems):
        want = R.solve(s, n, d) if LD == 8 else _register_solve(s, n, d)
        if want is None:
            refused += 1
            mismatches += line != "refused"
        else:
            mismatches += line == "refused" or not _same_bits(_floats(line), want)
    print(f"LD {LD} n {n}: {len(systems)} systems, {refused} refused by the replica, {mismatches} mismatches")
    assert mismatches == 0
    assert refused == 12                             # the zero columns, all among the first six


def test_solve_damped_refuses_a_pivot_that_is_not_a_number(harness):
    Hm, g, _ = _systems()[1]
    s = _sums(Hm, g, 8)
    s[0] = np.nan
    assert R.solve(s, 6, 0.0) is None
    assert harness([f"solve 8 6 {0.0.hex()} {_hex(s)}"]) == ["refused"]


# ---- rot_exp -------------------------------------------------------------------------------------------------------------------- #
def _omegas():
    """|omega| from 1e-9 to 1.5 (below pi / 2: the condition numbers in _bounds hold), both sides of |omega|^2 = 1e-8, and vectors with
    zero components."""
    rng = np.random.default_rng(21)
    out = [np.zeros(3), np.array([1e-5, 0.0, 0.0]), np.array([0.0, -0.3, 0.0]), np.array([0.0, 0.0, 1.5])]
    for _ in range(300):
        w = rng.standard_normal(3)
        out.append(w / np.linalg.norm(w) * min(10.0 ** rng.uniform(-9, 0.3), 1.5))
    for norm in (0.99e-4, 1.01e-4):
        w = rng.standard_normal(3)
        out.append(w / np.linalg.norm(w) * norm)
    return out


def _replica(w):
    """Rx and V of tests/refine_ref.py se3_exp: V's columns are the translations of the three unit upsilons (products with 1 and 0)."""
    Rx = R.se3_exp(np.concatenate([np.zeros(3), w]))[:3, :3]
    V = np.stack([R.se3_exp(np.concatenate([np.eye(3)[k], w]))[:3, 3] for k in range(3)], axis=1)
    return Rx, V


def _bounds(w):
    """What either implementation may be off the exact value of its own formula, per entry of Rx and V, for |omega|^2 >= 1e-8; two
    implementations differ by at most twice that.  th2 is the same bits on both sides (+ and * only).  Allowed: one ulp (2 U) for each
    of sqrt, sin and cos, U per arithmetic operation.
      th = sqrt(th2)                         2 U relative
      ca = sin(th) / th                      sin of the perturbed th: |th cot th| <= 1 below pi / 2, so 2 U; its own ulp 2 U; the
                                             divisor 2 U; the division U: 7 U
      cb = (1 - cos(th)) / th2               cos absolute: 2 U |cos| + 2 U th |sin|; the subtraction U (1 - cos); relative to 1 - cos,
                                             plus the division U
      cc = (th - sin(th)) / (th2 th)         numerator absolute: d/dth (th - sin th) = 1 - cos, so 2 U th (1 - cos); sin's ulp
                                             2 U |sin|; the subtraction U (th - sin th); relative to th - sin th; the divisor
                                             2 U + U, the division U
      W2 = (a + b) + c                       its products U each, its additions U each: 3 U relative (all terms of one sign or zero)
      entry = (id + c1 Wm) + c2 W2           |c1 Wm| (e1 + U) + U |id + c1 Wm| + |c2 W2| (e2 + 3 U + U) + U |entry|"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    s, c = np.sin(th), np.cos(th)
    e_ca = 7 * U
    e_cb = (2 * U * abs(c) + 2 * U * th * abs(s) + U * (1 - c)) / (1 - c) + U
    e_cc = (2 * U * th * (1 - c) + 2 * U * abs(s) + U * (th - s)) / (th - s) + 4 * U
    ca, cb, cc = s / th, (1 - c) / th2, (th - s) / (th2 * th)
    Wm = np.abs(np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]))
    W2 = Wm @ Wm                                   # |W^2| entry by entry: each is a sum of terms of one sign
    I = np.eye(3)

    def entry(c1, e1, c2, e2):
        return c1 * Wm * (e1 + U) + U * (I + c1 * Wm) + c2 * W2 * (e2 + 4 * U) + U * (I + c1 * Wm + c2 * W2)
    return entry(ca, e_ca, cb, e_cb), entry(cb, e_cb, cc, e_cc)


def test_rot_exp_equals_the_replica(harness):
    ws = _omegas()
    got = [_floats(l) for l in harness([f"rot {_hex(w)}" for w in ws])]
    exact = bounded = 0
    worst = 0.0
    for w, g in zip(ws, got):
        Rx, V, R1 = g[:9].reshape(3, 3), g[9:18].reshape(3, 3), g[18:].reshape(3, 3)
        assert _same_bits(Rx, R1), w                 # asking for V does not change Rx
        want_R, want_V = _replica(w)
        if (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2] < 1e-8:           # the series: + - * / only
            exact += 1
            assert _same_bits(Rx, want_R) and _same_bits(V, want_V), w
            continue
        bounded += 1
        bR, bV = _bounds(w)
        for a, b, bound in ((Rx, want_R, bR), (V, want_V, bV)):
            err = np.abs(a - b)
            assert (err <= 2 * bound).all(), (w, float(err.max()), float(bound.min()))
            worst = max(worst, float((err[bound > 0] / (2 * bound[bound > 0])).max()))      # (a zero entry of an axis' rotation: 0 of 0)
    print(f"rot_exp: {exact} vectors bit for bit, {bounded} within the derived bound, worst error / bound {worst:.3f}")
    assert exact > 100 and bounded > 100


def test_header_switches_contraction_off_itself(tmp_path):
    """Compiled with fused multiply-add available and contraction asked for, the harness holds no fused instruction: the header does
    not rely on its includer's flags."""
    out = tmp_path / "gn_solve.s"
    subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=fast", "-S", SRC, "-o", str(out)], check=True)
    asm = out.read_text()
    assert "solve_damped" in asm and "vfm" not in asm and "vfnm" not in asm
