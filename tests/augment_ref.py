"""Float64 numpy restatement of the augmentation contract (coivo_amd/data.py docstring), written from that text.

Frames are [n,h,w,3] uint8, `records` one per FRAME: anything with oy, ox, ch, cw (float32 values), flip, gamma and A [3,4]
(data.FrameAug; an AugRecord's .tgt / .ref).

One point of the contract is about number formats and is restated as such: the source coordinate is a FLOAT32 quantity,
fl32(step * (y + 0.5) + (oy - 0.5)) with step = fl32(ch/H) and a single rounding of the sum -- that is what makes the identity crop
today's kernel bit for bit.  Half an ulp of a coordinate near 300 is 1.5e-5 px, which on 8-bit noise (neighbours up to 1.0 apart)
is several times the project's 2e-6 resize tolerance; a reference with exact coordinates would measure that rounding and nothing
else.  `coords="float64"` gives the exact-coordinate variant, for the figures in DESIGN.md §3.6e.  Everything after the
coordinate -- weights, blend, /255, colour matrix, clamp, power -- is float64 here.
"""
import numpy as np


def _coords(origin, size, n_out, n_in, idx, coords):
    """Source coordinate of output indices `idx` along one axis, clamped to [0, n_in - 1], float64 values."""
    if coords == "float32":
        step = np.float64(np.float32(np.float64(size) / n_out))
        off = np.float64(np.float32(origin) - np.float32(0.5))
        # product of two float32 values: exact in float64; the sum is rounded to float64, then to float32 (the double rounding differs
        # from a true fused multiply-add only when the float64 sum falls within 2^-29 of a float32 tie)
        f = (step * (idx.astype(np.float64) + 0.5) + off).astype(np.float32).astype(np.float64)
    else:
        f = np.float64(origin) + (np.float64(size) / n_out) * (idx.astype(np.float64) + 0.5) - 0.5
    return np.clip(f, 0.0, n_in - 1.0)


def augment_frames(u8, records, H, W, coords="float32"):
    """-> [n,3,H,W] float64."""
    u8 = np.asarray(u8)
    n, h, w, _ = u8.shape
    assert len(records) == n
    out = np.empty((n, 3, H, W), dtype=np.float64)
    for i, r in enumerate(records):
        xs = np.arange(W)
        if int(r.flip):
            xs = W - 1 - xs
        fy = _coords(r.oy, r.ch, H, h, np.arange(H), coords)
        fx = _coords(r.ox, r.cw, W, w, xs, coords)
        y0 = np.floor(fy).astype(np.int64)
        x0 = np.floor(fx).astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        ly, lx = (fy - y0)[:, None, None], (fx - x0)[None, :, None]
        img = u8[i].astype(np.float64)
        top = (1.0 - lx) * img[y0][:, x0] + lx * img[y0][:, x1]
        bot = (1.0 - lx) * img[y1][:, x0] + lx * img[y1][:, x1]
        rgb = ((1.0 - ly) * top + ly * bot) / 255.0                         # [H,W,3]
        A = np.asarray(r.A, dtype=np.float64).reshape(3, 4)
        v = np.clip(rgb @ A[:, :3].T + A[:, 3], 0.0, 1.0)
        g = float(r.gamma)
        if g != 1.0:
            v = v ** g
        out[i] = v.transpose(2, 0, 1)
    return out


def augment_intrinsics(K, record, hw, HW):
    """K [3,3] at the native size hw -> K' (float64 numpy) of the cropped, resized, possibly mirrored frame: pixel centres on integers."""
    (H, W) = HW
    K = np.asarray(K, dtype=np.float64)
    sy, sx = H / np.float64(record.ch), W / np.float64(record.cw)
    K2 = K.copy()
    K2[0, 0] = K[0, 0] * sx
    K2[1, 1] = K[1, 1] * sy
    K2[0, 2] = (K[0, 2] + 0.5 - np.float64(record.ox)) * sx - 0.5
    K2[1, 2] = (K[1, 2] + 0.5 - np.float64(record.oy)) * sy - 0.5
    if int(record.flip):
        K2[0, 2] = W - 1 - K2[0, 2]
    return K2


def channel_bound(A):
    """Per-channel bar [3] of a colour-mapped, clamped pixel against this reference at gamma = 1: the project's resize tolerance 2e-6
    carried through the matrix row (|A_c[:3]|_1) plus four float32 roundings at the row's magnitude; the clamp is non-expansive."""
    A = np.abs(np.asarray(A, dtype=np.float64).reshape(3, 4))
    l1 = A[:, :3].sum(axis=1)
    return 2e-6 * l1 + 4 * 2.0 ** -24 * (l1 + A[:, 3])
