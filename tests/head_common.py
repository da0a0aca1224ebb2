"""float64 references and error bars for the loss head: pg_sigmoid_multi_loss, pg_mlp_head
and the head part of pg_mlp_l1_head (include/plagnn.h; code/model.py:28-29 and code/train.py:
89-108 of the reference).

Plain numpy float64. Each reference is computed from the kernel's inputs, or, where said,
from the kernel's own EARLIER output (the float32 probabilities, dz, A4), so that every bar
covers one short chain of float32 roundings and nothing that cancels: the loss math is
checked from p32 (the clamp masks are then decided exactly, without a band around the
clamp's edges), dA4 from dz32.

u = 2^-24 is float32's unit roundoff, TINY = 2^-126 its smallest normal number (an absolute
term for results that underflow; at z = -100 float32's exp overflows and p = 0, the float64
sigmoid being 4e-44).

Bars (each a count of float32 roundings of relative size u, first order):

  sigmoid       |p - s| <= 4 u s + TINY          expf within 1 ulp (2 u), the add, the
                                                 divide, one to spare.
  logits        dZ = (K + 2) u (sum_k |a w| + |b|)    K fused multiply-adds, the bias add,
                                                 one to spare.
  head's prob   4 u s + s (1 - s) dZ + TINY      the sigmoid's slope times the logit's error.
  dz            |dz - ref| <= 8 u mag + TINY,    mag = (|ga| + |gb|) q p. The roundings:
                                                 1/n, /w1, *w, /clip(p) on ga's side (4; *2
                                                 and *t are exact, t being 0 or 1), or 1/n,
                                                 /w1, /clip(q) on gb's side (3); the add; the
                                                 products by q and by p (2; exact only where
                                                 q or p is a power of two): 7 on the longer
                                                 side, and one to spare.
                dz == 0 exactly wherever ref == 0 (both branches masked or multiplied by an
                exact 0; p32 and q32 are held exactly, so no band).
  loss          |loss - ref| <= (n_s + C + 6) u sum|term| / n_s    six per term: logf within
                                                 1 ulp (2 u), *w, the add, /w1 (*t and *2 are
                                                 exact) and the final division by n_s; then
                                                 float32 sums whose chains are no longer than
                                                 n_s rows plus C classes.
  dA4           (C + 2) u sum_c |dz w| * |leaky'| + TINY    C fused multiply-adds, the
                                                 product by the slope, one to spare; a bf16
                                                 dA4 adds 2^-8 |ref| (the suite's bf16 bar).
                                                 The leaky mask is A4 > 0, exactly.

Every check prints its largest error-to-bar ratio."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
LO = float(np.float32(1e-9))   # the clamp's lower edge as the kernels hold it
SAT = np.array([30.0, -30.0, 100.0, -100.0, 17.0, -20.8], np.float32)  # saturated logits


def mixed_logits(rng, shape, frac=0.5):
    """N(0, 3) logits with a share `frac` replaced by the saturated values: at z >= 17.4 the
    float32 1 - p is exactly 0 (17 leaves 2^-24), below -20.73 p < 1e-9 (-20.8: 9.2e-10;
    -100: p = 0, exp overflows)."""
    z = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    pick = rng.random(shape) < frac
    z[pick] = SAT[rng.integers(0, len(SAT), int(pick.sum()))]
    return z


def class_weights(w64):
    """class_w of include/plagnn.h: [2c] = (float)w_c, [2c + 1] = (float)(w_c + 1)."""
    w64 = np.asarray(w64, np.float64)
    cw = np.empty(2 * len(w64), np.float32)
    cw[0::2] = w64.astype(np.float32)
    cw[1::2] = (w64 + 1.0).astype(np.float32)
    return cw


def sigmoid_ref(z32):
    """(s, bar): the float64 sigmoid of the float32 logits."""
    z = np.asarray(z32, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
    return s, 4 * U * s + TINY


def logits_ref(A, W2, b2):
    """(z, dZ): float64 A W2^T + b2 of the float32 inputs (bf16 ones widened by the caller)."""
    A = np.asarray(A, np.float32).astype(np.float64)
    W = np.asarray(W2, np.float32).astype(np.float64)
    b = np.asarray(b2, np.float32).astype(np.float64)
    K = A.shape[1]
    return A @ W.T + b, (K + 2) * U * (np.abs(A) @ np.abs(W).T + np.abs(b))


def prob_ref(A, W2, b2):
    """(s, bar) of the head's prob = sigmoid(A W2^T + b2)."""
    z, dZ = logits_ref(A, W2, b2)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
    return s, 4 * U * s + s * (1.0 - s) * dZ + TINY


def loss_ref(p32, t, w64, rows, n=None):
    """multi_loss over the rows `rows` of the float32 probabilities p32 [N][C] (labels t
    [N][C] of 0 / 1, float64 class weights w64 [C]); n = the divisor (len(rows) by default).
    Returns a dict over the selected rows, in `rows` order: loss, loss_bar, dz, mag (dz's bar
    is 8 U mag + TINY), and the masks lowp (p32 < 1e-9), q0 (q32 == 0)."""
    p32 = np.asarray(p32, np.float32)[rows]
    t = np.asarray(t, np.float64)[rows]
    n = len(rows) if n is None else n
    C = p32.shape[1]
    q32 = np.float32(1) - p32                      # the kernel's 1.f - pr: one IEEE subtraction
    cw = class_weights(w64).astype(np.float64)
    w, w1 = cw[0::2], cw[1::2]
    p, q = p32.astype(np.float64), q32.astype(np.float64)
    cp, cq = np.clip(p, LO, 10.0), np.clip(q, LO, 10.0)
    term = ((t * np.log(cp)) * w + (1.0 - t) * np.log(cq)) / w1 * 2.0
    out = {"lowp": p32 < np.float32(1e-9), "q0": q32 == 0}
    if n > 0:
        out["loss"] = -term.sum() / n
        out["loss_bar"] = (n + C + 6) * U * np.abs(term).sum() / n
        g = -(1.0 / n) * 2.0 / w1
        ga = np.where((p >= LO) & (p <= 10.0), g * w * t / cp, 0.0)
        gb = np.where((q >= LO) & (q <= 10.0), g * (1.0 - t) / cq, 0.0)
        out["dz"] = (ga - gb) * q * p
        out["mag"] = (np.abs(ga) + np.abs(gb)) * q * p
    return out


def dA4_ref(dz32, W2, A4, slope, bf16=False):
    """(ref, bar): (dz W2) * leaky'(A4) from the kernel's own float32 dz; the float32 slope."""
    dz = np.asarray(dz32, np.float32).astype(np.float64)
    W = np.asarray(W2, np.float32).astype(np.float64)
    C = W.shape[0]
    f = np.where(np.asarray(A4, np.float32) > 0, 1.0, float(np.float32(slope)))
    ref = (dz @ W) * f
    bar = (C + 2) * U * (np.abs(dz) @ np.abs(W)) * np.abs(f) + TINY
    if bf16:
        bar = bar + 2.0 ** -8 * np.abs(ref)
    return ref, bar


def check(name, got, ref, bar):
    """max |got - ref| / bar, printed; asserts it is <= 1 (and that nothing is NaN)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    bar = np.broadcast_to(np.asarray(bar, np.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    ratio = float((np.abs(got - ref) / bar).max()) if got.size else 0.0
    print(f"{name}: max err / bar = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: err / bar = {ratio:.3f}"
    return ratio


def check_dz(name, dz32, lr):
    """dz against loss_ref's result: inside 8 U mag + TINY, and exactly 0 where the
    reference is 0."""
    dz32 = np.asarray(dz32, np.float32)
    zero = lr["dz"] == 0
    assert (dz32[zero] == 0).all(), f"{name}: non-zero dz where the reference is exactly 0"
    print(f"{name}: {int(zero.sum())} exact zeros")
    return check(name, dz32, lr["dz"], 8 * U * lr["mag"] + TINY)


def coverage(lowp, q0, need=20):
    """The case holds what it is for: `need` elements each below the clamp (p32 < 1e-9), with
    q32 == 0, and with neither."""
    counts = (int(lowp.sum()), int(q0.sum()), int((~lowp & ~q0).sum()))
    assert min(counts) >= need, f"coverage (p < 1e-9, q == 0, neither) = {counts}, need {need}"
    return counts
