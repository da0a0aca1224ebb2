"""The per-epoch evaluation's exact reference: pg_loc_correction restated in numpy float32 in
the order the kernel's header comment documents (csrc/loc_eval.hip: column min and max, the
normalised row summed sequentially in column order, a float32 alpha, fmaxf / fminf over the
row), which the kernel must match bit for bit; and the margin rule under which that
restatement is compared with the reference's own function (oracle.protein_loc_correction,
torch-CPU float32, whose vectorised row sum may associate differently, so that a normalised
score can differ in its last bits).

Margin rule: an entry is compared with the oracle when its float64 margin |v - th| exceeds
8 u rmax (u = 2^-24: the two divisions, a row sum that differs by association, the
threshold's subtraction and product, with room). Entries that sit AT the threshold by
construction are left to the exact restatement and not counted as left out: at alpha = 0 the threshold is the
row maximum itself and at alpha = 1 it is rmax - (rmax - rmin), the row minimum up to
rounding, so one entry per row has margin 0 whatever the seed (every entry when C = 1); rows
holding a NaN (a constant column, n = 1: 0 / 0) predict 0 in both. Of the remaining entries
at most 1e-3 may be left out.

Those threshold entries are where the column-order row sum shows: at alpha = 1 the
restatement (and the kernel) differs from torch-CPU's vectorised sum on the row-minimum entry
of 415 of 4 097 rows at C = 10 and 235 of 2 048 at C = 12 (the last bit of rmax - (rmax -
rmin) decides `rmin > th`); at alpha = 0 and 0.2 no entry of any case here differs."""
import numpy as np

U = 2.0 ** -24
f32 = np.float32

# (C, n, alpha, seed): a sample of C in {1, 3, 10, 12, 33, 64} x n in {1, 255, 257, 2048,
# 2049, 4097} x alpha in {0, 0.2, 1}. n = 255: below one 256-row part; 2048 / 2049 / 4097:
# loc_perf_sum_kernel's chunk boundaries; C != 12: the generic kernel.
CASES = [
    (1, 257, 0.2, 1), (1, 2049, 1.0, 2), (3, 1, 0.0, 3), (3, 255, 1.0, 4), (3, 2049, 0.2, 5),
    (10, 257, 0.0, 6), (10, 2048, 0.2, 7), (10, 4097, 1.0, 8), (12, 255, 0.2, 9), (12, 2048, 1.0, 10),
    (12, 4097, 0.0, 11), (33, 1, 1.0, 12), (33, 2049, 0.2, 13), (64, 257, 1.0, 14), (64, 2048, 0.0, 15),
    (64, 4097, 0.2, 16),
]


def make_proba(C, n, seed, const_col=None):
    rng = np.random.default_rng(seed)
    p = rng.random((n, C)).astype(f32)
    if const_col is not None:
        p[:, const_col] = f32(0.25)          # max == min: 0 / 0 down the whole column
    return p


def make_true(C, n, seed):
    rng = np.random.default_rng(1000 + seed)
    t = (rng.random((n, C)) < 0.2).astype(f32)
    t[t.sum(1) == 0, C // 2] = 1.0           # every row labelled (the special rows are added by the test)
    return t


def loc_correction_f32(p, alpha):
    """pg_loc_correction's float32 operations in its order; pred as float64 0 / 1."""
    p = np.asarray(p, f32)
    n, C = p.shape
    mn, mx = p.min(0), p.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (p - mn) / (mx - mn)
        s = np.zeros(n, f32)
        for c in range(C):
            s = s + v[:, c]
        v = v / s[:, None]
        rmax = np.fmax.reduce(v, axis=1, initial=f32(-np.inf))     # fmaxf: a NaN operand is skipped
        rmin = np.fmin.reduce(v, axis=1, initial=f32(np.inf))
        th = rmax - (rmax - rmin) * f32(alpha)
        return (v > th[:, None]).astype(np.float64)


def comparable(p, alpha):
    """(mask of the entries compared with the oracle, share left out): see the module
    docstring."""
    p = np.asarray(p, f32).astype(np.float64)
    n, C = p.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (p - p.min(0)) / (p.max(0) - p.min(0))
        v = v / v.sum(1, keepdims=True)
        rmax, rmin = v.max(1, keepdims=True), v.min(1, keepdims=True)
        th = rmax - (rmax - rmin) * float(f32(alpha))
        nanrow = np.isnan(v).any(1, keepdims=True)
        wide = np.abs(v - th) > 8 * U * rmax
    at_th = np.zeros_like(wide)
    if alpha == 0.0:
        at_th = v == rmax
    elif alpha == 1.0:
        at_th = v == rmin
    at_th = at_th | (rmax == rmin)
    counted = ~nanrow & ~at_th
    left = counted & ~wide
    share = left.sum() / max(int(counted.sum()), 1)
    return wide | nanrow, float(share)
