"""The loss head at its entry points: pg_sigmoid_multi_loss (multi_loss_kernel),
pg_mlp_head (head_kernel<float | bf16>) and the head part of pg_mlp_l1_head
(mlp_l1_head_kernel), each against tests/head_common.py's float64 references and bars, called
through the C ABI with padded leading dimensions into sentinel-filled buffers.

The three kernels each carry their own copy of the loss math (sigmoid, the clamp to
[1e-9, 10], the clamp's zero gradient, sigmoid_backward); every case here holds logits on
both sides of both clamp edges (asserted: p32 < 1e-9, q32 == 0, and neither), rows of every
set, and, on the head cases, a ragged last block of 32 rows ((64, 128, 16) is the one case
of whole blocks at the largest K and C). Where n C is too small for 20 elements of each kind
((33, 1, 1) has 33 elements) the case asks for n C / 4 of each.

Largest error-to-bar ratios printed on an MI355X:
  pg_sigmoid_multi_loss   prob 0.51   dz 0.44   loss 0.06
  pg_mlp_head f32         prob 0.35   dz 0.38   dA4 0.42   loss2 0.11
  pg_mlp_head bf16        prob 0.25   dz 0.34   dA4 1.00   loss2 0.10
  pg_mlp_l1_head          prob 0.25   dz 0.43   dA4 0.30   loss2 0.02
(bf16 dA4 at 0.996: round to nearest even of an 8-bit significand errs by up to 2^-8 of the
value, which is the bf16 term of the bar; the float32 term keeps one rounding to spare.)

Tried against deliberately wrong kernels (scratch builds): `set == 1` -> `set != 0` in
head_kernel fails all ten pg_mlp_head cases; the clamp mask's edge moved (`pr >= 1e-9f` ->
`pr >= 1e-10f`, all three copies) fails 13 cases. `pr >= 1e-9f` -> `pr > 1e-9f` passes: the
two differ only at p32 == float32(1e-9) bit for bit (at p == 0 both mask, and dz carries the
factor p), which no float32 logit here reaches (neighbouring logits near -20.72 are 17 ulps
of p apart); tests/test_head_ref_cpu.py pins the reference itself at that edge.
"""
import numpy as np
import pytest
import torch

import head_common as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -768.0          # exact in bf16 too
SLOPE = 0.01


# ---- buffers ---------------------------------------------------------------------------
def _to_dev(a, ld, dtype=torch.float32):
    """a [rows][cols] as the leading columns of a sentinel-filled [rows][ld] device buffer."""
    a = np.asarray(a)
    buf = torch.full((a.shape[0], ld), SENT, dtype=dtype)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dtype)
    return buf.to(DEV)


def _out(rows, ld, dtype=torch.float32):
    return torch.full((rows, ld), SENT, dtype=dtype, device=DEV)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 1),), 255, dtype=torch.uint8, device=DEV)  # NaNs if read unwritten


def _np(buf, cols):
    """(the leading columns as float32 numpy; asserts the padding kept the sentinel)."""
    h = buf.detach().cpu()
    assert (h[:, cols:].float() == SENT).all(), "padding overwritten"
    return h[:, :cols].float().numpy()


def _bits(buf):
    h = buf.detach().cpu().contiguous()
    return h.view(torch.int16 if h.element_size() == 2 else torch.int32).numpy()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- pg_sigmoid_multi_loss -------------------------------------------------------------
def _multi_loss(z, t, cw, idx, want=("prob", "dz", "loss")):
    from plagnn import _lib

    n, C = z.shape
    zd, td = _to_dev(z, C + 1), _to_dev(t, C + 2)
    cwd = torch.from_numpy(cw).to(DEV)
    idd = torch.from_numpy(np.asarray(idx, np.int32)).to(DEV) if len(idx) else None
    o = {"prob": _out(n, C + 3) if "prob" in want else None,
         "dz": _out(n, C + 5) if "dz" in want else None,
         "loss": torch.full((2,), SENT, device=DEV) if "loss" in want else None}
    nws = _lib.lib().pg_sigmoid_multi_loss_workspace(len(idx), C)
    ws = _ws(nws)
    _lib.call("pg_sigmoid_multi_loss", zd.data_ptr(), C + 1, n, C, td.data_ptr(), C + 2, cwd.data_ptr(),
              _ptr(idd), len(idx), _ptr(o["prob"]), C + 3, _ptr(o["loss"]), _ptr(o["dz"]), C + 5,
              ws.data_ptr(), nws, _lib.stream_handle(zd.device))
    torch.cuda.synchronize()
    return o


def _ml_case(C, seed):
    rng = np.random.default_rng(seed)
    n = 300
    z = H.mixed_logits(rng, (n, C))
    t = (rng.random((n, C)) < 0.3).astype(np.float32)
    w = rng.uniform(0.5, 30.0, C)
    return rng, z, t, w


@pytest.mark.parametrize("C", [1, 3, 12, 16, 33, 64])
def test_sigmoid_multi_loss_against_float64(C):
    """prob on all rows, dz on the index rows (exactly 0 elsewhere) and the loss, on shuffled
    index subsets of R - 1, R, R + 1 and 173 rows (R = 256 // C rows per block; C = 33: 7
    rows and 231 live threads); each optional output NULL once; two calls bitwise equal."""
    rng, z, t, w = _ml_case(C, 200 + C)
    cw = H.class_weights(w)
    n = len(z)
    R = 256 // C
    s, sbar = H.sigmoid_ref(z)
    for ln in (R - 1, R, R + 1, 173):
        rows = rng.permutation(n)[:ln]
        o = _multi_loss(z, t, cw, rows)
        p32 = _np(o["prob"], C)
        H.check(f"C={C} len={ln} prob", p32, s, sbar)
        lr = H.loss_ref(p32, t, w, rows)
        H.coverage(lr["lowp"], lr["q0"])
        dz = _np(o["dz"], C)
        H.check_dz(f"C={C} len={ln} dz", dz[rows], lr)
        rest = np.setdiff1d(np.arange(n), rows)
        assert not dz[rest].any(), "dz outside the index rows"
        loss = o["loss"].cpu().numpy()
        assert loss[1] == SENT
        H.check(f"C={C} len={ln} loss", np.float64(loss[0]), np.float64(lr["loss"]), lr["loss_bar"])
    # the last subset again: bitwise, and with each optional output left out
    again = _multi_loss(z, t, cw, rows)
    for k in o:
        assert np.array_equal(_bits(o[k]), _bits(again[k])), f"{k}: two calls differ"
    for drop in ("prob", "dz", "loss"):
        part = _multi_loss(z, t, cw, rows, want=tuple(k for k in o if k != drop))
        for k in o:
            if k != drop:
                assert np.array_equal(_bits(o[k]), _bits(part[k])), f"{k} with {drop} = NULL"


@pytest.mark.parametrize("C", [12, 33])
def test_sigmoid_multi_loss_empty_index(C):
    """n_index = 0 (index may be NULL): prob and an all-zero dz are written for every row,
    loss[0] is left as it was (include/plagnn.h)."""
    _, z, t, w = _ml_case(C, 300 + C)
    o = _multi_loss(z, t, H.class_weights(w), [])
    s, sbar = H.sigmoid_ref(z)
    H.check(f"C={C} empty prob", _np(o["prob"], C), s, sbar)
    assert not _np(o["dz"], C).any()
    assert (o["loss"].cpu().numpy() == SENT).all()


# ---- pg_mlp_head -----------------------------------------------------------------------
B2 = (0.0, 30.0, -30.0, 18.0, -21.0)


def _row_set(rng, n, sets=(0, 1, 2)):
    rs = rng.choice(np.array(sets, np.int8), n, p=None if len(sets) != 3 else [0.25, 0.5, 0.25])
    rs[:len(sets)] = sets              # every set present
    return rng.permutation(rs).astype(np.int8)


def _head_inputs(n, K, C, seed, bf16):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((n, K)) + 0.25).astype(np.float32)      # ~40 % <= 0
    W2 = (rng.standard_normal((C, K)) * 3.0 / np.sqrt(1.0625 * K)).astype(np.float32)
    b2 = np.array([B2[c % len(B2)] for c in range(C)], np.float32)
    # scaled rows: a multiple of one W2 row, so that class r % C sits at +-30 (+ b2)
    plus, minus = ((1, 4), (3, 4)) if C < 3 else ((5, 16), (11, 16))
    for r in range(n):
        sg = 1.0 if r % plus[1] == plus[0] else -1.0 if r % minus[1] == minus[0] else 0.0
        if sg:
            wr = W2[r % C].astype(np.float64)
            A[r] = (sg * 30.0 * wr / (wr @ wr)).astype(np.float32)
    zero = rng.random((n, K)) < 0.02
    A[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0).astype(np.float32)   # y > 0 is false at +-0
    if bf16:
        A = torch.from_numpy(A).bfloat16().float().numpy()
    t = (rng.random((n, C)) < 0.3).astype(np.float32)
    w = rng.uniform(0.5, 30.0, C)
    return rng, A, W2, b2, t, w


def _mlp_head(A, W2, b2, t, cw, rs, bf16, want=("prob", "dz", "dz_bf16", "dA4")):
    from plagnn import _lib

    n, K = A.shape
    C = W2.shape[0]
    adt = torch.bfloat16 if bf16 else torch.float32
    Ad, Wd, td = _to_dev(A, K + 3, adt), _to_dev(W2, K + 1), _to_dev(t, C + 2)
    bd, cwd, rsd = (torch.from_numpy(x).to(DEV) for x in (b2, cw, rs))
    o = {"prob": _out(n, C + 3) if "prob" in want else None,
         "dz": _out(n, C + 5) if "dz" in want else None,
         "dz_bf16": _out(n, C + 5, torch.bfloat16) if "dz_bf16" in want else None,
         "dA4": _out(n, K + 2, adt) if "dA4" in want else None,
         "loss2": torch.full((3,), SENT, device=DEV)}
    nws = _lib.lib().pg_mlp_head_workspace(n, C)
    ws = _ws(nws)
    _lib.call("pg_mlp_head", Ad.data_ptr(), K + 3, n, K, _lib.PG_DTYPE_BF16 if bf16 else _lib.PG_DTYPE_F32,
              Wd.data_ptr(), K + 1, bd.data_ptr(), C, td.data_ptr(), C + 2, cwd.data_ptr(), rsd.data_ptr(),
              int((rs == 1).sum()), int((rs == 2).sum()), _ptr(o["prob"]), C + 3, _ptr(o["dz"]), C + 5,
              _ptr(o["dz_bf16"]), _ptr(o["dA4"]), K + 2, SLOPE, o["loss2"].data_ptr(), ws.data_ptr(), nws,
              _lib.stream_handle(Ad.device))
    torch.cuda.synchronize()
    return o


def _check_head(tag, o, A4, W2, b2, t, w, rs, bf16, C, K):
    """The head's outputs against the references, from the A4 it read: prob, then dz and
    both losses from the kernel's p32, dA4 from the kernel's dz. Returns p32."""
    n = len(A4)
    s, sbar = H.prob_ref(A4, W2, b2)
    p32 = _np(o["prob"], C)
    H.check(f"{tag} prob", p32, s, sbar)
    tr, va = np.flatnonzero(rs == 1), np.flatnonzero(rs == 2)
    lr = H.loss_ref(p32, t, w, tr)
    dz = _np(o["dz"], C)
    H.check_dz(f"{tag} dz", dz[tr], lr)
    assert not dz[rs != 1].any(), "dz outside the train rows"
    if o.get("dz_bf16") is not None:
        _np(o["dz_bf16"], C)
        want = torch.from_numpy(dz).bfloat16()            # round to nearest even
        assert np.array_equal(_bits(o["dz_bf16"][:, :C]), _bits(want)), "dz_bf16 != bf16(dz)"
    ref, bar = H.dA4_ref(dz, W2, A4, SLOPE, bf16)
    H.check(f"{tag} dA4", _np(o["dA4"], K), ref, bar)
    loss2 = o["loss2"].cpu().numpy()
    assert loss2[2] == SENT
    H.check(f"{tag} loss2[train]", np.float64(loss2[0]), np.float64(lr["loss"]), lr["loss_bar"])
    lv = H.loss_ref(p32, t, w, va)
    H.check(f"{tag} loss2[val]", np.float64(loss2[1]), np.float64(lv["loss"]), lv["loss_bar"])
    # the case holds what it is for
    all_rows = H.loss_ref(p32, t, w, np.arange(n), n=0)
    H.coverage(all_rows["lowp"], all_rows["q0"], need=min(20, n * C // 4))
    H.coverage(lr["lowp"], lr["q0"], need=min(20, n * C // 4) // 4)      # and on the train rows
    assert set(np.unique(rs)) == {0, 1, 2}
    return p32


# (n, K, C, ragged last block of 32 rows)
HEAD_CASES = [(97, 28, 3, True), (64, 128, 16, False), (33, 1, 1, True), (700, 100, 12, True), (31, 127, 5, True)]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,K,C,ragged", HEAD_CASES)
def test_mlp_head_against_float64(n, K, C, ragged, bf16):
    rng, A, W2, b2, t, w = _head_inputs(n, K, C, 400 + n + K, bf16)
    rs = _row_set(rng, n)
    cw = H.class_weights(w)
    assert (n % 32 != 0) == ragged
    share = (A <= 0).mean()
    assert 0.3 < share < 0.55, share                     # both leaky branches
    o = _mlp_head(A, W2, b2, t, cw, rs, bf16)
    _check_head(f"head {'bf16' if bf16 else 'f32'} ({n}, {K}, {C})", o, A, W2, b2, t, w, rs, bf16, C, K)
    # each optional output NULL once: the others bitwise unchanged
    for drop in ("prob", "dz", "dz_bf16", "dA4"):
        part = _mlp_head(A, W2, b2, t, cw, rs, bf16, want=tuple(k for k in o if k not in (drop, "loss2")))
        for k in o:
            if k != drop:
                assert np.array_equal(_bits(o[k]), _bits(part[k])), f"{k} with {drop} = NULL"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("sets", [(0, 2), (0, 1), (0,)], ids=["no-train", "no-val", "neither"])
def test_mlp_head_empty_sets(sets, bf16):
    """n_train = 0: loss2[0] is left as it was, dz and dA4 are 0 everywhere; n_val = 0:
    loss2[1] is left as it was (include/plagnn.h). The other slot is still right."""
    n, K, C = 97, 28, 3
    rng, A, W2, b2, t, w = _head_inputs(n, K, C, 500, bf16)
    rs = _row_set(rng, n, sets)
    o = _mlp_head(A, W2, b2, t, H.class_weights(w), rs, bf16)
    s, sbar = H.prob_ref(A, W2, b2)
    p32 = _np(o["prob"], C)
    H.check("empty-set prob", p32, s, sbar)
    loss2 = o["loss2"].cpu().numpy()
    for slot, sid in ((0, 1), (1, 2)):
        rows = np.flatnonzero(rs == sid)
        if len(rows) == 0:
            assert loss2[slot] == SENT
        else:
            lr = H.loss_ref(p32, t, w, rows)
            H.check(f"loss2[{slot}]", np.float64(loss2[slot]), np.float64(lr["loss"]), lr["loss_bar"])
    if 1 not in sets:
        assert not _np(o["dz"], C).any() and not _np(o["dA4"], K).any()
        assert not _np(o["dz_bf16"], C).any()
    else:
        lr = H.loss_ref(p32, t, w, np.flatnonzero(rs == 1))
        H.check_dz("no-val dz", _np(o["dz"], C)[rs == 1], lr)


# ---- pg_mlp_l1_head --------------------------------------------------------------------
def _l1_head(H3, W1, b1, W2, b2, t, cw, rs, want=("prob", "dz")):
    from plagnn import _lib

    n, F3 = H3.shape
    K1, C = W1.shape[0], W2.shape[0]
    ldw = (K1 + 3) // 4 * 4 + 4
    Hd, W1d, W2d, td = _to_dev(H3, F3 + 4), _to_dev(W1, F3 + 4), _to_dev(W2, ldw), _to_dev(t, C + 2)
    b1d, b2d, cwd, rsd = (torch.from_numpy(x).to(DEV) for x in (b1, b2, cw, rs))
    o = {"A4": _out(n, K1 + 3), "prob": _out(n, C + 3) if "prob" in want else None,
         "dz": _out(n, C + 5) if "dz" in want else None, "dA4": _out(n, K1 + 2), "dH3": _out(n, F3 + 1),
         "loss2": torch.full((3,), SENT, device=DEV)}
    nws = _lib.lib().pg_mlp_l1_head_workspace(n, C, F3, K1)
    ws = _ws(nws)
    _lib.call("pg_mlp_l1_head", Hd.data_ptr(), F3 + 4, n, F3, W1d.data_ptr(), F3 + 4, b1d.data_ptr(), K1,
              o["A4"].data_ptr(), K1 + 3, W2d.data_ptr(), ldw, b2d.data_ptr(), C, td.data_ptr(), C + 2,
              cwd.data_ptr(), rsd.data_ptr(), int((rs == 1).sum()), int((rs == 2).sum()), _ptr(o["prob"]), C + 3,
              _ptr(o["dz"]), C + 5, o["dA4"].data_ptr(), K1 + 2, o["dH3"].data_ptr(), F3 + 1, SLOPE,
              o["loss2"].data_ptr(), ws.data_ptr(), nws, None, 0.0, 0.0, 0.0, _lib.stream_handle(Hd.device))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("n,F3,K1,C", [(97, 60, 28, 3), (600, 200, 100, 12)])
def test_mlp_l1_head_against_float64(n, F3, K1, C):
    """The fused kernel's own copy of the head, from the A4 it wrote (A4 and dH3 themselves
    are pinned bitwise to the GEMMs by tests/test_gpu_mlp_head.py)."""
    rng = np.random.default_rng(600 + n)
    H3 = rng.standard_normal((n, F3)).astype(np.float32)
    H3[5::16] *= 15.0                                     # a few scaled rows
    H3[11::16] *= -15.0
    W1 = (rng.standard_normal((K1, F3)) / np.sqrt(F3)).astype(np.float32)
    b1 = (0.25 + 0.1 * rng.standard_normal(K1)).astype(np.float32)
    W2 = (rng.standard_normal((C, K1)) * 3.0 / np.sqrt(0.6 * K1)).astype(np.float32)
    b2 = np.array([B2[c % len(B2)] for c in range(C)], np.float32)
    t = (rng.random((n, C)) < 0.3).astype(np.float32)
    w = rng.uniform(0.5, 30.0, C)
    rs = _row_set(rng, n)
    cw = H.class_weights(w)
    assert n % 32 != 0
    o = _l1_head(H3, W1, b1, W2, b2, t, cw, rs)
    A4 = _np(o["A4"], K1)
    pre = H3.astype(np.float64) @ W1.astype(np.float64).T + b1
    A4ref = np.where(pre > 0, pre, pre * SLOPE)
    assert np.abs(A4 - A4ref).max() <= 1e-4 * np.abs(A4ref).max()       # the right operand at all
    share = (A4 <= 0).mean()
    assert 0.3 < share < 0.55, share
    _np(o["dH3"], F3)
    _check_head(f"l1 head ({n}, {F3}, {K1}, {C})", o, A4, W2, b2, t, w, rs, False, C, K1)
    for drop in ("prob", "dz"):
        part = _l1_head(H3, W1, b1, W2, b2, t, cw, rs, want=tuple(k for k in ("prob", "dz") if k != drop))
        for k in o:
            if k != drop:
                assert np.array_equal(_bits(o[k]), _bits(part[k])), f"{k} with {drop} = NULL"
