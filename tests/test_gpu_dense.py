"""The dense helpers of the training step at their entry points (csrc/dense.hip), through the
C ABI with padded leading dimensions into sentinel-filled buffers: pg_bias_act and
pg_act_bwd bitwise against the float32 numpy composition (one add, one select), pg_col_sum
against float64 under (rows + 2) u sum|x| (a chain of at most rows additions in whatever
order, two to spare; accumulate adds the rounding of out + s: u (|out| + sum|x|)),
pg_cast_bf16_f32 on all 65 536 bit patterns and the round trip with pg_cast_f32_bf16 against
torch, pg_adam_apply with weight decay and past one round of its 32768 x 256 grid against a
float64 restatement of include/plagnn.h's formula.

Largest error-to-bar ratios printed on an MI355X: col_sum 0.011 (accumulate 0.011);
Adam p 0.22 (rtol 1e-6, atol 1e-9), m 0.38, v 0.39."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -768.0
U = 2.0 ** -24
f32 = np.float32


def _to_dev(a, ld):
    a = np.asarray(a, f32)
    buf = torch.full((a.shape[0], ld), SENT, dtype=torch.float32)
    buf[:, :a.shape[1]] = torch.from_numpy(a)
    return buf.to(DEV)


def _back(buf, cols):
    h = buf.cpu()
    assert (h[:, cols:] == SENT).all(), "padding overwritten"
    return h[:, :cols].contiguous().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.int32), np.ascontiguousarray(b, f32).view(np.int32))


def _values(rng, rows, cols):
    """N(0, 1) with exact +0 and -0 sprinkled in."""
    x = rng.standard_normal((rows, cols)).astype(f32)
    k = rng.random((rows, cols))
    x[k < 0.05] = 0.0
    x[k > 0.95] = -0.0
    return x


def _act(v, act, slope):
    from plagnn import _lib

    if act == _lib.PG_ACT_RELU:
        return np.where(v > 0, v, f32(0))
    if act == _lib.PG_ACT_LEAKY:
        return np.where(v > 0, v, v * f32(slope))
    return v


@pytest.mark.parametrize("rows,cols", [(1, 1), (300, 40), (5, 2049)])
def test_bias_act_bitwise(rows, cols):
    from plagnn import _lib

    rng = np.random.default_rng(rows + cols)
    y = _values(rng, rows, cols)
    bias = rng.standard_normal(cols).astype(f32)
    bias[::7] = -y[0, ::7]                       # exact cancellation to +0 in the first row
    bd = torch.from_numpy(bias).to(DEV)
    for act in (_lib.PG_ACT_NONE, _lib.PG_ACT_RELU, _lib.PG_ACT_LEAKY):
        for b in (None, bias):
            yd = _to_dev(y, cols + 3)
            _lib.call("pg_bias_act", yd.data_ptr(), cols + 3, rows, cols, None if b is None else bd.data_ptr(),
                      act, 0.01, _lib.stream_handle(yd.device))
            torch.cuda.synchronize()
            ref = _act(y if b is None else y + b, act, 0.01)
            assert _same_bits(_back(yd, cols), ref), (act, b is not None)


def test_bias_act_empty_and_bad_act():
    from plagnn import _lib

    L = _lib.lib()
    yd = _to_dev(np.ones((4, 4), f32), 7)
    for rows, cols in ((0, 4), (4, 0), (0, 0)):
        assert L.pg_bias_act(yd.data_ptr(), 7, rows, cols, None, _lib.PG_ACT_RELU, 0.01, None) == 0
        assert L.pg_bias_act(None, 7, rows, cols, None, _lib.PG_ACT_RELU, 0.01, None) == 0
    for act in (-1, 3, 7):
        assert L.pg_bias_act(yd.data_ptr(), 7, 4, 4, None, act, 0.01, None) != 0
    assert L.pg_bias_act(yd.data_ptr(), 3, 4, 4, None, _lib.PG_ACT_RELU, 0.01, None) != 0     # ldy < cols
    torch.cuda.synchronize()
    assert (_back(yd, 4) == 1.0).all()


@pytest.mark.parametrize("rows,cols", [(1, 1), (300, 40), (5, 2049)])
def test_act_bwd_bitwise_padded(rows, cols):
    """relu and leaky from the activation OUTPUT y with lddy != ldy; at y = +0 and y = -0 the
    gradient takes the `y > 0` branch's other side (0, or dy * slope)."""
    from plagnn import _lib

    rng = np.random.default_rng(7 * rows + cols)
    y = _values(rng, rows, cols)
    dy = _values(rng, rows, cols)
    assert rows * cols < 10 or ((y == 0).any() and np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all())
    for act, other in ((_lib.PG_ACT_RELU, lambda g: np.zeros_like(g)), (_lib.PG_ACT_LEAKY, lambda g: g * f32(0.01)),
                       (_lib.PG_ACT_NONE, None)):
        yd, dyd = _to_dev(y, cols + 5), _to_dev(dy, cols + 3)
        _lib.call("pg_act_bwd", dyd.data_ptr(), cols + 3, yd.data_ptr(), cols + 5, rows, cols, act, 0.01,
                  _lib.stream_handle(yd.device))
        torch.cuda.synchronize()
        ref = dy if other is None else np.where(y > 0, dy, other(dy))
        assert _same_bits(_back(dyd, cols), ref), act
        assert _same_bits(_back(yd, cols), y)


@pytest.mark.parametrize("rows,cols", [(0, 5), (1, 1), (63, 65), (700, 100), (8193, 64)])
def test_col_sum_against_float64(rows, cols):
    from plagnn import _lib

    L = _lib.lib()
    rng = np.random.default_rng(rows + cols)
    x = rng.standard_normal((rows, cols)).astype(f32)
    xd = _to_dev(x, cols + 3) if rows else torch.full((1, cols + 3), SENT, device=DEV)
    out0 = rng.standard_normal(cols).astype(f32)
    nws = int(L.pg_col_sum_workspace(rows, cols))
    ref = x.astype(np.float64).sum(0)
    mag = np.abs(x.astype(np.float64)).sum(0)
    for acc in (0, 1):
        res = []
        for _ in range(2):
            ws = torch.full((nws,), 255, dtype=torch.uint8, device=DEV)
            od = _to_dev(out0[None, :], cols + 2)
            _lib.call("pg_col_sum", xd.data_ptr(), cols + 3, rows, cols, od.data_ptr(), acc, ws.data_ptr(), nws,
                      _lib.stream_handle(xd.device))
            torch.cuda.synchronize()
            res.append(_back(od, cols)[0])
        assert _same_bits(res[0], res[1]), "two calls differ"
        want = ref + (out0.astype(np.float64) if acc else 0.0)
        bar = (rows + 2) * U * mag + (U * (np.abs(out0) + mag) if acc else 0.0)
        err = np.abs(res[0].astype(np.float64) - want)
        if rows == 0:
            assert (err == 0).all()
        else:
            ratio = float((err / bar).max())
            print(f"col_sum ({rows}, {cols}) accumulate={acc}: max err / bar = {ratio:.3f}")
            assert ratio <= 1.0
    ws = torch.full((nws,), 255, dtype=torch.uint8, device=DEV)
    od = _to_dev(out0[None, :], cols + 2)
    assert L.pg_col_sum(xd.data_ptr(), cols + 3, rows, cols, od.data_ptr(), 0, ws.data_ptr(), nws - 1, None) != 0
    torch.cuda.synchronize()
    assert _same_bits(_back(od, cols)[0], out0)           # nothing was launched


def test_cast_bf16_f32_every_bit_pattern():
    from plagnn import _lib

    src = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    srcd = torch.from_numpy(src.view(np.int16)).to(DEV)
    dst = torch.full((65536 + 3,), SENT, device=DEV)
    _lib.call("pg_cast_bf16_f32", srcd.data_ptr(), 65536, dst.data_ptr(), _lib.stream_handle(srcd.device))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[65536:] == SENT).all()
    assert np.array_equal(got[:65536].view(np.uint32), src.astype(np.uint32) << 16)    # NaN patterns as bits


def test_cast_round_trip_equals_torch():
    """pg_cast_f32_bf16 then pg_cast_bf16_f32 == torch's float32 -> bfloat16 -> float32 (round
    to nearest even): halfway cases both ways, one bit either side of them, +-0, +-inf,
    float32 and bf16 denormals, the largest finite values (rounding up to inf)."""
    from plagnn import _lib

    rng = np.random.default_rng(0)
    hi = np.concatenate([rng.integers(0, 65536, 4000), np.arange(0, 0x0100), np.arange(0x8000, 0x8100),
                         [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x7F7E, 0x0001, 0x007F, 0x0080]]).astype(np.uint32)
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)
    b = ((hi[:, None] << 16) | lo[None, :]).ravel()
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    b = np.ascontiguousarray(b[~nan])
    x = b.view(f32)
    n = len(x)
    xd = torch.from_numpy(x).to(DEV)
    mid = torch.full((n + 3,), 0x55AA, dtype=torch.int16, device=DEV)
    back = torch.full((n + 3,), SENT, device=DEV)
    s = _lib.stream_handle(xd.device)
    _lib.call("pg_cast_f32_bf16", xd.data_ptr(), None, n, mid.data_ptr(), s)
    _lib.call("pg_cast_bf16_f32", mid.data_ptr(), n, back.data_ptr(), s)
    torch.cuda.synchronize()
    assert (mid.cpu()[n:] == 0x55AA).all() and (back.cpu()[n:] == SENT).all()
    ref = torch.from_numpy(x).bfloat16()
    assert np.array_equal(mid.cpu()[:n].numpy(), ref.view(torch.int16).numpy())
    assert np.array_equal(back.cpu()[:n].numpy().view(np.uint32), ref.float().numpy().view(np.uint32))
    halfway = (b & 0xFFFF) == 0x8000
    assert halfway.sum() > 1000


def _adam_case(n, wd, seed):
    from plagnn import _lib

    g = torch.Generator(device="cpu").manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.1
    v0 = torch.rand(n, generator=g) * 0.01 + 1e-6
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    st = torch.tensor([4.0, 0.0, 0.0, 0.0], device=DEV)           # the fifth step
    pd, gd, md, vd = (t.to(DEV) for t in (p0, gr, m0, v0))
    s = _lib.stream_handle(pd.device)
    _lib.call("pg_adam_prepare", st.data_ptr(), lr, b1, b2, s)
    _lib.call("pg_adam_apply", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, st.data_ptr(), b1, b2,
              eps, wd, s)
    torch.cuda.synchronize()
    sth = st.cpu().numpy().astype(np.float64)
    assert sth[0] == 5.0
    # the scalars as the header states them: formed in double, rounded to float once
    assert sth[1] == float(f32(lr / (1 - b1 ** 5))) and sth[2] == float(f32(np.sqrt(1 - b2 ** 5)))
    F = lambda x: float(f32(x))  # noqa: E731
    p, gg, m, v = (t.numpy().astype(np.float64) for t in (p0, gr, m0, v0))
    gw = gg + F(wd) * p                                           # torch 1.10: grad.add(param, alpha=wd)
    m1 = m * F(b1) + F(1 - b1) * gw
    v1 = v * F(b2) + F(1 - b2) * gw * gw
    p1 = p + (-sth[1]) * (m1 / (np.sqrt(v1) / sth[2] + F(eps)))
    got_p, got_m, got_v = (t.cpu().numpy().astype(np.float64) for t in (pd, md, vd))
    rp = float((np.abs(got_p - p1) / (1e-9 + 1e-6 * np.abs(p1))).max())
    # m and v: the header's two products and one add each, on top of g + wd p (cancellation in
    # m is measured against the operands): 6 u and 8 u of the operands' magnitudes
    gmag = np.abs(gg) + F(wd) * np.abs(p)
    rm = float((np.abs(got_m - m1) / (6 * U * (np.abs(m) * F(b1) + F(1 - b1) * gmag) + 2.0 ** -126)).max())
    rv = float((np.abs(got_v - v1) / (8 * U * (v * F(b2) + F(1 - b2) * gmag * gmag) + 2.0 ** -126)).max())
    print(f"adam n={n} wd={wd}: p err / (1e-9 + 1e-6 |p|) = {rp:.3f}, m err / bar = {rm:.3f}, v err / bar = {rv:.3f}")
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0
    return p0.numpy(), pd.cpu().numpy()


def test_adam_weight_decay_matches_float64():
    """weight_decay = 0.01 (the gradient becomes g + wd p, as torch 1.10), from non-zero m and
    v."""
    _adam_case(70_001, 0.01, 1)


def test_adam_second_grid_round():
    """n = 32768 * 256 + 5: the grid is capped at 32768 blocks of 256, so the last five
    elements are a second round of the first five threads; every one of them must move."""
    n = 32768 * 256 + 5
    p0, p1 = _adam_case(n, 0.0, 2)
    assert (p0[32768 * 256:] != p1[32768 * 256:]).all()
    assert (p0 != p1).mean() > 0.99
