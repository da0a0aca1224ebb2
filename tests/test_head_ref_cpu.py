"""Pins tests/head_common.py's references before the GPU tests rely on them: loss_ref, fed
torch's own float32 probabilities, against oracle.multi_loss(torch.sigmoid(z32), t, w)
through float32 autograd on the CPU, inside the same bars the kernels get and with torch's
zero pattern exactly; sigmoid_ref against torch.sigmoid. Logits: N(0, 3) mixed with the
saturated values +-30, +-100, 17 and -20.8; C in {1, 3, 12, 16}.

Largest error-to-bar ratios here (torch 2.x CPU): sigmoid 0.46, dz 0.38, loss 0.011."""
import numpy as np
import pytest
import torch

import head_common as H


def _case(C, seed):
    rng = np.random.default_rng(seed)
    n = 300
    z = H.mixed_logits(rng, (n, C))
    t = (rng.random((n, C)) < 0.3).astype(np.float32)
    w = rng.uniform(0.5, 30.0, C)
    rows = rng.permutation(n)[:173]
    return z, t, w, rows


@pytest.mark.parametrize("C", [1, 3, 12, 16])
def test_loss_ref_matches_torch_autograd(C):
    import oracle

    z, t, w, rows = _case(C, 100 + C)
    zt = torch.from_numpy(z).requires_grad_(True)
    p = torch.sigmoid(zt)
    idx = torch.from_numpy(rows)
    loss = oracle.multi_loss(p[idx], torch.from_numpy(t)[idx], w)
    loss.backward()
    p32 = p.detach().numpy()
    s, bar = H.sigmoid_ref(z)
    H.check("torch sigmoid", p32, s, bar)
    lr = H.loss_ref(p32, t, w, rows)
    H.coverage(lr["lowp"], lr["q0"])
    g = zt.grad.numpy()
    H.check_dz("torch dz", g[rows], lr)
    assert ((g[rows] == 0) == (lr["dz"] == 0)).all()   # the zero patterns are identical
    rest = np.setdiff1d(np.arange(len(z)), rows)
    assert not g[rest].any()
    H.check("torch loss", np.float64(loss.item()), np.float64(lr["loss"]), lr["loss_bar"])


def test_loss_ref_masks_follow_the_clamp():
    """The clamp's zero gradient, on hand-made probabilities: p = 0 and p just below 1e-9
    (ga masked, gb alive), p = float32(1e-9) itself (inside: torch.clamp passes its edges),
    p = 1 (q = 0: gb masked, and the factor q zeroes dz)."""
    lo = np.float32(1e-9)
    p = np.array([[0.0], [np.nextafter(lo, np.float32(0))], [lo], [0.5], [1.0]], np.float32)
    for tv in (0.0, 1.0):
        t = np.full_like(p, tv)
        pt = torch.from_numpy(p).requires_grad_(True)
        import oracle

        oracle.multi_loss(pt, torch.from_numpy(t), np.array([3.0])).backward()
        lr = H.loss_ref(p, t, np.array([3.0]), np.arange(len(p)))
        q = (np.float32(1) - p).astype(np.float64)
        dz_t = pt.grad.numpy().astype(np.float64) * q * p     # sigmoid_backward(grad, out)
        assert ((dz_t == 0) == (lr["dz"] == 0)).all()
        H.check(f"dz, t = {tv}", dz_t, lr["dz"], 8 * H.U * lr["mag"] + H.TINY)
        if tv == 1.0:
            assert lr["dz"][1] == 0 and lr["dz"][2] != 0      # the edge itself is inside
