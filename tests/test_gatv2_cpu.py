"""The fused GATv2 score on the CPU device: pg_gatv2_score_cpu / pg_gatv2_bwd_cpu against the
float64 references of tests/gatv2_common.py (bitwise on the grid family, derived bars on the
Gaussian one), ops.GATv2Score and dgl.nn.pytorch.GATv2Conv against float64 torch compositions,
and the module's surface."""
import pytest

import gatv2_common as vc

DEV = "cpu"


@pytest.mark.parametrize("family", vc.FAMILIES)
@pytest.mark.parametrize("H,Fh", vc.SHAPES)
@pytest.mark.parametrize("gname", vc.GRAPHS)
def test_score_and_gradients(gname, H, Fh, family):
    vc.check_kernels(DEV, gname, H, Fh, family)


@pytest.mark.parametrize("H,Fh,pad", [(2, 3, 3), (4, 64, 4)], ids=["scalar", "vector"])
def test_padded_leading_dimensions(H, Fh, pad):
    for family in vc.FAMILIES:
        vc.check_kernels(DEV, "hub", H, Fh, family, pad=pad, epad=3)


def test_each_gradient_output_alone():
    vc.check_outputs_alone(DEV)


def test_rejections():
    vc.check_rejections(DEV)


def test_empty_shapes():
    vc.check_empty_shapes(DEV)


def test_autograd_score(monkeypatch):
    vc.check_autograd_score(DEV, monkeypatch)


@pytest.mark.parametrize("fin,fout,H,residual,share,bias", [
    (20, 8, 4, False, False, True), (12, 16, 1, True, False, True), (16, 8, 2, True, True, True),
    (10, 6, 3, True, False, False)], ids=["plain", "residual", "shared_identity_residual", "no_bias"])
def test_gatv2conv(fin, fout, H, residual, share, bias):
    vc.check_gatv2conv(DEV, fin, fout, H, residual, share, bias)


def test_gatv2conv_zero_in_degree_rows():
    vc.check_gatv2conv(DEV, 20, 8, 4, self_loop=False)


def test_gatv2conv_frozen_attn_skips_dattn(monkeypatch):
    vc.check_gatv2conv_frozen_attn(DEV, monkeypatch)


def test_gatv2conv_matches_unfused_shim_composition():
    vc.check_fused_vs_unfused(DEV)


def test_module_surface():
    vc.check_module_surface(DEV)
