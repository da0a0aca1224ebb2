"""The fused GATv2 score on the GPU: the kernels behind pg_gatv2_score and pg_gatv2_bwd against
the float64 references of tests/gatv2_common.py (bitwise on the grid family, derived bars on the
Gaussian one; scalar and vector paths, H*Fh past one 256-column tile, heads that straddle a tile,
the head limit, split rows, both directions of the node-gradient kernel), agreement with the
_cpu entry points, bitwise-equal repeated calls, autograd, the module, the memory budget that
shows no edge-sized feature tensor exists, and HIP-graph capture of a whole layer step."""
import pytest
import torch

import gat_common as gc
import gatv2_common as vc
import sddmm_common as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("family", vc.FAMILIES)
@pytest.mark.parametrize("H,Fh", vc.SHAPES)
@pytest.mark.parametrize("gname", vc.GRAPHS)
def test_score_and_gradients(gname, H, Fh, family):
    vc.check_kernels(DEV, gname, H, Fh, family)


@pytest.mark.parametrize("H,Fh,pad", [(2, 3, 3), (4, 64, 4), (4, 100, 4)], ids=["scalar", "vector", "straddle"])
def test_padded_leading_dimensions(H, Fh, pad):
    for family in vc.FAMILIES:
        vc.check_kernels(DEV, "hub", H, Fh, family, pad=pad, epad=3)


def test_unaligned_vector_shape_takes_the_scalar_path():
    """Fh % 4 == 0 but a leading dimension of F + 3: the scalar kernels, the same results."""
    for family in vc.FAMILIES:
        vc.check_kernels(DEV, "hub64", 4, 64, family, pad=3)
        vc.check_kernels(DEV, "hub64", 4, 100, family, pad=3)  # two tiles, heads across them


def test_each_gradient_output_alone():
    vc.check_outputs_alone(DEV)


@pytest.mark.parametrize("H,Fh", [(4, 64), (2, 3), (3, 100)])
@pytest.mark.parametrize("gname", ["hub", "hub64"])
def test_matches_cpu_entry_points_and_repeats_bitwise(gname, H, Fh):
    """GPU vs _cpu: bitwise on the grid, within twice the bars on Gaussian inputs; two GPU calls
    on the same inputs are torch.equal."""
    for family in vc.FAMILIES:
        c = vc.case(gname, H, Fh, family)
        runs = [("s", lambda dev: vc.run_score(dev, c)),
                ("dxr", lambda dev: vc.run_bwd(dev, c, False)[0]),
                ("dxl", lambda dev: vc.run_bwd(dev, c, True)[0]),
                ("dattn", lambda dev: vc.run_bwd(dev, c, False)[1]),
                ("dattn", lambda dev: vc.run_bwd(dev, c, True)[1])]
        for key, run in runs:
            a, b, host = run(DEV), run(DEV), run("cpu")
            assert torch.equal(a, b), f"{key}: two calls differ"
            if family == "grid":
                assert torch.equal(a.cpu(), host), f"{key}: GPU and CPU differ on the grid"
            else:
                gc.within(a, host.double().numpy(), c[key][1], f"{key} GPU vs CPU", factor=2.0)


def test_rejections():
    vc.check_rejections(DEV)


def test_empty_shapes():
    vc.check_empty_shapes(DEV)
    torch.cuda.synchronize()


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


def test_no_edge_sized_feature_temporary():
    """n = 512, E = 32 768 random edges plus self-loops, H*Fh = 256: one forward + backward of
    GATv2Score allocates less than half of one (E, H, Fh) float32 tensor (16.8 MB; the node
    tensors are 0.5 MB each, the scores 0.5 MB). The unfused composition, run the same way,
    exceeds the budget, so the measurement can fail."""
    import plagnn
    from conftest import random_graph
    from plagnn import ops

    n, E0, H, Fh = 512, 32768, 4, 64
    src, dst = random_graph(n, E0, seed=5)
    g = plagnn.CSRGraph(src, dst, n)
    dg = g.on(DEV)
    E = g.num_edges
    budget = E0 * H * Fh * 4 // 2
    torch.manual_seed(3)
    xl, xr = torch.randn(n, H * Fh, device=DEV), torch.randn(n, H * Fh, device=DEV)
    attn, dS = torch.randn(1, H, Fh, device=DEV), torch.randn(E, H, device=DEV)
    d, s, _ = sc.slot_edges(g)
    s, d = torch.from_numpy(s).to(DEV), torch.from_numpy(d).to(DEV)

    def fused(a, b, w):
        return ops.GATv2Score.apply(a, b, w, dg, H, 0.2)

    def unfused(a, b, w):
        return vc.score64(s, d, a.view(n, H, Fh), b.view(n, H, Fh), w, 0.2)

    def peak(fn):
        a, b, w = (t.clone().requires_grad_(True) for t in (xl, xr, attn))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(a, b, w)
        out.backward(dS)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out.detach(), (a.grad, b.grad, w.grad)

    peak(fused)  # the library's cached scratch buffer is allocated once, before the measurement
    p_f, out_f, g_f = peak(fused)
    p_u, out_u, g_u = peak(unfused)
    print(f"peak bytes above the inputs: fused {p_f}, unfused {p_u}, budget {budget}")
    assert p_f < budget
    assert p_u > budget
    sc.close(out_f, out_u, 1e-5, "scores")
    for a, b, name in zip(g_f, g_u, ("d xl", "d xr", "d attn")):
        sc.close(a, b, 1e-5, name)


def test_graph_capture_of_a_layer_step():
    """A forward + backward of GATv2Conv captured in a HIP graph on one stream: the entry points
    allocate nothing and do not synchronise, and the replays equal the eager step."""
    src, dst, g, rng, conv = vc.conv_case(DEV, 12, 8, 4, True, False, True)
    n = g.num_nodes()
    x = gc._randn(rng, n, 12).to(DEV).requires_grad_(True)
    dZ = gc._randn(rng, n, 4, 8).to(DEV)
    params = [x] + list(conv.parameters())

    def step():
        y = conv(g, x)
        (y * dZ).sum().backward()
        return y

    y_eager = step().detach().clone()
    g_eager = [p.grad.detach().clone() for p in params]
    for p in params:
        p.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_cap = step()
    for _ in range(2):
        y_cap.detach().zero_()
        for p in params:
            p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        sc.close(y_cap, y_eager, 1e-5, "captured out")
        for p, e in zip(params, g_eager):
            sc.close(p.grad, e, 1e-5, "captured grad")
