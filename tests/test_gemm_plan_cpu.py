"""The GEMM host plans are pinned: the split-K recommendations, the workspace sizes and the
grouped launches' workspace sizes of the f32 and bf16 families equal the values recorded in
tests/golden/gemm_plan.json. These are host functions (they read sizes, never an operand),
so the test needs no GPU. A change of a tile rule, a split target or the slab layout shows
here first; a refactor of the host front end must leave every value where it is.

The fixture was recorded from the library before the shared front end (csrc/gemm_host.hpp)
existed. To regenerate it after a deliberate change of a plan:

    python tests/test_gemm_plan_cpu.py --write
"""
import json
import os
import sys
from types import SimpleNamespace

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.json")

EXTENTS = [1, 63, 64, 65, 128, 129, 256, 512, 513, 1024]
K_EXTRA = [1023, 2047, 2048, 24041, 384656]  # (1024 is among EXTENTS already)
# (engine class name, dims, nodes): the weight-gradient products of the cfg2 and cfg5 steps
ENGINES = {"cfg2": ("TrainEngine", [503, 256, 256, 256, 100, 12], 24041),
           "cfg5": ("TrainEngineBF16", [503, 512, 512, 512, 100, 12], 384656)}


def _wgrad_shapes(name):
    """TrainEngine._wgrad_shapes of a config, from the padded widths its constructor derives
    (plagnn/engine.py, TrainEngine.__init__, "pd = ...": WIDTH_ALIGN, then SAGE inputs to a
    multiple of 64 when that costs <= 2 %; a change of that rule has to be made here too, and
    the fixture's "shapes" lists then show it)."""
    from plagnn import engine, engine_bf16

    cls_name, dims, n = ENGINES[name]
    cls = getattr(engine_bf16 if cls_name.endswith("BF16") else engine, cls_name)
    a, L = cls.WIDTH_ALIGN, len(dims) - 3
    pd = [(d + a - 1) // a * a for d in dims]
    for l in range(L):
        r64 = -(-dims[l] // 64) * 64
        if r64 <= 1.02 * dims[l]:
            pd[l] = r64
    return [list(s) for s in cls._wgrad_shapes(SimpleNamespace(pd=pd, N=n, L=L))]


def _shapes():
    out = [[m, n, k] for m in EXTENTS for n in EXTENTS for k in EXTENTS + K_EXTRA]
    return out + _wgrad_shapes("cfg2") + _wgrad_shapes("cfg5")


def _part_lists():
    return {
        "cfg2": _wgrad_shapes("cfg2"),
        "cfg5": _wgrad_shapes("cfg5"),
        "single": [[512, 1024, 24041]],
        "sixteen": [[64 * (1 + p % 4), 256 + 8 * p, 2048 + 1000 * p] for p in range(16)],
        "m8": [[8, 512, 384656]],  # 256 x 256 tiles would waste > 4x its area: not a bf16 group member
    }


def _plans():
    from plagnn import _lib

    L = _lib.lib()
    table = []
    for m, n, k in _shapes():
        sf, sb = int(L.pg_gemm_f32_split_k(m, n, k)), int(L.pg_gemm_bf16_split_k(m, n, k))
        table.append([m, n, k, sf, int(L.pg_gemm_f32_workspace(m, n, k, sf)), sb,
                      int(L.pg_gemm_bf16_workspace(m, n, k, sb))])
    groups = {}
    for name, shapes in _part_lists().items():
        parts = (_lib.PgGemmPart * len(shapes))()
        for q, (m, n, k) in zip(parts, shapes):  # transposed A, plain B: a weight gradient dY^T X
            q.transa, q.transb, q.M, q.N, q.K = 1, 0, m, n, k
        groups[name] = {"shapes": shapes,
                        "f32": int(L.pg_gemm_f32_group_workspace(parts, len(shapes))),
                        "bf16": int(L.pg_gemm_bf16_group_workspace(parts, len(shapes)))}
    return {"columns": ["M", "N", "K", "f32_split_k", "f32_workspace", "bf16_split_k", "bf16_workspace"],
            "table": table, "groups": groups}


def test_gemm_plans_match_the_fixture():
    want = json.load(open(FIXTURE))
    got = _plans()
    assert got["columns"] == want["columns"]
    assert len(got["table"]) == len(want["table"]) == len(EXTENTS) ** 2 * (len(EXTENTS) + len(K_EXTRA)) + 16
    bad = [(g, w) for g, w in zip(got["table"], want["table"]) if g != w]
    assert not bad, f"{len(bad)} plans moved, first (got, want): {bad[0]}"
    assert got["groups"] == want["groups"]
    # the fixture exercises what it claims: split and unsplit plans of both families, and a
    # grouped workspace larger than the minimum
    assert any(r[3] > 1 for r in want["table"]) and any(r[5] > 1 for r in want["table"])
    assert all(v["f32"] >= 256 and v["bf16"] >= 256 for v in want["groups"].values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pla-gnn_amd"))
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(FIXTURE, "w") as f:
        json.dump(_plans(), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE)
