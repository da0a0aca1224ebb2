"""Shared by test_gpu_max_paths.py, test_gpu_max_strides.py and test_max_strides_cpu.py: the
max family's graph, exact-integer operands and host-twin results, the window / sentinel
harness for leading dimensions and base pointers, the dispatch contract of include/plagnn.h
restated in plain Python (predict_*), and the case tables of the stride suite.

Data (case): small integers with 30 % zeros and weights from {-1, 0.5, 1, 2}, so every
product is exact in f32 and in bf16, most maxima are ties, and the backward's sums are exact
in any order: every comparison against the twins pg_spmm_max_fwd_cpu / pg_spmm_max_bwd_cpu
(on contiguous operands) is of bit patterns, for bf16 storage of the twin's value rounded
once to bf16. No tolerance appears anywhere.

Windows: an operand is the columns [:, :F] of an (n, ld) buffer whose base sits `off`
elements past a 16-byte boundary; the pad columns and the elements before and after hold a
fill chosen so that a pad value that is read changes the result and a pad element that is
written is seen (untouched compares bit patterns):
  X pads 2^100 (exact in bf16, wins every maximum); dout, mask, fwd_out pads NaN; out and dx
  NaN before the call; argpos 0x7F7F / 0x7F7F7F7F before the forward (neither a position nor
  "none"). A record buffer that is an input holds "none" in its pads: a record read from a
  pad drops a term, and no position past a row's end reaches a kernel.

predict_* are checks of the tables (every path reached, each single-term case differs from
its baseline in exactly the decision it names), like sum_common.check_width_list; they do
not observe what the GPU ran.
"""
import functools

import numpy as np
import torch

import sum_common as sm

CHUNK = 4
U16, I32 = 16, 32  # PG_ARG_U16, PG_ARG_I32
X_PAD = 2.0 ** 100
NAN = float("nan")
ARG_JUNK = {U16: 0x7F7F, I32: 0x7F7F7F7F}
ARG_NONE = -1  # 0xFFFF as int16, -1 as int32
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


# ------------------------------------------------------------------ graph and operands
@functools.lru_cache(maxsize=None)
def graph(trans=False, i32=False):
    """The ladder graph at chunk 4 (sum_common.ladder_graph checks its degrees); trans: with
    the in-CSR slots' transposed indices (g->epos); i32: 4-byte records on a graph whose
    degrees would fit u16."""
    import plagnn
    from plagnn import _lib

    base = sm.ladder_graph(chunk=CHUNK)
    if not trans and not i32:
        g = base
    else:
        src, dst, degs = sm.ladder_coo(CHUNK)
        g = plagnn.CSRGraph(src, dst, len(degs), chunk=CHUNK, bwd_trans=trans)
        if i32:
            g.arg_kind = _lib.PG_ARG_I32
    assert g.bwd_trans == trans and (g.fwd.epos is not None) == trans
    assert g.fwd.n_merges >= 3 and g.bwd.n_merges > 0 and g.bwd.epos is not None
    return g


def _frozen(ts):
    res = tuple(None if t is None else t.numpy() for t in ts)
    for a in res:
        if a is not None:
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(F, weighted, i32):
    """(X, w, out, argpos, dout, dx, dx_masked) of one shape from the host twins, computed once
    and never modified; w in in-CSR slot order or None."""
    from plagnn import ops

    g = graph(False, i32)
    rng = np.random.default_rng(7 * F + weighted)
    X = rng.integers(-3, 4, (g.num_src, F)).astype(np.float32)
    X[rng.random(X.shape) < 0.3] = 0.0
    w = rng.choice(np.array([-1.0, 0.5, 1.0, 2.0], np.float32), g.num_edges) if weighted else None
    dout = rng.integers(-4, 5, (g.num_dst, F)).astype(np.float32)
    cg = g.on("cpu")
    Xt, dt = torch.from_numpy(X), torch.from_numpy(dout)
    wt = None if w is None else torch.from_numpy(w)
    out, arg = ops.spmm_max(cg, Xt, wt)
    dx = ops.spmm_max_backward(cg, arg, dt, wt)
    dxm = ops.spmm_max_backward(cg, arg, dt, wt, mask=Xt)
    return _frozen((Xt, wt, out, arg, dt, dx, dxm))


@functools.lru_cache(maxsize=None)
def relu_case(F, weighted):
    """(X, w, argpos, dout, dx) for PG_ARG_DEAD_NONE records (u16): X = relu of case's X (the
    flag's contract: X >= 0), argpos with "none" wherever the maximum is 0, dx the twin's
    masked result on those records (a skipped entry's winner has X = 0, so it is masked)."""
    from plagnn import ops

    X, w, _, _, dout, _, _ = case(F, weighted, False)
    cg = graph(False, False).on("cpu")
    Xt, dt = torch.from_numpy(np.maximum(X, np.float32(0))), torch.from_numpy(np.array(dout))
    wt = None if w is None else torch.from_numpy(np.array(w))
    out, arg = ops.spmm_max(cg, Xt, wt)
    arg = torch.where(out == 0, torch.full_like(arg, ARG_NONE), arg)
    assert (arg == ARG_NONE).float().mean() > 0.2 and (arg != ARG_NONE).float().mean() > 0.2
    dx = ops.spmm_max_backward(cg, arg, dt, wt, mask=Xt)
    return _frozen((Xt, wt, arg, dt, dx))


@functools.lru_cache(maxsize=None)
def rows_case(F, weighted):
    """(active [N] bool, dout with NaN in the inactive rows, dx) for pg_spmm_max_bwd_rows: the
    longest destination row and every third row inactive; they count as zero in the twin."""
    from plagnn import ops

    _, w, _, arg, dout, *_ = case(F, weighted, False)
    g = graph(False, False)
    active = np.ones(g.num_dst, bool)
    active[::3] = False
    hub = int(np.argmax(g.in_degrees()))
    active[hub] = False
    assert g.in_degrees()[hub] == 129 and active.sum() > g.num_dst // 2
    zeroed = np.where(active[:, None], dout, np.float32(0))
    wt = None if w is None else torch.from_numpy(np.array(w))
    dx = ops.spmm_max_backward(g.on("cpu"), torch.from_numpy(np.array(arg)), torch.from_numpy(zeroed), wt)
    holes = np.where(active[:, None], dout, np.float32("nan")).astype(np.float32)
    res = (active, holes, dx.numpy())
    for a in res:
        a.setflags(write=False)
    return res


def same(got, want, name):
    """got (f32 or bf16, on the device) holds exactly the f32 twin's bits; bf16 storage: the
    twin's values rounded once to bf16 (round to nearest even, as the kernels' stores)."""
    assert tuple(got.shape) == want.shape, name
    if got.dtype == torch.bfloat16:
        want = torch.from_numpy(np.array(want)).to(torch.bfloat16).float().numpy()
    sm.assert_bits(got.float(), want, name)


# ------------------------------------------------------------------ windows
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Window:
    """See window(). view: the (n, F) operand; flat: the whole buffer, from the 16-byte
    boundary; ptr / ld: what the C-ABI takes."""

    def __init__(self, t, ld, off, fill):
        n, F = t.shape
        assert ld >= F and off >= 0
        self.n, self.F, self.ld, self.off, self.fill = n, F, ld, off, fill
        self.flat = torch.full((off + n * ld + 4,), fill, dtype=t.dtype, device=t.device)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[off:off + n * ld].view(n, ld)[:, :F]
        self.view.copy_(t)
        self.ptr = self.view.data_ptr()
        assert self.ptr == self.flat.data_ptr() + off * t.element_size() and self.view.stride(0) == ld

    def bits(self):
        """The window's bit patterns, contiguous, on the host."""
        return self.view.contiguous().view(_INT[self.view.element_size()]).cpu()


def window(t, ld, off, fill):
    """The 2-D tensor t as the columns [:, :F] of an (n, ld) buffer whose base sits `off`
    elements past a 16-byte boundary; the pad columns and the elements before and after the
    rows hold `fill`."""
    return Window(t, ld, off, fill)


def filled(n, F, dtype, dev, ld, off, fill):
    """An output window that holds `fill` everywhere, inside too."""
    return Window(torch.full((n, F), fill, dtype=dtype, device=dev), ld, off, fill)


def untouched(win, fill=None):
    """Everything of the buffer outside the window still holds `fill`, compared as integers
    (bit patterns), so a NaN sentinel works."""
    fill = win.fill if fill is None else fill
    it = _INT[win.flat.element_size()]
    keep = torch.ones(win.flat.numel(), dtype=torch.bool, device=win.flat.device)
    keep[win.off:win.off + win.n * win.ld].view(win.n, win.ld)[:, :win.F] = False
    want = torch.full_like(win.flat, fill)
    return bool((win.flat.view(it)[keep] == want.view(it)[keep]).all())


def holds(win, fill=None):
    """The window itself still holds `fill` in every element (a rejected call wrote nothing)."""
    fill = win.fill if fill is None else fill
    it = _INT[win.flat.element_size()]
    return bool((win.flat.view(it) == torch.full_like(win.flat, fill).view(it)).all())


def workspace(nbytes, dev, off=0):
    """nbytes of scratch whose base sits `off` bytes past a 256-byte boundary."""
    buf = torch.empty(int(nbytes) + 512 + off, dtype=torch.uint8, device=dev)
    ws = buf[(-buf.data_ptr()) % 256 + off:]
    assert ws.data_ptr() % 256 == off % 256 and ws.numel() >= nbytes
    return ws


# ------------------------------------------------------------------ the contract, restated
def _ld(F, spec, key):
    return F + spec[key][0]


def _al(spec, key, esize, nbytes):
    return (spec[key][1] * esize) % nbytes == 0


def predict_fwd(F, spec, kind, esize):
    """(vector | scalar, slices | whole_row | scalar_tiles_<n>, in_launch | by_launch) of
    pg_spmm_max_fwd[_bf16] on a graph with split rows; spec: operand -> (pad, offset in
    elements) for X, out, arg and the workspace's offset in bytes past a 256-byte boundary."""
    rsize = kind // 8
    vec = (F % 4 == 0 and all(_ld(F, spec, k) % 4 == 0 for k in ("X", "out", "arg"))
           and _al(spec, "X", esize, 16) and _al(spec, "out", esize, 16) and spec["ws"] % 16 == 0
           and _al(spec, "arg", rsize, 4 * rsize))
    if not vec:
        return "scalar", f"scalar_tiles_{-(-F // 1024)}", "by_launch"
    lpr0 = min(32, 256 // (4 * esize))
    for lpr in (lpr0, 2 * lpr0):
        n_sl = -(-F // (4 * lpr))
        if lpr <= 32 and (n_sl % 8 == 0 or n_sl in (1, 2, 4)):
            return "vector", "slices", "in_launch"  # split rows whole, by the launch's first workgroups
    return "vector", "whole_row", "in_launch" if spec["ws"] % 256 == 0 else "by_launch"


def predict_bwd(F, spec, mode, esize):
    """(pack vector | scalar, pull merge_in | by_launch) of the grouped backward on a graph
    whose transpose has split rows; mode: plain (no mask), mask, mask_fout, dead_none."""
    assert spec["ws"] % 16 == 0, "below 16 bytes the call is rejected"
    a4 = lambda k, sz: _al(spec, k, sz, 4 * sz)  # noqa: E731
    pack = (F % 4 == 0 and _ld(F, spec, "arg") % 4 == 0 and _ld(F, spec, "dout") % 4 == 0 and a4("arg", 2)
            and a4("dout", esize))
    if mode == "mask_fout":
        pack = pack and _ld(F, spec, "fout") % 4 == 0 and a4("fout", esize)
    pull = F % 4 == 0 and _ld(F, spec, "dx") % 4 == 0 and a4("dx", esize)
    if mode in ("mask", "mask_fout"):  # dead_none: the mask is implied and not read
        pull = pull and _ld(F, spec, "mask") % 4 == 0 and a4("mask", esize)
    return "vector" if pack else "scalar", "merge_in" if pull else "by_launch"


def predict_gather(F, spec, mode):
    """(vector | scalar, launches) of launch_max_bwd (i32 records, f32)."""
    keys = ["arg", "dout", "dx"] + (["mask"] if mode == "mask" else [])
    vec = (F % 4 == 0 and all(_ld(F, spec, k) % 4 == 0 for k in keys) and spec["ws"] % 16 == 0
           and all(_al(spec, k, 4, 16) for k in keys))
    return ("vector", -(-F // 256)) if vec else ("scalar", -(-F // 1024))


# ------------------------------------------------------------------ case tables
def _with(base, **kw):
    d = dict(base)
    d.update(kw)
    return d


# the baseline: every operand in a window, distinct 4-multiple pads (a swapped pair shows),
# aligned bases
FWD_BASE = {"X": (4, 0), "out": (8, 0), "arg": (12, 0), "ws": 0}
FWD_FLAT = {"X": (0, 0), "out": (0, 0), "arg": (0, 0), "ws": 0}
# id, spec, record kinds, the path the term must give
FWD_TERMS = [
    ("baseline", FWD_BASE, (U16, I32), "vector"),
    ("ldx_odd", _with(FWD_BASE, X=(1, 0)), (U16, I32), "scalar"),
    ("ldo_odd", _with(FWD_BASE, out=(1, 0)), (U16, I32), "scalar"),
    ("lda_odd", _with(FWD_BASE, arg=(1, 0)), (U16, I32), "scalar"),
    ("x_off1", _with(FWD_BASE, X=(4, 1)), (U16, I32), "scalar"),
    ("out_off1", _with(FWD_BASE, out=(8, 1)), (U16, I32), "scalar"),
    ("arg_off1", _with(FWD_BASE, arg=(12, 1)), (U16, I32), "scalar"),
    ("arg_off4", _with(FWD_BASE, arg=(12, 4)), (U16,), "vector"),  # 8 bytes: enough for u16 records
    ("arg_off2", _with(FWD_BASE, arg=(12, 2)), (I32,), "scalar"),  # 8 bytes: not for i32
]
FWD_WIDTHS = (256, 300)  # vector: slices; whole rows in two feature tiles


def _fwd_cases():
    cases = []
    for F in FWD_WIDTHS:
        for i, (name, spec, kinds, want) in enumerate(FWD_TERMS):
            for kind in kinds:
                for dt in DTYPES:
                    cases.append((f"{name}-F{F}-{dt}-{'u16' if kind == U16 else 'i32'}", F, dt, kind,
                                  (i + (F == 300)) % 2 == 1, spec, want))
    # the vector whole-row path with split rows combined by max_merge_kernel's launch
    for dt in DTYPES:
        cases.append((f"ws16-F300-{dt}-u16", 300, dt, U16, dt == "bf16", _with(FWD_BASE, ws=16), "vector"))
    # the scalar path past one 1024-column tile
    for dt in DTYPES:
        cases.append((f"tiles_flat-F1027-{dt}-u16", 1027, dt, U16, dt == "f32", FWD_FLAT, "scalar"))
        cases.append((f"tiles_ldx-F1100-{dt}-u16", 1100, dt, U16, dt == "bf16", _with(FWD_BASE, X=(1, 0)), "scalar"))
    cases.append(("tiles_ldx-F1100-f32-i32", 1100, "f32", I32, True, _with(FWD_BASE, X=(1, 0)), "scalar"))
    return cases


FWD_CASES = _fwd_cases()

BWD_BASE = {"arg": (4, 0), "dout": (8, 0), "fout": (12, 0), "dx": (16, 0), "mask": (20, 0), "ws": 0}
BWD_MODES = ("mask", "mask_fout", "dead_none")
# id, spec, side (which decision the term names), the modes in which the operand is read
BWD_TERMS = [
    ("baseline", BWD_BASE, None, BWD_MODES),
    ("lda_odd", _with(BWD_BASE, arg=(1, 0)), "pack", BWD_MODES),
    ("ldd_odd", _with(BWD_BASE, dout=(1, 0)), "pack", BWD_MODES),
    ("ldf_odd", _with(BWD_BASE, fout=(1, 0)), "pack", ("mask_fout",)),
    ("arg_off1", _with(BWD_BASE, arg=(4, 1)), "pack", BWD_MODES),
    ("dout_off1", _with(BWD_BASE, dout=(8, 1)), "pack", BWD_MODES),
    ("fout_off1", _with(BWD_BASE, fout=(12, 1)), "pack", ("mask_fout",)),
    ("ldx_odd", _with(BWD_BASE, dx=(1, 0)), "pull", BWD_MODES),
    ("dx_off1", _with(BWD_BASE, dx=(16, 1)), "pull", BWD_MODES),
    ("ldm_odd", _with(BWD_BASE, mask=(1, 0)), "pull", ("mask", "mask_fout")),
    ("mask_off1", _with(BWD_BASE, mask=(20, 1)), "pull", ("mask", "mask_fout")),
    ("both", _with(BWD_BASE, dout=(1, 0), dx=(1, 0)), "both", BWD_MODES),
    ("ws16", _with(BWD_BASE, ws=16), None, BWD_MODES),
]
BWD_F = 260


def bwd_expect(side, mode, modes):
    """The (pack, pull) a term of BWD_TERMS must give in `mode`."""
    if mode not in modes:
        side = None  # the operand is not read in this mode: the baseline's decisions
    return ("scalar" if side in ("pack", "both") else "vector",
            "by_launch" if side in ("pull", "both") else "merge_in")


def _bwd_cases():
    cases = []
    for name, spec, side, modes in BWD_TERMS:
        for mode in BWD_MODES:
            if name in ("ldf_odd", "fout_off1") and mode != "mask_fout":
                continue  # no fwd_out operand in the call
            for dt in DTYPES:
                for trans in (False, True):
                    for weighted in (False, True):
                        cases.append((f"{name}-{mode}-{dt}-{'epos' if trans else 'slots'}-{'w' if weighted else 'u'}",
                                      BWD_F, dt, trans, weighted, mode, spec, bwd_expect(side, mode, modes)))
    for name, spec, want in (("baseline", BWD_BASE, ("vector", "merge_in")),
                             ("ldx_odd", _with(BWD_BASE, dx=(1, 0)), ("vector", "by_launch"))):
        for dt in DTYPES:
            for trans in (False, True):
                cases.append((f"{name}-F1024-mask-{dt}-{'epos' if trans else 'slots'}-u", 1024, dt, trans, False,
                              "mask", spec, want))
    return cases


BWD_CASES = _bwd_cases()

ROWS_TERMS = [("baseline", BWD_BASE, ("vector", "merge_in")),
              ("ldd_odd", _with(BWD_BASE, dout=(1, 0)), ("scalar", "merge_in")),
              ("ldx_odd", _with(BWD_BASE, dx=(1, 0)), ("vector", "by_launch"))]
ROWS_CASES = [(f"{name}-{dt}-{'epos' if trans else 'slots'}", BWD_F, dt, trans, True, "plain", spec, want)
              for name, spec, want in ROWS_TERMS for dt in DTYPES for trans in (False, True)]

# launch_max_bwd: i32 records, f32, with the relu' mask; id, F, weighted, spec, (path, launches)
GATHER_CASES = [
    ("baseline-F260", 260, False, BWD_BASE, ("vector", 2)),
    ("lda_odd-F260", 260, True, _with(BWD_BASE, arg=(1, 0)), ("scalar", 1)),
    ("ldd_odd-F260", 260, False, _with(BWD_BASE, dout=(1, 0)), ("scalar", 1)),
    ("ldx_odd-F260", 260, True, _with(BWD_BASE, dx=(1, 0)), ("scalar", 1)),
    ("ldm_odd-F260", 260, False, _with(BWD_BASE, mask=(1, 0)), ("scalar", 1)),
    ("ldd_odd-F1100", 1100, True, _with(BWD_BASE, dout=(1, 0)), ("scalar", 2)),
]

SCATTER_SPEC = {"arg": (3, 0), "dout": (8, 0), "dx": (5, 1)}
SCATTER_CASES = [(f"F{F}-{'u16' if kind == U16 else 'i32'}-{'w' if weighted else 'u'}", F, kind, weighted)
                 for F in (65, 260) for kind in (U16, I32) for weighted in (False, True)]
ARGSRC_SPEC = {"arg": (3, 1), "argx": (5, 1)}


def check_tables():
    """The tables against the restated contract: every path predict_* can return is reached,
    each single-term case gives exactly the decision it names, both storage types, both
    record kinds and both descriptor placements occur."""
    seen = set()
    for name, F, dt, kind, _w, spec, want in FWD_CASES:
        got = predict_fwd(F, spec, kind, DTYPES[dt].itemsize)
        assert got[0] == want, (name, got)
        seen.add(got)
        if F in FWD_WIDTHS:
            base = predict_fwd(F, _with(FWD_BASE, ws=spec["ws"]), kind, DTYPES[dt].itemsize)
            assert base[0] == "vector" and base[1] == ("slices" if F == 256 else "whole_row"), (name, base)
            differs = [k for k in FWD_BASE if spec[k] != FWD_BASE[k]]
            assert len(differs) <= 1, name  # one term at a time
            assert (got == base) == (want == "vector"), (name, got, base)
    assert seen == {("vector", "slices", "in_launch"), ("vector", "whole_row", "in_launch"),
                    ("vector", "whole_row", "by_launch"), ("scalar", "scalar_tiles_1", "by_launch"),
                    ("scalar", "scalar_tiles_2", "by_launch")}, seen
    assert {(c[2], c[3]) for c in FWD_CASES} == {(d, k) for d in DTYPES for k in (U16, I32)}
    assert {c[4] for c in FWD_CASES if c[1] == 256} == {False, True} == {c[4] for c in FWD_CASES if c[1] == 300}

    seen = set()
    for name, F, dt, _trans, _w, mode, spec, want in BWD_CASES + ROWS_CASES:
        got = predict_bwd(F, spec, mode, DTYPES[dt].itemsize)
        assert got == want, (name, got, want)
        seen.add((got, dt, _trans))
    for combo in (("vector", "merge_in"), ("vector", "by_launch"), ("scalar", "merge_in"), ("scalar", "by_launch")):
        for dt in DTYPES:
            for trans in (False, True):
                assert (combo, dt, trans) in seen, (combo, dt, trans)
    for name, spec, side, modes in BWD_TERMS:  # one term at a time, each its own decision
        differs = [k for k in BWD_BASE if spec[k] != BWD_BASE[k]]
        assert len(differs) == {None: 0, "both": 2}.get(side, 1) or name == "ws16", name
        for mode in BWD_MODES:
            base = predict_bwd(BWD_F, BWD_BASE, mode, 4)
            got = predict_bwd(BWD_F, spec, mode, 4)
            assert base == ("vector", "merge_in")
            changed = {i for i in (0, 1) if got[i] != base[i]}
            named = {"pack": {0}, "pull": {1}, "both": {0, 1}, None: set()}[side if mode in modes else None]
            assert changed == named, (name, mode, got)
    # dead-none records: an odd ldm or an offset mask does not change the pull's decision
    for name in ("ldm_odd", "mask_off1"):
        spec = dict((t[0], t[1]) for t in BWD_TERMS)[name]
        assert predict_bwd(BWD_F, spec, "dead_none", 4) == ("vector", "merge_in")
    assert {c[5] for c in BWD_CASES} == set(BWD_MODES)
    assert {c[4] for c in BWD_CASES if c[2] == "bf16"} == {False, True}  # 4-byte and 8-byte records

    seen = set()
    for name, F, _w, spec, want in GATHER_CASES:
        got = predict_gather(F, spec, "mask")
        assert got == want, (name, got)
        seen.add(got)
    assert seen == {("vector", 2), ("scalar", 1), ("scalar", 2)}
    for spec in (SCATTER_SPEC, ARGSRC_SPEC):  # distinct pads, an odd one among them
        pads = [p for p, _ in spec.values()]
        assert len(set(pads)) == len(pads) and any(p % 2 for p in pads)
    for base in (FWD_BASE, BWD_BASE):
        pads = [v[0] for k, v in base.items() if k != "ws"]
        assert len(set(pads)) == len(pads) and all(p % 4 == 0 and p > 0 for p in pads)


# ------------------------------------------------------------------ runners (GPU, or the _cpu twins)
def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def _weights(F, weighted, i32, dev, relu=False):
    w = (relu_case(F, weighted)[1] if relu else case(F, weighted, i32)[1])
    return None if w is None else _t(w, dev)


def _win(t, F, spec, key, fill):
    return window(t, F + spec[key][0], spec[key][1], fill)


def _out(n, F, dtype, dev, spec, key, fill):
    return filled(n, F, dtype, dev, F + spec[key][0], spec[key][1], fill)


def _stream(dev):
    return torch.cuda.current_stream().cuda_stream if dev != "cpu" else None


def run_fwd(dev, F, dt, kind, weighted, spec, name):
    """pg_spmm_max_fwd[_bf16] (dev "cpu": pg_spmm_max_fwd_cpu) with every operand in its
    window: values and positions bitwise the twin's, nothing outside the windows written, a
    second call into fresh buffers the same bits."""
    from plagnn import _lib

    dtype, i32 = DTYPES[dt], kind == I32
    X, _, out_ref, arg_ref, *_ = case(F, weighted, i32)
    g = graph(False, i32)
    dg = g.on(dev)
    assert dg.arg_kind == kind
    gs = dg.fwd.struct(_weights(F, weighted, i32, dev))
    Xw = _win(_t(X, dev, dtype), F, spec, "X", X_PAD)
    adt = torch.int32 if i32 else torch.int16
    x_bits = Xw.flat.clone()
    if dev != "cpu":
        ws_n = _lib.lib().pg_spmm_max_fwd_workspace(gs, F, kind)
        ws = workspace(ws_n, dev, spec["ws"])

    def once():
        ow = _out(g.num_dst, F, dtype, dev, spec, "out", NAN)
        aw = _out(g.num_dst, F, adt, dev, spec, "arg", ARG_JUNK[kind])
        if dev == "cpu":
            assert dtype == torch.float32
            _lib.call("pg_spmm_max_fwd_cpu", gs, Xw.ptr, Xw.ld, F, ow.ptr, ow.ld, aw.ptr, aw.ld, kind)
        else:
            _lib.call("pg_spmm_max_fwd" + ("_bf16" if dt == "bf16" else ""), gs, Xw.ptr, Xw.ld, F, ow.ptr, ow.ld,
                      aw.ptr, aw.ld, kind, ws.data_ptr(), ws_n, _stream(dev))
        return ow, aw

    ow, aw = once()
    ow2, aw2 = once()
    same(ow.view, out_ref, f"{name}: values")
    assert np.array_equal(aw.view.cpu().numpy(), arg_ref), f"{name}: positions"
    assert untouched(ow) and untouched(aw), f"{name}: written outside the F columns"
    assert torch.equal(ow.bits(), ow2.bits()) and torch.equal(aw.bits(), aw2.bits()), f"{name}: second call"
    assert untouched(ow2) and untouched(aw2), f"{name}: second call wrote outside the F columns"
    assert torch.equal(Xw.flat.view(_INT[Xw.flat.element_size()]), x_bits.view(_INT[x_bits.element_size()])), name


def bwd_operands(dev, F, dt, weighted, i32, mode, spec, rows=False):
    """(windows of argpos, dout, mask, fwd_out; the twin's dx; edge weights) of one backward
    case. dead_none: the mask buffer holds NaN everywhere (it must not be read)."""
    dtype = DTYPES[dt]
    if mode == "dead_none":
        X, _, arg, dout, ref = relu_case(F, weighted)
        out = None
    else:
        X, _, out, arg, dout, dx, dxm = case(F, weighted, i32)
        ref = dx if mode == "plain" else dxm
    if rows:
        assert mode == "plain"
        _, dout, ref = rows_case(F, weighted)
    aw = _win(_t(arg, dev), F, spec, "arg", ARG_NONE)
    dw = _win(_t(dout, dev, dtype), F, spec, "dout", NAN)
    mw = fw = None
    if mode == "dead_none":
        mw = _out(X.shape[0], F, dtype, dev, spec, "mask", NAN)
    elif mode != "plain":
        mw = _win(_t(X, dev, dtype), F, spec, "mask", NAN)
    if mode == "mask_fout":
        fw = _win(_t(out, dev, dtype), F, spec, "fout", NAN)
    return aw, dw, mw, fw, ref, _weights(F, weighted, i32, dev, relu=mode == "dead_none")


def bwd_call(dev, entry, g, dg, wd, F, dt, kind, aw, dw, mw, fw, xw, ws_off=0, rows=None):
    """One call of pg_spmm_max_bwd[_rows][_bf16] (dev "cpu": pg_spmm_max_bwd_cpu) on windows."""
    from plagnn import _lib

    fs, gt = dg.fwd.struct(wd), dg.bwd.struct(None)
    p = lambda w: None if w is None else w.ptr  # noqa: E731
    ld = lambda w: 0 if w is None else w.ld  # noqa: E731
    if dev == "cpu":
        assert fw is None and rows is None and dt == "f32"
        _lib.call("pg_spmm_max_bwd_cpu", fs, gt, aw.ptr, aw.ld, kind, dw.ptr, dw.ld, F, p(mw), ld(mw), xw.ptr, xw.ld)
        return
    ws_n = _lib.lib().pg_spmm_max_bwd_workspace(gt, F)
    ws = workspace(max(ws_n, 256), dev, ws_off)
    tail = (ws.data_ptr(), ws_n, _stream(dev))
    if rows is not None:
        tail = rows + tail
    _lib.call(entry + ("_bf16" if dt == "bf16" else ""), fs, gt, aw.ptr, aw.ld, kind, dw.ptr, dw.ld, F, p(mw), ld(mw),
              p(fw), ld(fw), xw.ptr, xw.ld, *tail)


def run_bwd(dev, F, dt, trans, weighted, mode, spec, name, i32=False, rows=False):
    """The backward on windows: dx bitwise the twin's, nothing outside its F columns written, a
    second call into a fresh buffer the same bits."""
    from plagnn import _lib

    dtype = DTYPES[dt]
    g = graph(trans, i32)
    dg = g.on(dev)
    kind = (I32 if i32 else U16) | (_lib.PG_ARG_DEAD_NONE if mode == "dead_none" else 0)
    aw, dw, mw, fw, ref, wd = bwd_operands(dev, F, dt, weighted, i32, mode, spec, rows)
    extra = None
    if rows:
        act = _t(rows_case(F, weighted)[0], dev)
        row_active = act.to(torch.int8)
        eslot_active = torch.where(act[dg.bwd.col.long()], dg.bwd.eslot, torch.full_like(dg.bwd.eslot, -1))
        extra = (row_active.data_ptr(), eslot_active.data_ptr())
    res = []
    for _ in range(2):
        xw = _out(g.num_src, F, dtype, dev, spec, "dx", NAN)
        bwd_call(dev, "pg_spmm_max_bwd_rows" if rows else "pg_spmm_max_bwd", g, dg, wd, F, dt, kind, aw, dw, mw, fw, xw,
                 spec["ws"], extra)
        res.append(xw)
    same(res[0].view, ref, f"{name}: dx")
    assert untouched(res[0]) and untouched(res[1]), f"{name}: written outside the F columns"
    assert torch.equal(res[0].bits(), res[1].bits()), f"{name}: second call"


def run_argsrc(dev, kind, F=65):
    """pg_argpos_to_src (dev "cpu": pg_argpos_to_src_cpu) on padded, odd, offset windows against
    col[ptr[v] + a], -1 for "none"."""
    from plagnn import _lib

    i32 = kind == I32
    arg = case(F, True, i32)[3]
    g = graph(False, i32)
    dg = g.on(dev)
    a = arg.astype(np.int64)
    none = a == ARG_NONE
    ref = np.where(none, -1, g.fwd.col[np.minimum(g.fwd.ptr[:-1, None] + np.where(none, 0, a), g.fwd.nnz - 1)])
    assert none.any() and not none.all()
    aw = _win(_t(arg, dev), F, ARGSRC_SPEC, "arg", ARG_NONE)
    res = []
    for _ in range(2):
        xw = _out(g.num_dst, F, torch.int64, dev, ARGSRC_SPEC, "argx", -7)
        tail = () if dev == "cpu" else (_stream(dev),)
        _lib.call("pg_argpos_to_src" + ("_cpu" if dev == "cpu" else ""), dg.fwd.struct(None), aw.ptr, aw.ld, kind, F,
                  xw.ptr, xw.ld, *tail)
        res.append(xw)
    assert np.array_equal(res[0].view.cpu().numpy(), ref), "source ids"
    assert untouched(res[0]) and untouched(res[1]), "written outside the F columns"
    assert torch.equal(res[0].bits(), res[1].bits()), "second call"
