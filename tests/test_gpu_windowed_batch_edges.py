"""GPU parity of the windowed kernels where a workgroup's windows span images.

Several windowed kernels put more than one window into a workgroup: win_rows1s x2 / x3,
win_rows and win_fused (four), win_strip / win_bwd_strip (eight), win_bwd_rows x2.  The
other parity files run images of 6 to 60 windows at B = 2 or 3, so a workgroup's windows
lie in one image, at most in two, and the last workgroup is full.  Here the images hold
one to five windows and the batch is 1, 2 or 7 (coprime to 2, 3, 4 and 8): workgroups
straddle two or three images, and the last one is ragged.  A second table runs the auto
rules' thresholds at the shapes tests/test_windowed_plan_host.py pins (one-window images,
batches of a few hundred).

Every call goes through the C ABI with y, l, m (dq, dk, dv) pre-filled with 777.0: a
fresh torch.empty often returns the block that held the previous mode's correct result, so
a window a kernel never stored would read as right.  The float64 oracle is
oracle/fa_oracle.py (windowed_fa, windowed_fa_backward) on the same bf16-representable
inputs, a different draw per image.  Each case asks the plan entries
(fa_debug_win_fwd_plan / fa_debug_win_bwd_plan) which kernel it ran; a failure names the
images that are wrong, so a pattern such as every third image shows."""
from __future__ import annotations

import ctypes
import zlib

import numpy as np
import pytest
import torch

from conftest import assert_close, assert_lm_close
from oracle import fa_oracle as O

pytestmark = pytest.mark.gpu

# (spatial, ws, stride, pad); S[0] % 8 == 0 and stride >= ws: the row-staged kernels apply
GEOMS = {
    "ONE7": ((8, 7), 7, 8, 0),      # 1 x 1 windows; stride != ws: never the strip kernel
    "ONE7S": ((8, 7), 7, 7, 0),     # 1 x 1; strip-eligible, first strip k0 = 8, the covered right end x = 7 inside a 16-B chunk
    "PAIRX": ((16, 7), 7, 8, 0),    # 2 x 1: triples straddle images, pairs do not
    "TRIPX": ((24, 7), 7, 8, 0),    # 3 x 1: pairs straddle, triples do not
    "PAIRY": ((8, 16), 7, 8, 0),    # 1 x 2: consecutive windows are vertical neighbours
    "QUAD5": ((8, 8), 5, 5, 1),     # 2 x 2: windows hang over both edges of an 8-wide image, the second shifts by 4 pixels
    "EDGE7": ((8, 7), 7, 7, 3),     # 2 x 1, pad 3; strip-eligible and aligned (k0 = 5, right end past the image)
    "TRI7S": ((16, 7), 7, 7, 3),    # 3 x 1; strip-eligible and aligned
    "ONE8": ((8, 8), 8, 8, 0),      # 1 x 1, ws 8: row scatter, one live wave of four in win_rows
    "PAIR8": ((16, 8), 8, 8, 0),    # 2 x 1
    "FIVE8": ((40, 8), 8, 8, 0),    # 5 x 1: the second four-window group holds one window
}
WS7 = ["ONE7", "ONE7S", "PAIRX", "TRIPX", "PAIRY", "QUAD5", "EDGE7", "TRI7S"]
WS8 = ["ONE8", "PAIR8", "FIVE8"]
BATCHES = (1, 2, 7)
DIMS = [(64, 64), (32, 64), (64, 32), (20, 48)]   # as tests/test_gpu_windowed_paths.py
FWD_MODES7 = (0, 1, 2, 3, 4, 6, 10, 12)           # fa_debug_set_win_composed (fa::WinMode)
FWD_MODES8 = (0, 1, 3, 4, 5)
BWD_MODES = (0, 1, 3, 10, 13)

DT = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
# backward: max|x - ref| / max(max|ref|, 1e-2), the rule and bounds of test_windowed_backward_strip_kernel,
# test_windowed_backward_paths (16-bit) and test_windowed_backward_f32_paths (fp32)
GTOL = {"bfloat16": 2e-2, "float16": 2e-2, "float32": 2e-5}

FWD_K = ("Composed", "Fused", "FusedWs", "Rows", "Rows1", "Shift1", "Shift2", "Shift3", "Shift128", "Strip", "F32")
BWD_K = ("Composed", "Rows1", "Rows2", "Rows128", "Strip", "StripPartial", "F32")
# pinned by hand from the dispatch rules (16-bit types): (geometry, mode) -> kernel
FWD_PINS = {("ONE7", 12): "Shift3", ("ONE7", 6): "Shift2", ("ONE7S", 10): "Strip"}
BWD_PINS = {("ONE7", 13): "Rows2", ("ONE7S", 10): "StripPartial", ("EDGE7", 10): "Strip"}


def bind_plans(L):
    """The plan entries' signatures, as tests/test_windowed_plan_host.py binds them."""
    i64, ci = ctypes.c_int64, ctypes.c_int
    geom = [ci, ci, ctypes.POINTER(i64), i64, i64, i64, i64, i64, i64]
    L.fa_debug_win_fwd_plan.restype = ci
    L.fa_debug_win_fwd_plan.argtypes = geom + [ci, ci, ci]
    L.fa_debug_win_bwd_plan.restype = ci
    L.fa_debug_win_bwd_plan.argtypes = geom + [ci, ci, ci, ci]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    bind_plans(fa_hip.lib())
    return fa_hip


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def variants(B):
    """(dtype, d, dv): bf16 at d = dv = 64 everywhere; at B = 7 every dtype and DIMS."""
    if B != 7:
        return [("bfloat16", 64, 64)]
    return [(dt, d, dv) for dt in DT for d, dv in DIMS]


def plan(fa, direction, geom, B, dtype, d, dv, mode, cus):
    """Name of the kernel the library plans for this call (pointers 16-B aligned, as torch's are)."""
    S, ws, st, pad = geom
    args = (CODE[dtype], len(S), (ctypes.c_int64 * len(S))(*S), d, dv, B, ws, st, pad, mode, 1, 1)
    if direction == "fwd":
        return FWD_K[fa.lib().fa_debug_win_fwd_plan(*args)]
    return BWD_K[fa.lib().fa_debug_win_bwd_plan(*args, cus)]


class Case:
    """Inputs (device and float64), the oracle's results and the auto-mode forward of one shape."""

    def __init__(self, fa, geom, B, dtype, d, dv):
        self.fa, self.geom, self.B, self.dtype, self.d, self.dv = fa, geom, B, dtype, d, dv
        S, ws, st, pad = geom
        rng = np.random.default_rng(zlib.crc32(repr((geom, B, dtype, d, dv)).encode()))

        def draw(c):   # seeded standard_normal rounded to bf16, every image its own draw
            a = torch.tensor(rng.standard_normal(S + (c, B))).to(torch.bfloat16)
            t = fa.jl_tensor(a, DT[dtype])
            return t, _np(t)

        (self.Q, self.q), (self.K, self.k) = draw(d), draw(d)
        (self.V, self.v), (self.DY, self.dy) = draw(dv), draw(dv)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.fwd_ref = O.windowed_fa(self.q, self.k, self.v, ws, st, pad)
        self._bwd_ref = self._auto = None

    @property
    def bwd_ref(self):
        if self._bwd_ref is None:
            S, ws, st, pad = self.geom
            self._bwd_ref = O.windowed_fa_backward(self.q, self.k, self.v, self.dy, ws, st, pad)
        return self._bwd_ref

    @property
    def auto_forward(self):
        if self._auto is None:
            self._auto = forward(self, 0)
        return self._auto


_CASES = {}


def case(fa, name, B, dtype, d, dv):
    """The matrix's shapes are shared between the modes: one draw, one oracle call."""
    key = (name, B, dtype, d, dv)
    if key not in _CASES:
        _CASES[key] = Case(fa, GEOMS[name], B, dtype, d, dv)
    return _CASES[key]


def _abi_args(c):
    S, ws, st, pad = c.geom
    return len(S), (ctypes.c_int64 * len(S))(*S), c.d, c.dv, c.B, ws, st, pad


def _poisoned(fa, shape, dtype):
    return fa.jl_empty(shape, dtype).fill_(777.0)


def forward(c, mode):
    """fa_windowed_fwd through ctypes under a forced mode, into outputs pre-filled with 777.0."""
    fa, L = c.fa, c.fa.lib()
    S, ws, st, pad = c.geom
    T, nwin = ws ** len(S), int(np.prod(O.window_geometry(S, ws, st, pad)))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    y = _poisoned(fa, S + (c.dv, c.B), DT[c.dtype])
    l, m = (_poisoned(fa, (T, 1, nwin, c.B), torch.float32) for _ in range(2))
    old = L.fa_debug_set_win_composed(mode)
    try:
        nws = L.fa_windowed_fwd_workspace(CODE[c.dtype], *_abi_args(c))
        ws_buf = torch.empty(nws + 1, dtype=torch.uint8, device="cuda")
        rc = L.fa_windowed_fwd(CODE[c.dtype], P(c.Q), P(c.K), P(c.V), P(y), P(l), P(m), *_abi_args(c), 0.0,
                               P(ws_buf), nws, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_last_error()
        torch.cuda.synchronize()
    finally:
        L.fa_debug_set_win_composed(old)
    return y, l, m


def backward(c, mode):
    """fa_windowed_bwd through ctypes under a forced mode, on the auto-mode forward's y, l, m."""
    fa, L = c.fa, c.fa.lib()
    S = c.geom[0]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    y, l, m = c.auto_forward
    dq, dk = (_poisoned(fa, S + (c.d, c.B), DT[c.dtype]) for _ in range(2))
    dv = _poisoned(fa, S + (c.dv, c.B), DT[c.dtype])
    old = L.fa_debug_set_win_composed(mode)
    try:
        nws = L.fa_windowed_workspace(CODE[c.dtype], *_abi_args(c))
        ws_buf = torch.empty(nws + 1, dtype=torch.uint8, device="cuda")
        rc = L.fa_windowed_bwd(CODE[c.dtype], P(c.Q), P(c.K), P(c.V), P(y), P(c.DY), P(l), P(m), P(dq), P(dk), P(dv),
                               *_abi_args(c), 0.0, P(ws_buf), nws,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_last_error()
        torch.cuda.synchronize()
    finally:
        L.fa_debug_set_win_composed(old)
    return dq, dk, dv


def _images(bad, B):
    bad = [int(b) for b in bad]
    head = ", ".join(map(str, bad[:16])) + (", ..." if len(bad) > 16 else "")
    return f"{len(bad)} of {B} images wrong: b = {head}; their b mod 3: {sorted({b % 3 for b in bad})}"


def _no_fill_left(outs, names, B, tag):
    for nm, t in zip(names, outs):
        left = (t == torch.tensor(777.0, dtype=t.dtype, device=t.device)).flatten(0, -2).any(0)
        assert not bool(left.any()), f"{tag} {nm}: the 777.0 fill is left; {_images(torch.nonzero(left)[:, 0].tolist(), B)}"


def _per_image(check, x, ref, B):
    """check(x, ref) on the whole batch; when it fails, say which images fail on their own."""
    try:
        check(x, ref)
    except AssertionError as e:
        bad = []
        for b in range(B):
            try:
                check(x[..., b:b + 1], ref[..., b:b + 1])
            except AssertionError:
                bad.append(b)
        raise AssertionError(f"{e}; {_images(bad, B)}") from None


def check_forward(c, outs, tag):
    _no_fill_left(outs, ("y", "l", "m"), c.B, tag)
    y, l, m = (_np(t) for t in outs)
    yr, lr, mr = c.fwd_ref
    _per_image(lambda a, r: assert_close(a, r, c.dtype, f"{tag} y", nan_ok=True), y, yr, c.B)
    _per_image(lambda a, r: assert_lm_close(a, r, c.dtype, f"{tag} l"), l, lr, c.B)
    _per_image(lambda a, r: assert_lm_close(a, r, c.dtype, f"{tag} m"), m, mr, c.B)


def check_backward(c, grads, tag):
    _no_fill_left(grads, ("dq", "dk", "dv"), c.B, tag)
    for t, r, nm in zip(grads, c.bwd_ref, ("dq", "dk", "dv")):
        x = _np(t)
        scale = max(np.abs(r).max(), 1e-2)
        with np.errstate(invalid="ignore"):
            err = np.abs(x - r).reshape(-1, c.B).max(0) / scale     # per image, on the batch's scale
        err = np.where(np.isfinite(err), err, np.inf)              # a non-finite gradient fails its image
        bad = np.nonzero(err > GTOL[c.dtype])[0]
        assert bad.size == 0, (f"{tag} {nm}: worst image {int(err.argmax())} err {err.max():.2e} > "
                               f"{GTOL[c.dtype]:.0e}; {_images(bad, c.B)}")


FWD_MATRIX = ([(n, B, md) for n in WS7 for B in BATCHES for md in FWD_MODES7] +
              [(n, B, md) for n in WS8 for B in BATCHES for md in FWD_MODES8])
BWD_MATRIX = [(n, B, md) for n in WS7 for B in BATCHES for md in BWD_MODES]
_ids = lambda row: "{}-B{}-mode{}".format(*row)


@pytest.mark.parametrize("name,B,mode", FWD_MATRIX, ids=[_ids(r) for r in FWD_MATRIX])
def test_forward_batch_edges(fa, cus, name, B, mode):
    for dtype, d, dv in variants(B):
        c = case(fa, name, B, dtype, d, dv)
        kern = plan(fa, "fwd", c.geom, B, dtype, d, dv, mode, cus)
        if (name, mode) in FWD_PINS and dtype != "float32":
            assert kern == FWD_PINS[(name, mode)], f"{name} x {B} mode {mode} {dtype}: planned {kern}"
        check_forward(c, forward(c, mode), f"{name} x {B} mode {mode} [{kern}] {dtype} d {d} dv {dv}:")


@pytest.mark.parametrize("name,B,mode", BWD_MATRIX, ids=[_ids(r) for r in BWD_MATRIX])
def test_backward_batch_edges(fa, cus, name, B, mode):
    for dtype, d, dv in variants(B):
        c = case(fa, name, B, dtype, d, dv)
        kern = plan(fa, "bwd", c.geom, B, dtype, d, dv, mode, cus)
        if (name, mode) in BWD_PINS and dtype != "float32":
            assert kern == BWD_PINS[(name, mode)], f"{name} x {B} mode {mode} {dtype}: planned {kern}"
        check_backward(c, backward(c, mode), f"{name} x {B} mode {mode} [{kern}] {dtype} d {d} dv {dv}:")


def test_matrix_reaches_every_multi_window_kernel(fa, cus):
    """The two matrices above, asked of the plan entries alone: every kernel that puts
    windows of several images into a workgroup (and the one-window and composed ones
    they are compared with) is reached by some case.  Prints mode -> kernels."""
    reached = {"fwd": {}, "bwd": {}}
    for direction, matrix in (("fwd", FWD_MATRIX), ("bwd", BWD_MATRIX)):
        for name, B, mode in matrix:
            for dtype, d, dv in variants(B):
                reached[direction].setdefault(mode, set()).add(plan(fa, direction, GEOMS[name], B, dtype, d, dv, mode, cus))
    for direction, by_mode in reached.items():
        for mode in sorted(by_mode):
            print(f"{direction} mode {mode}: {', '.join(sorted(by_mode[mode]))}")
    fwd, bwd = set().union(*reached["fwd"].values()), set().union(*reached["bwd"].values())
    assert fwd >= {"Fused", "Rows", "Rows1", "Shift1", "Shift2", "Shift3", "Strip", "Composed", "F32"}, fwd
    assert bwd >= {"Rows1", "Rows2", "Strip", "StripPartial", "Composed", "F32"}, bwd


# The auto rules' thresholds at the host table's own shapes (bf16, d = dv = 64, mode 0); the
# kernel of each row is pinned by hand for 256 CUs (kRows3Min 600 / kRows3Max 1000,
# kRows4Min 1024, kStripMin / kStripBwdMin 256, kBwdPairMaxPerCu 1.5).
FWD_THRESHOLDS = [
    ("ONE7", 599, "Shift2"),
    ("ONE7", 600, "Shift3"),
    ("ONE7", 999, "Shift3"),
    ("PAIRX", 300, "Shift3"),
    ("ONE8", 1023, "Rows1"),
    ("ONE8", 1024, "Rows"),
    ("ONE7S", 255, "Shift2"),
    ("ONE7S", 256, "Strip"),
]
# batches as functions of the CU count: the pair rule is per CU, and the strip backward runs
# one workgroup per CU, so "one more strip than workgroups" follows the device too
BWD_THRESHOLDS = [
    ("ONE7", "1.5 CUs", lambda n: int(1.5 * n), "Rows2"),
    ("ONE7", "1.5 CUs + 1", lambda n: int(1.5 * n) + 1, "Rows1"),
    ("ONE7S", "kStripBwdMin", lambda n: 256, "StripPartial"),
    ("ONE7S", "CUs + 1", lambda n: max(n, 256) + 1, "StripPartial"),   # the dynamic deal draws exactly one strip
    ("EDGE7", "kStripBwdMin", lambda n: 256, "Strip"),
]


@pytest.mark.parametrize("name,B,want", FWD_THRESHOLDS, ids=[f"{n}-B{B}-{k}" for n, B, k in FWD_THRESHOLDS])
def test_forward_auto_thresholds(fa, cus, name, B, want):
    c = Case(fa, GEOMS[name], B, "bfloat16", 64, 64)
    kern = plan(fa, "fwd", c.geom, B, "bfloat16", 64, 64, 0, cus)
    assert kern == want, f"{name} x {B}: planned {kern}"
    check_forward(c, forward(c, 0), f"{name} x {B} auto [{kern}]:")


@pytest.mark.parametrize("name,what,batch,want", BWD_THRESHOLDS, ids=[f"{r[0]}-{r[1]}-{r[3]}" for r in BWD_THRESHOLDS])
def test_backward_auto_thresholds(fa, cus, name, what, batch, want):
    B = batch(cus)
    if cus != 256:
        print(f"the device reports {cus} CUs, not 256: B = {what} = {B} derived from it (256 CUs: {batch(256)})")
    c = Case(fa, GEOMS[name], B, "bfloat16", 64, 64)
    kern = plan(fa, "bwd", c.geom, B, "bfloat16", 64, 64, 0, cus)
    assert kern == want, f"{name} x {B}: planned {kern}"
    check_backward(c, backward(c, 0), f"{name} x {B} auto [{kern}]:")
