"""GPU tests of the cache writers (fa_hip.paged_kv_append_, paged_kv_append_fp8_, quantize_kv_fp8_hip)
against a CPU scatter written with plain indexing, and for fp8 quantize_kv_fp8's own expression on
the CPU.  Everything is compared bit for bit: whole pools as int16 / uint8, so a wrong row, a wrong
page, an unwritten element and a clobbered neighbour all show."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
SCALES = [0.37, 1.0, 2.5, 0.011]


@pytest.fixture(scope="module")
def fa():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    fa_hip.lib()
    return fa_hip


def lengths(case, ps):
    """(N, max_pages, q_lens, k_lens) of four slabs; lengths past N / cap are clamped by the kernel."""
    if case == "decode":      # N = 1 at a page's first, last and a middle row; nq = 0
        return 1, 3, [1, 1, 1, 0], [ps + 1, 2 * ps, ps + ps // 2 + 1, 5]
    if case == "short":       # rows 2..4 of one chunk; from position 0; nk < nq; both lengths clamped
        return 3, 2, [3, 3, 3, 9], [5, 3, 2, 2 * ps + 7]
    if case == "ragged":      # mid-chunk start, page boundaries crossed, mid-chunk end; from 0; nq = 0; a shorter run
        mp = 37 // ps + 3
        return 37, mp, [37, 37, 0, 20], [ps - 3 + 37, 37, 11, 2 * ps + 5]
    return 2 * ps, 2, None, None   # "full": NULL lengths with N == cap


def to_fp8(x, s):
    return (x.float() / torch.tensor(s, dtype=torch.float32)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def ref_scatter(kp, vp, table, kn, vn, ql, kl, ks=None, vs=None):
    """The append on CPU pools (int16 views of 16-bit pools, or uint8 pools with scales), in place."""
    ps, P, N, B = kp.shape[0], kp.shape[2], kn.shape[0], kn.shape[2]
    cap = table.shape[0] * ps
    for b in range(B):
        nq = N if ql is None else min(max(ql[b], 0), N)
        nk = cap if kl is None else min(max(kl[b], 0), cap)
        for i in range(nq):
            j = nk - nq + i
            if j < 0:
                continue
            page = min(max(int(table[j // ps, b]), 0), P - 1)
            for pool, new, sc in ((kp, kn, ks), (vp, vn, vs)):
                pool[j % ps, :, page] = new[i, :, b].view(torch.int16) if sc is None else to_fp8(new[i, :, b], sc[b])
    return kp, vp


def offset_tensor(fa, x, off):
    """x on the device, column-major, starting `off` elements into its allocation."""
    flat = torch.empty(x.numel() + off, dtype=x.dtype, device="cuda")
    t = flat[off:].as_strided(x.shape, fa.jl_strides(x.shape))
    t.copy_(x)
    return t


def pool_case(dtype, fp8, ps, d, dv, case):
    g = torch.Generator().manual_seed(1000 * ps + d + len(case))
    N, mp, ql, kl = lengths(case, ps)
    B, P = 4, 4 * mp + 3
    pdt, lo, hi = (torch.uint8, 0, 256) if fp8 else (torch.int16, -32768, 32768)    # every bit pattern, NaNs included
    kp, vp = (torch.randint(lo, hi, (ps, n, P), generator=g, dtype=pdt) for n in (d, dv))
    if fp8:
        kp[0, 0, :], vp[-1, -1, :] = 0x7F, 0xFF
    kn, vn = ((3 * torch.randn(N, n, B, generator=g)).to(DT[dtype]) for n in (d, dv))
    table = torch.randint(-10 ** 6, 10 ** 6, (mp, B), generator=g, dtype=torch.int32)  # garbage past the used pages
    perm = 1 + torch.randperm(P - 2, generator=g)
    for b in range(B):
        used = mp if kl is None else min(mp, -(-max(kl[b], 0) // ps))
        table[:used, b] = perm[b * mp:b * mp + used].int()
    table[0, 0], table[0, 1] = -5, P + 7                      # out of range inside the used pages: pages 0 and P - 1
    sc = (SCALES, SCALES[::-1]) if fp8 else (None, None)
    rk, rv = ref_scatter(kp.clone(), vp.clone(), table, kn, vn, ql, kl, *sc)
    return kp, vp, kn, vn, table, ql, kl, rk, rv


@pytest.mark.parametrize("case", ["decode", "short", "ragged", "full"])
@pytest.mark.parametrize("d,dv", [(128, 128), (40, 72)])
@pytest.mark.parametrize("fp8,ps", [(False, 8), (False, 24), (False, 64), (True, 16), (True, 48), (True, 64)])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_whole_pools_bitwise(fa, dtype, fp8, ps, d, dv, case):
    kp, vp, kn, vn, table, ql, kl, rk, rv = pool_case(dtype, fp8, ps, d, dv, case)
    dev = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device="cuda")
    KN, VN, T = offset_tensor(fa, kn, 1), offset_tensor(fa, vn, 3), fa.jl_tensor(table, torch.int32)
    runs = []
    for _ in range(2):
        KP, VP = (fa.jl_tensor(p, p.dtype) for p in (kp, vp))
        if fp8:
            ks, vs = (torch.tensor(s, device="cuda") for s in (SCALES, SCALES[::-1]))
            fa.paged_kv_append_fp8_(KP, VP, T, KN, VN, ks, vs, dev(kl), dev(ql))
        else:
            fa.paged_kv_append_(KP.view(DT[dtype]), VP.view(DT[dtype]), T, KN, VN, dev(kl), dev(ql))
        runs.append((KP.cpu(), VP.cpu()))
    for got, ref in zip(runs[0], (rk, rv)):
        bad = (got != ref).nonzero()
        assert bad.numel() == 0, f"{len(bad)} elements differ, first (row, feature, page) {bad[0].tolist()}"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # two runs, the same bits


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_every_finite_16_bit_pattern(fa, dtype, scale):
    """Ties, subnormals, -0 and saturation: each of the 65536 patterns once (NaN -> 0, +-Inf kept)."""
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(DT[dtype])
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    kn = x[torch.randperm(65536, generator=torch.Generator().manual_seed(1))].reshape(1, 128, 512).permute(2, 1, 0)
    vn = x.reshape(1, 128, 512).permute(2, 1, 0)
    table = torch.arange(8, dtype=torch.int32).flip(0).reshape(8, 1)
    rk, rv = ref_scatter(torch.zeros(64, 128, 8, dtype=torch.uint8), torch.zeros(64, 128, 8, dtype=torch.uint8), table,
                         kn, vn, None, None, [scale], [scale])
    KP, VP = (fa.jl_tensor(torch.full((64, 128, 8), 0x7F, dtype=torch.uint8), torch.uint8) for _ in range(2))
    s = None if scale == 1.0 else torch.tensor([scale], device="cuda")
    fa.paged_kv_append_fp8_(KP, VP, table.cuda(), fa.jl_tensor(kn, DT[dtype]), fa.jl_tensor(vn, DT[dtype]), s, s)
    for got, ref in ((KP, rk), (VP, rv)):
        bad = (got.cpu() != ref).nonzero()
        assert bad.numel() == 0, f"{len(bad)} bytes differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_chunked_appends_rebuild_the_cache(fa, dtype):
    g = torch.Generator().manual_seed(7)
    Nk, d, dv, B, ps, mp = 100, 64, 40, 3, 16, 7
    K, V = (torch.randn(Nk, n, B, generator=g).to(DT[dtype]) for n in (d, dv))
    final, P = [100, 77, 30], 3 * 7
    table = torch.randperm(P, generator=g).int().reshape(B, mp).t().contiguous()
    KP, VP = (fa.jl_tensor(torch.randn(ps, n, P, generator=g), DT[dtype]) for n in (d, dv))
    rk, rv = KP.cpu().view(torch.int16), VP.cpu().view(torch.int16)
    T, done, cum = fa.jl_tensor(table, torch.int32), [0] * B, 0
    for N in (41, 1, 58):                                 # the decode path in the middle
        cum += N
        kl = [min(f, cum) for f in final]
        ql = [a - b for a, b in zip(kl, done)]
        kn, vn = (torch.zeros(N, X.shape[1], B, dtype=DT[dtype]) for X in (K, V))
        for b in range(B):
            kn[:ql[b], :, b], vn[:ql[b], :, b] = K[done[b]:kl[b], :, b], V[done[b]:kl[b], :, b]
        lens = [torch.tensor(x, dtype=torch.int32, device="cuda") for x in (kl, ql)]
        fa.paged_kv_append_(KP, VP, T, fa.jl_tensor(kn, DT[dtype]), fa.jl_tensor(vn, DT[dtype]), *lens)
        ref_scatter(rk, rv, table, kn, vn, ql, kl)
        done = kl
    GK, GV = fa.paged_kv_gather(KP, VP, T)
    for b in range(B):
        assert torch.equal(GK[:final[b], :, b].cpu().view(torch.int16), K[:final[b], :, b].view(torch.int16))
        assert torch.equal(GV[:final[b], :, b].cpu().view(torch.int16), V[:final[b], :, b].view(torch.int16))
    Q = fa.jl_tensor(torch.randn(58, d, B, generator=g), DT[dtype])
    RK, RV = (fa.jl_tensor(r, torch.int16).view(DT[dtype]) for r in (rk, rv))
    for a, r in zip(fa.paged_prefill_fa(Q, KP, VP, T, *lens), fa.paged_prefill_fa(Q, RK, RV, T, *lens)):
        assert torch.equal(a.view(torch.int16 if a.dtype != torch.float32 else torch.int32),
                           r.view(torch.int16 if r.dtype != torch.float32 else torch.int32))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_quantize_kv_fp8_hip(fa, dtype):
    """Nk % 8 != 0; 333 * 128 elements are three spans of maxima; a zero slab; a maximum in the last element."""
    g = torch.Generator().manual_seed(3)
    k, v = (torch.randn(333, n, 3, generator=g).to(DT[dtype]) for n in (128, 72))
    k[:, :, 0], v[:, :, 0] = 0, 0
    k[-1, -1, 2], v[-1, -1, 2] = 9.5, -7.25
    got = fa.quantize_kv_fp8_hip(fa.jl_tensor(k, DT[dtype]), fa.jl_tensor(v, DT[dtype]))
    ref = fa.quantize_kv_fp8(k, v)
    assert ref[2][0] == 1.0 and k[:, :, 2].abs().max() == 9.5 and v[:, :, 2].abs().max() == 7.25
    for a, r in zip(got, ref):
        bits = torch.uint8 if r.dtype == torch.float8_e4m3fn else torch.int32
        assert torch.equal(a.cpu().view(bits), r.view(bits))
