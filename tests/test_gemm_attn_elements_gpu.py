"""ln3d_gemm_bf16 and ln3d_attention_bf16 per element: exact where the result does not depend on the summation order (integer operands,
one-hot and uniform softmax), otherwise within the float64 bounds of tests/kernel_refs.py (GEMM: c fp32 ulps of the summed magnitudes /
1 bf16 ulp; attention: 2^-8 sum p |v| + 1 bf16 ulp), under every GEMM tile configuration and on every path of the attention dispatcher.
The bounds are derived or measured from CPU restatements (tests/test_gemm_attn_refs_cpu.py), never from the kernels' output."""
import functools
import math
import os

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = kr.GEMM_F32_ULPS
BF = torch.bfloat16
SENT = -3.0                                   # bf16 / fp32 sentinel in positions a kernel must not write
TILES = ["auto", "s", "x7", "x8", "x9", "x12", "x13", "x14", "x16"]


@pytest.fixture(scope="module", params=TILES)
def tile(hip_lib, request):
    """(ops, name): the GEMM tile selection left to the library and forced to each configuration; LN3D_GEMM_TILE is restored on exit."""
    from ln3diff_amd import ops as o
    old = os.environ.get("LN3D_GEMM_TILE")
    if request.param == "auto":
        os.environ.pop("LN3D_GEMM_TILE", None)
    else:
        os.environ["LN3D_GEMM_TILE"] = request.param
    o.reload_env()
    yield o, request.param
    if old is None:
        os.environ.pop("LN3D_GEMM_TILE", None)
    else:
        os.environ["LN3D_GEMM_TILE"] = old
    o.reload_env()


@pytest.fixture
def ops(hip_lib):
    from ln3diff_amd import ops as o
    return o


def test_epilogue_numbers(ops):
    assert (ops.EPI_F32, ops.EPI_BF16, ops.EPI_GELU_ERF, ops.EPI_GELU_TANH, ops.EPI_SILU, ops.EPI_GATE_RES, ops.EPI_HEADS, ops.EPI_F32_SILU,
            ops.EPI_QUICK_GELU, ops.EPI_CROSS_ATTN) == tuple(range(10))


def _full(shape, dtype, value=float("nan")):
    return torch.full(shape, value, device=DEV, dtype=dtype)


def _eq(y, ref64, what):
    """every element of y equals ref64 (double); names the first that does not"""
    yd = y.detach().double().cpu().reshape(-1)
    rd = ref64.reshape(-1)
    assert yd.numel() == rd.numel(), (what, yd.numel(), rd.numel())
    bad = ~(yd == rd)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {yd.numel()} elements differ; first at flat index {i}: got {float(yd[i])!r}, expected {float(rd[i])!r}")


# ================================================================ integer GEMM: exact under any summation order
@functools.lru_cache(maxsize=None)
def _int_case(M, N, K):
    g = torch.Generator().manual_seed(77 * M + 13 * N + K)
    x = torch.randint(-8, 9, (M, K), generator=g)
    w = torch.randint(-8, 9, (N, K), generator=g)
    b = torch.randint(-64, 65, (N,), generator=g)
    return x, w, b, (x @ w.t() + b).double()                  # int64 products and sums: |.| <= 64 K + 64 < 2^24


def _int_gate(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    rows = max(1, M // 2)
    ns = (M + rows - 1) // rows
    gate = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])[torch.randint(0, 6, (ns, N), generator=g)]
    res = torch.randint(-500, 501, (M, N), generator=g).float()
    rb = torch.randint(-100, 101, (ns, N), generator=g).float()
    return rows, gate, res, rb


@pytest.mark.parametrize("shape", range(4))
def test_gemm_integer_exact(tile, shape):
    """x, w in {-8 .. 8}, integer bias: every product and partial sum is an integer below 2^24, so F32 must equal the int64 result and
    BF16 its rounding, at one row, one short of a tile, one past it (2 x 2 ragged tiles) and two token tiles less a row, with fewer K
    stages than the ring is deep (K = 64), a few (192) and many (1024).  GATE_RES with gates +-1, +-2, +-0.5 per sample, integer residual
    and per-sample row is exact in both outputs; the activation epilogues keep sign and zero."""
    ops, name = tile
    M, N = kr.gemm_shapes(*kr.TILE_SHAPE[name])[shape]
    for K in (64, 192, 1024):
        x, w, b, ref = _int_case(M, N, K)
        xb, wb, bd = x.to(DEV, BF), w.to(DEV, BF), b.float().to(DEV)
        what = f"{name} integer {M}x{N}x{K}"
        y = _full((M, N), torch.float32)
        ops.gemm(xb, wb, bd, ops.EPI_F32, y)
        _eq(y, ref, what + " F32")
        y16 = _full((M, N), BF)
        ops.gemm(xb, wb, bd, ops.EPI_BF16, y16)
        _eq(y16, kr.bf16_rne(ref), what + " BF16")
        ops.gemm(xb, wb, None, ops.EPI_F32, y)
        _eq(y, ref - b.double(), what + " F32 without bias")
        rows, gate, res, rb = _int_gate(M, N, M + K)
        gfull = torch.cat([torch.zeros_like(gate), gate], 1).to(DEV)           # the gate is a column slice of a wider matrix
        acc, copy = res.to(DEV).clone(), _full((M, N), BF)
        ops.gemm(xb, wb, bd, ops.EPI_GATE_RES, acc, copy, gate=gfull[:, N:], gate_rows=rows, gate_ld=2 * N, res_bias=rb.to(DEV), res_bias_ld=N)
        gref = res.double() + gate.double().repeat_interleave(rows, 0)[:M] * ref + rb.double().repeat_interleave(rows, 0)[:M]
        _eq(acc, gref, what + " GATE_RES out0")
        _eq(copy, kr.bf16_rne(gref), what + " GATE_RES out1")
        o32 = _full((M, N), torch.float32)
        for epi in (ops.EPI_GELU_ERF, ops.EPI_GELU_TANH, ops.EPI_SILU, ops.EPI_QUICK_GELU, ops.EPI_F32_SILU):
            y16 = _full((M, N), BF)
            if epi == ops.EPI_F32_SILU:
                ops.gemm(xb, wb, bd, epi, o32, y16)
                _eq(o32, ref, what + " F32_SILU out0")
            else:
                ops.gemm(xb, wb, bd, epi, y16)
            yd = y16.double().cpu()
            ok = torch.where(ref == 0, yd == 0, torch.where(ref > 0, yd > 0, (yd <= 0) & ((ref < -4) | (yd < 0))))
            assert bool(ok.all()), f"{what} epilogue {epi}: sign / zero pattern wrong at flat index {int((~ok).reshape(-1).nonzero()[0])}"


@pytest.mark.parametrize("shape", [2, 3])
def test_gemm_integer_exact_with_row_strides(tile, shape):
    """ldx = K + 8, ldw = K + 16, ldo = N + 12 through column-slice views: the gap columns of x and w hold NaN (one read of them poisons
    the sum), the gap columns of the NaN-filled output stay untouched."""
    ops, name = tile
    M, N = kr.gemm_shapes(*kr.TILE_SHAPE[name])[shape]
    for K in (64, 192):
        x, w, b, ref = _int_case(M, N, K)
        xw, ww = _full((M, K + 8), BF), _full((N, K + 16), BF)
        xw[:, :K], ww[:, :K] = x.to(DEV, BF), w.to(DEV, BF)
        bd = b.float().to(DEV)
        for epi, dt in ((ops.EPI_F32, torch.float32), (ops.EPI_BF16, BF)):
            out = _full((M, N + 12), dt)
            ops.gemm(xw[:, :K], ww[:, :K], bd, epi, out[:, :N], ldo=N + 12)
            what = f"{name} strided {M}x{N}x{K} epilogue {epi}"
            _eq(out[:, :N], ref if dt == torch.float32 else kr.bf16_rne(ref), what)
            assert bool(torch.isnan(out[:, N:]).all()), what + ": gap columns of the output written"


HEAD_SPLITS = [(64, 64, 2), (72, 128, 8), (72, 80, 8), (80, 80, 4), (32, 64, 4), (40, 64, 8), (128, 128, 1)]       # head_dim, head_dim_pad (attn_head_pad), heads


@pytest.mark.parametrize("tokens", [96, 77])
@pytest.mark.parametrize("Dh,Dp,H", HEAD_SPLITS)
def test_gemm_heads_split_integer_exact(tile, Dh, Dp, H, tokens):
    """HEADS with integer operands: q, k and the key-permuted V^T equal the rounded int64 result at the position heads_split_ref gives;
    padding rows and columns keep the sentinel.  tokens = 96 takes the staged head-aware epilogue on the ring tiles, tokens = 77 (into
    128 padded rows) the direct stores."""
    ops, name = tile
    B, tp = 2, 128
    M, N = B * tokens, 3 * H * Dh
    shapes, which, index, untouched = kr.heads_split_ref(M, N, tokens, tp, H, Dh, Dp, 0b100)
    for K in (64, 192):
        x, w, b, ref = _int_case(M, N, K)
        outs = [_full(s, BF, SENT) for s in shapes]
        ops.gemm(x.to(DEV, BF), w.to(DEV, BF), b.float().to(DEV), ops.EPI_HEADS, *outs, M=M, tokens=tokens, tok_pad=tp, heads=H, head_dim=Dh,
                 transpose_mask=0b100, head_dim_pad=Dp)
        want = kr.bf16_rne(ref)
        for wi, out in enumerate(outs):
            flat = out.double().cpu().reshape(-1)
            cols = which == wi
            _eq(flat[index[:, cols].reshape(-1)], want[:, cols], f"{name} HEADS {Dh}->{Dp} tokens {tokens} K {K} out{wi}")
            assert bool((flat[untouched[wi]] == SENT).all()), f"{name} HEADS {Dh}->{Dp} tokens {tokens} K {K} out{wi}: padding written"


# ================================================================ random GEMM against float64
@functools.lru_cache(maxsize=None)
def _rand_case(M, N, K):
    x, w, b = kr.gemm_inputs(M, N, K)
    return x, w, b, kr.gemm_lin(x, w, b)


def _check_epilogues(ops, M, N, K, what):
    x, w, b, lin = _rand_case(M, N, K)
    xb, wb, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    c = kr.gemm_ulps(K)
    y = _full((M, N), torch.float32)
    ops.gemm(xb, wb, bd, ops.EPI_F32, y)
    kr.assert_f32_close(y, lin[0], lin[1], c, what=what + " F32")
    for epi in (ops.EPI_BF16, ops.EPI_GELU_ERF, ops.EPI_GELU_TANH, ops.EPI_SILU, ops.EPI_QUICK_GELU, ops.EPI_F32_SILU):
        y16 = _full((M, N), BF)
        if epi == ops.EPI_F32_SILU:
            y.fill_(float("nan"))
            ops.gemm(xb, wb, bd, epi, y, y16)
            kr.assert_f32_close(y, lin[0], lin[1], c, what=what + " F32_SILU out0")
        else:
            ops.gemm(xb, wb, bd, epi, y16)
        ref, scale = kr.gemm_ref(x, w, b, epi, lin=lin)
        if epi == ops.EPI_GELU_ERF:
            kr.assert_bf16_close_abs(y16, ref, scale, c, kr.GELU_ERF_ABS, what=what + " GELU_ERF")
        elif epi == ops.EPI_GELU_TANH:
            # 0.5 x (1 + tanh(.)) cancels for x << 0: the fp32 formula itself is then off the correctly rounded value (shown on the CPU in
            # tests/test_gemm_attn_refs_cpu.py), inside the fp32 term of the bound.  The mismatch fraction is taken where the bound is the
            # bf16 ulp, where only near-ties can flip (at least two thirds of the elements at every shape: the CPU file checks that
            # too); the other elements are held to the per-element bound alone.
            over = kr.ulp_dominated(ref, scale, c)
            assert float(over.double().mean()) >= 2.0 / 3.0, f"{what} GELU_TANH: the mismatch fraction would cover {float(over.double().mean()):.2f} of the elements"
            kr.assert_bf16_close(y16, ref, scale, floor_ulps=c, max_mismatch=0.01, what=what + " GELU_TANH", flips_over=over)
        else:
            kr.assert_bf16_close(y16, ref, scale, floor_ulps=c, max_mismatch=0.01, what=f"{what} epilogue {epi}")
    g = torch.Generator().manual_seed(M + N + K)
    rows = max(1, M // 2)
    ns = (M + rows - 1) // rows
    gate, res, rb = torch.randn(ns, N, generator=g), torch.randn(M, N, generator=g), torch.randn(ns, N, generator=g)
    ref, scale = kr.gemm_ref(x, w, b, kr.EPI_GATE_RES, gate=gate, gate_rows=rows, res=res, res_bias=rb, lin=lin)
    acc, copy = res.to(DEV).clone(), _full((M, N), BF)
    ops.gemm(xb, wb, bd, ops.EPI_GATE_RES, acc, copy, gate=gate.to(DEV), gate_rows=rows, gate_ld=N, res_bias=rb.to(DEV), res_bias_ld=N)
    kr.assert_f32_close(acc, ref, scale, c, what=what + " GATE_RES out0")
    kr.assert_bf16_close(copy, ref, scale, floor_ulps=c, max_mismatch=0.01, what=what + " GATE_RES out1")


@pytest.mark.parametrize("shape", range(4))
def test_gemm_epilogues_float64(tile, shape):
    """Every epilogue on random asymmetric operands at the ragged shapes of the forced tile, K = 64 / 320 / 1024: fp32 outputs within c
    fp32 ulps of sum |x w| + |b|, bf16 outputs within 1 bf16 ulp (or that term) with at most 1 % off the correctly rounded value, the
    erf-GELU polynomial's 1.5e-4 added."""
    ops, name = tile
    M, N = kr.gemm_shapes(*kr.TILE_SHAPE[name])[shape]
    for K in (64, 320, 1024):
        _check_epilogues(ops, M, N, K, f"{name} {M}x{N}x{K}")


def test_gemm_persistent_kernel_interior_tiles(ops, monkeypatch):
    """cfg 16 at (512, 512, 512): four interior 256 x 256 tiles on the persistent kernel (BF16, GELU_ERF; the other epilogues take its
    non-persistent form)."""
    monkeypatch.setenv("LN3D_GEMM_TILE", "x16")
    ops.reload_env()
    try:
        _check_epilogues(ops, 512, 512, 512, "x16 512x512x512")
    finally:
        monkeypatch.undo()
        ops.reload_env()


def test_gemm_persistent_kernel_tile_carry_integer_exact(ops, monkeypatch):
    """cfg 16 with more 256 x 256 tiles than CUs (N = 4096, M = 256 (CUs / 16 + 1)): some workgroups run a second tile, whose K loop
    stores the first tile's output parked in registers.  Integer operands: every element of the BF16 output must be the rounded
    exact result, whatever tile and pass it came from."""
    N, K = 4096, 512
    M = 256 * (ops.device_cus() // 16 + 1)
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-8, 9, (M, K), generator=g).double()
    w = torch.randint(-8, 9, (N, K), generator=g).double()
    b = torch.randint(-64, 65, (N,), generator=g).double()
    ref = x @ w.t() + b                                        # integers below 2^24: exact in double as in fp32
    monkeypatch.setenv("LN3D_GEMM_TILE", "x16")
    ops.reload_env()
    try:
        y = _full((M, N), BF)
        ops.gemm(x.to(DEV, BF), w.to(DEV, BF), b.float().to(DEV), ops.EPI_BF16, y)
        _eq(y, kr.bf16_rne(ref), f"x16 persistent {M}x{N}x{K} BF16")
    finally:
        monkeypatch.undo()
        ops.reload_env()


def test_gemm_heads_split_with_fused_norm_float64(tile):
    """HEADS with head_norm0 / head_norm1 at the smallest accepting shape (1536 x 384 x 128, tokens 768): q, k = RMSNorm_64 of the fp32
    accumulators within the propagated bound, V^T plain; the tiles without the head-aligned epilogue must refuse."""
    ops, name = tile
    M, N, K, T, H, Dh = 1536, 384, 128, 768, 2, 64
    x, w, b, lin = _rand_case(M, N, K)
    g = torch.Generator().manual_seed(9)
    nq, nk = 1 + 0.3 * torch.randn(Dh, generator=g), 1 + 0.3 * torch.randn(Dh, generator=g)
    shapes, which, index, untouched = kr.heads_split_ref(M, N, T, T, H, Dh, Dh, 0b100)
    outs = [_full(s, BF, SENT) for s in shapes]
    run = lambda: ops.gemm(x.to(DEV), w.to(DEV), b.to(DEV), ops.EPI_HEADS, *outs, M=M, tokens=T, tok_pad=T, heads=H, head_dim=Dh,   # noqa: E731
                           transpose_mask=0b100, head_norm0=nq.to(DEV), head_norm1=nk.to(DEV), head_norm_eps=1e-5)
    accepts = name in ("auto", "x8", "x9", "x12", "x14")
    assert ops.heads_norm_fusable(M, N, T, Dh) == accepts
    if not accepts:
        with pytest.raises(RuntimeError, match=r"\(-3\)"):               # LN3D_ERR_UNSUPPORTED
            run()
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs)
        return
    run()
    for wi, wt in enumerate((nq, nk, None)):
        cols = which == wi
        ref, scale = lin[0][:, cols], lin[1][:, cols]
        if wt is not None:
            ref, scale = kr.heads_norm_ref(ref, scale, wt, 1e-5)
        got = outs[wi].double().cpu().reshape(-1)[index[:, cols].reshape(-1)]
        kr.assert_bf16_close(got, ref, scale, floor_ulps=kr.gemm_ulps(K), max_mismatch=0.01, what=f"{name} HEADS fused norm out{wi}")
        assert not bool(untouched[wi].any())


@pytest.mark.parametrize("M", [192, 384])
def test_gemm_cross_attention_epilogue_float64(tile, M):
    """CROSS_ATTN at its smallest legal shape (tokens 192, 4 heads, K 64; 128 x 192 tiles, 256 x 192 under x9).  Integer x, w make every
    q an integer below 256 - its bf16 rounding is the identity, wherever the kernel rounds it.  Random K / V caches, sentinels in the
    rows >= ctx_keys; against the float64 attention within the attention bound, and against the unfused HEADS GEMM + attention kernel
    within twice that bound."""
    ops, name = tile
    T, N, K, H = 192, 256, 64, 4
    Bn = M // T
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-1, 2, (M, K), generator=g)
    w = torch.randint(-1, 2, (N, K), generator=g)
    q = (x @ w.t()).double().reshape(Bn, T, H, 64).permute(0, 2, 1, 3)            # |q| <= 64
    xb, wb = x.to(DEV, BF), w.to(DEV, BF)
    for Lc in (1, 33, 64, 65, 96):
        lpad = (Lc + 63) // 64 * 64
        kc = torch.full((Bn, H, lpad, 64), 1e4)
        vc = torch.full((Bn, H, lpad, 64), 1e4)
        kc[:, :, :Lc] = torch.randn(Bn, H, Lc, 64, generator=g) * 0.5
        vc[:, :, :Lc] = torch.randn(Bn, H, Lc, 64, generator=g) + torch.arange(64) / 64
        kc, vc = kc.to(BF), vc.to(BF)
        ref, S = kr.attention_ref(q, kc, vc, 0.125, Lc)
        ref, S = (t.permute(0, 2, 1, 3).reshape(M, N) for t in (ref, S))
        kd, vt = kc.to(DEV), kr.to_vt(vc).to(DEV)
        kp = kd[..., ops.vt_key_order(64, DEV)].contiguous()
        out = _full((M, N), BF)
        ops.gemm(xb, wb, None, ops.EPI_CROSS_ATTN, out, kp, vt, M=M, tokens=T, heads=H, head_dim=64, ctx_keys=Lc, ctx_pad=lpad, ctx_scale=0.125)
        kr.assert_attention_close(out, ref, S, what=f"{name} CROSS_ATTN M {M} ctx {Lc}")
        qh = _full((Bn, H, T, 64), BF, SENT)
        ops.gemm(xb, wb, None, ops.EPI_HEADS, qh, M=M, tokens=T, tok_pad=T, heads=H, head_dim=64)
        _eq(qh, q, f"{name} HEADS q M {M}")
        o2 = _full((M, N), BF)
        ops.attention(qh, kd, vt, o2, Bn, H, T, T, Lc, lpad, 64, scale=0.125)
        kr.assert_attention_close(o2, ref, S, what=f"{name} unfused attention M {M} ctx {Lc}")
        kr.assert_attention_close(out, o2.double().cpu(), S, factor=2.0, what=f"{name} CROSS_ATTN vs unfused M {M} ctx {Lc}")


# ================================================================ attention: every path of the dispatcher
CASES = kr.attention_cases()
CASE_IDS = [f"{c[0]}-{c[3]}x{c[4]}" + (f"p{c[5]}" if c[5] else "") for c in CASES]
BH = kr.ATTENTION_BH


def _run_attention(ops, q, k, v, B, H, Nq, Nk, Dp, dt, causal, scale):
    """q [B, H, Nq_pad, Dp], k / v [B, H, Nk_pad, Dp] bf16 on the CPU, natural key order -> O [B, H, Nq, Do] as double on the CPU"""
    Do = dt or Dp
    out = _full((B, Nq, H * Do), BF)
    ops.attention(q.to(DEV), k.to(DEV), kr.to_vt(v).to(DEV), out, B, H, Nq, q.shape[2], Nk, k.shape[2], Dp, scale=scale, causal=causal, dh_true=dt)
    return out.double().cpu().reshape(B, Nq, H, Do).permute(0, 2, 1, 3)


def _pad_keys(t, nkp, value):
    """key rows padded to nkp with `value` in every stored dim"""
    if nkp is None or nkp == t.shape[2]:
        return t
    pad = torch.full((*t.shape[:2], nkp - t.shape[2], t.shape[3]), value, dtype=t.dtype)
    return torch.cat([t, pad], 2)


def _kres_heads(ops):
    cus = ops.device_cus()
    return (cus // 8, 8) if cus % 8 == 0 else (cus, 1)


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attention_selector_exact(ops, case, B, H):
    """q_i = code(pi(i)), k_j = code(j) with +-32 entries: the selected score beats every other by more than 150 in the exp2 domain, the
    softmax is exactly one-hot in fp32 and the output must be the selected V row bit for bit - batch / head indexing, Q / K row order,
    the V^T key permutation, tail and causal masking, ring wrap and the compact Dh_true output, whatever the arithmetic.  No two (b, h, key) rows of
    V coincide (kernel_refs.selector_values), so a row from the wrong batch, head, key block or ring lap shows.  Padded keys hold 1e4 in K
    and V^T and must never show."""
    path, Dp, dt, Nq, Nk, nkp, causal = case
    Dh = dt or Dp
    q, k, v, pi = kr.selector_inputs(B, H, Nq, Nk, Dh, Dp, nkp, causal)
    out = _run_attention(ops, q, k, v, B, H, Nq, Nk, Dp, dt, causal, Dh ** -0.5)
    _eq(out[..., :Dh], v[:, :, pi, :Dh].double(), f"selector {path} B {B} H {H} {Nq}x{Nk} (flat over [B, H, Nq, Dh])")
    if out.shape[-1] > Dh:
        assert float(out[..., Dh:].abs().max()) == 0


def _uniform_check(out, v, Nq, Nk, causal, what):
    vd = v[:, :, :Nk].double()
    if causal:
        cnt = torch.arange(1, Nq + 1, dtype=torch.float64)
        mean = vd.cumsum(2)[:, :, :Nq] / cnt[:, None]
    else:
        cnt = torch.full((Nq,), float(Nk), dtype=torch.float64)
        mean = vd.mean(2, keepdim=True).expand(-1, -1, Nq, -1)
    pow2 = (torch.frexp(cnt)[0] == 0.5)[None, None, :, None].expand_as(mean)
    want = kr.bf16_rne(mean)
    err = (out - want).abs()
    bad = torch.where(pow2, err != 0, err > kr.bf16_ulp(mean))
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements off the mean; first at flat index {i}: got {float(out.reshape(-1)[i])!r}, "
                             f"mean {float(mean.reshape(-1)[i])!r}")


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attention_uniform_exact(ops, case, B, H):
    """All keys zero, integer V: the output is the mean of the visible V rows - exactly its bf16 rounding where their count is a power of
    two, within 1 bf16 ulp otherwise."""
    path, Dp, dt, Nq, Nk, nkp, causal = case
    Dh = dt or Dp
    g = torch.Generator().manual_seed(Nq + 3 * Nk + B)
    nqp, nkp = (Nq + 63) // 64 * 64, nkp or (Nk + 63) // 64 * 64
    q = torch.zeros(B, H, nqp, Dp)
    q[:, :, :Nq, :Dh] = torch.randn(B, H, Nq, Dh, generator=g)
    k = torch.zeros(B, H, nkp, Dp)
    k[:, :, Nk:, :Dh] = 1e4
    v = torch.zeros(B, H, nkp, Dp)
    v[:, :, Nk:, :Dh] = 1e4
    v[:, :, :Nk, :Dh] = torch.randint(-8, 9, (B, H, Nk, Dh), generator=g).float()
    out = _run_attention(ops, q.to(BF), k.to(BF), v.to(BF), B, H, Nq, Nk, Dp, dt, causal, Dh ** -0.5)
    _uniform_check(out[..., :Dh], v[..., :Dh], Nq, Nk, causal, f"uniform {path} B {B} H {H} {Nq}x{Nk}")


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_attention_float64(ops, case, B, H):
    """Random operands (asymmetric V, a late spiked key where Nk > 128, 1e4 in the padded key rows) against the float64 softmax
    attention, masked when causal: |o - ref| <= 2^-8 sum p |v| + 1 bf16 ulp for every element."""
    path, Dp, dt, Nq, Nk, nkp, causal = case
    Dh = dt or Dp
    q, k, v = kr.attention_inputs(B, H, Nq, Nk, Dh, dh_pad=Dp, pad_value=1e4)
    k, v = _pad_keys(k, nkp, 1e4), _pad_keys(v, nkp, 1e4)
    if nkp:
        k[:, :, Nk:, Dh:], v[:, :, Nk:, Dh:] = 0, 0
    out = _run_attention(ops, q, k, v, B, H, Nq, Nk, Dp, dt, causal, Dh ** -0.5)
    ref, S = kr.attention_ref(q[:, :, :Nq, :Dh], k[..., :Dh], v[..., :Dh], Dh ** -0.5, Nk, causal)
    # the streaming kernel rounds the scaled query to bf16 a second time: that term, from its arithmetic, is added for its path only -
    # and, with that documented rounding put into the reference's query, the kernel is held to the plain bound like every other path
    extra = kr.attention_q_rounding_term(q[:, :, :Nq], k, v, Dh ** -0.5, ref, Nk) if path == "stream" else None
    kr.assert_attention_close(out[..., :Dh], ref, S, what=f"{path} B {B} H {H} {Nq}x{Nk}", extra=extra)
    if path == "stream":
        ref2, S2 = kr.attention_ref(kr.requantised_query(q[:, :, :Nq], Dh ** -0.5), k, v, None, Nk, base2=True)
        kr.assert_attention_close(out, ref2, S2, what=f"{path} B {B} H {H} {Nq}x{Nk}, re-rounded query in the reference")
    if out.shape[-1] > Dh:
        assert float(out[..., Dh:].abs().max()) == 0


@pytest.mark.parametrize("Nq,Nk", kr.KRES_SHAPES)
def test_attention_k_resident_kernel_elements(ops, Nq, Nk):
    """attn_kres_kernel (a head for every CU): selector, uniform and random operands as above."""
    B, H = _kres_heads(ops)
    q, k, v, pi = kr.selector_inputs(B, H, Nq, Nk, 64, 64)
    out = _run_attention(ops, q, k, v, B, H, Nq, Nk, 64, 0, False, 0.125)
    _eq(out, v[:, :, pi].double(), f"selector kres {B}x{H} {Nq}x{Nk} (flat over [B, H, Nq, Dh])")
    g = torch.Generator().manual_seed(Nk)
    vi = torch.randint(-8, 9, (B, H, Nk, 64), generator=g).float()
    out = _run_attention(ops, torch.randn(B, H, Nq, 64, generator=g).to(BF), torch.zeros(B, H, Nk, 64, dtype=BF), vi.to(BF), B, H, Nq, Nk, 64, 0,
                         False, 0.125)
    _uniform_check(out, vi, Nq, Nk, False, f"uniform kres {Nq}x{Nk}")
    q, k, v = kr.attention_inputs(B, H, Nq, Nk, 64)
    out = _run_attention(ops, q, k, v, B, H, Nq, Nk, 64, 0, False, 0.125)
    # the selector above holds every head exactly, with V rows that differ between any two heads; the float64 bound is taken over every
    # 29th head, the first and the last (independent workgroups of the same code; the float64 reference of all takes several seconds)
    pick = sorted(set(range(0, B * H, 29)) | {B * H - 1})
    qs, ks, vs, os_ = (t.reshape(1, B * H, *t.shape[2:])[:, pick] for t in (q, k, v, out))
    ref, S = kr.attention_ref(qs, ks, vs, 0.125)
    extra = kr.attention_q_rounding_term(qs, ks, vs, 0.125, ref)              # the second rounding of the scaled query, as attn_stream
    kr.assert_attention_close(os_, ref, S, what=f"kres {B}x{H} {Nq}x{Nk} heads {pick}", extra=extra)
    ref2, S2 = kr.attention_ref(kr.requantised_query(qs, 0.125), ks, vs, None, base2=True)
    kr.assert_attention_close(os_, ref2, S2, what=f"kres {B}x{H} {Nq}x{Nk} heads {pick}, re-rounded query in the reference")


UNSUPPORTED, BAD_ARG = r"\(-3\)", r"\(-1\)"            # LN3D_ERR_UNSUPPORTED / LN3D_ERR_BAD_ARG as _lib.check reports them


@pytest.mark.parametrize("what,code,kw", [("causal with Dh 128", UNSUPPORTED, dict(Dh=128, Nk=64, causal=True)),
                                          ("causal with Nk 129", UNSUPPORTED, dict(Dh=64, Nk=129, causal=True)),
                                          ("Dh_true 70 in 128", UNSUPPORTED, dict(Dh=128, Nk=64, dh_true=70)),
                                          ("Dh_true 70 in 80", UNSUPPORTED, dict(Dh=80, Nk=64, dh_true=70)),
                                          ("Dh_true 48 in 64", UNSUPPORTED, dict(Dh=64, Nk=64, dh_true=48)),
                                          ("Nk_pad 100", BAD_ARG, dict(Dh=64, Nk=64, nkp=100))])
def test_attention_refusals_leave_the_output_untouched(ops, what, code, kw):
    """Each documented refusal, by its own error code (a refusal for another reason does not pass), with the NaN-filled output untouched."""
    Dh, Nk, Nq = kw["Dh"], kw["Nk"], 64
    nkp = kw.get("nkp") or (Nk + 63) // 64 * 64
    alloc = (nkp + 63) // 64 * 64
    q, k, vt = (torch.zeros(s, device=DEV, dtype=BF) for s in ((1, 1, Nq, Dh), (1, 1, alloc, Dh), (1, 1, Dh, alloc)))
    out = _full((1, Nq, 128), BF)
    with pytest.raises(RuntimeError, match=code):
        ops.attention(q, k, vt, out, 1, 1, Nq, Nq, Nk, nkp, Dh, causal=kw.get("causal", False), dh_true=kw.get("dh_true", 0))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), what
