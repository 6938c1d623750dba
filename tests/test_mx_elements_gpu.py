"""The MX-FP8 kernels of include/ln3d_mx.h per element: ln3d_quantize_mx over the whole E4M3 code space and its non-finite rule,
ln3d_gemm_mxfp8 EXACTLY (integer elements, power-of-two block scales: every partial sum exact in fp32, tests/mx_refs.py) in every
epilogue at the smallest shapes that reach every tile edge, K-stage count and operand stride, its GELU -> MXFP8 epilogue and
ln3d_norm_modulate_mx against the reference quantizer of the float64 result.  Every output buffer starts as a sentinel and every test
asserts that nothing outside the written region changed."""
import functools

import pytest
import torch

import kernel_refs as kr
import mx_refs as mr
from test_mxfp8_cpu import quantize_mx_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SENT = -3.0                                   # fp32 / bf16 sentinel
SENT8 = 0xA5                                  # byte sentinel
NAN8 = 0x7F                                   # operand padding: the E4M3 NaN code, so that a read of it poisons the result


@pytest.fixture
def ops(hip_lib):
    from ln3diff_amd import ops as o
    return o


def _eq(y, ref, what):
    """every element of y equals ref; names the first that does not"""
    yd, rd = y.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    assert yd.numel() == rd.numel() and yd.dtype == rd.dtype, (what, yd.shape, rd.shape, yd.dtype, rd.dtype)
    bad = ~(yd == rd)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} / {yd.numel()} elements differ; first at flat index {i}: got {yd[i].item()!r}, expected {rd[i].item()!r}")


# ================================================================ quantizer
def _quantize_strided(ops, x):
    """x (CPU, [R, K]) through ln3d_quantize_mx with ldx = K + 8, ldq = K + 4, lds = K / 32 + 3 (column-sliced views of sentinel-filled
    buffers with one more row) -> (q, s) on the CPU, after the check that nothing but [R, K] / [R, K / 32] was written."""
    R, K = x.shape
    xb = torch.full((R + 1, K + 8), 7.0, dtype=x.dtype)
    xb[:R, :K] = x
    qb = torch.full((R + 1, K + 4), SENT8, dtype=torch.uint8, device=DEV)
    sb = torch.full((R + 1, K // 32 + 3), SENT8, dtype=torch.uint8, device=DEV)
    ops.quantize_mx(xb.to(DEV)[:R, :K], out=ops.MX(qb[:R, :K], sb[:R, :K // 32]))
    qb, sb = qb.cpu(), sb.cpu()
    assert bool((qb[:, K:] == SENT8).all()) and bool((qb[R:] == SENT8).all()), "element bytes outside [R, K] written"
    assert bool((sb[:, K // 32:] == SENT8).all()) and bool((sb[R:] == SENT8).all()), "scale bytes outside [R, K / 32] written"
    return qb[:R, :K], sb[:R, :K // 32]


def _probe_blocks(p):
    """magnitudes p -> f32 [n, 32] blocks [448, 31 probes] with both signs (e = 0: the element is RNE(probe) itself)"""
    v = torch.cat([p, -p])
    n = (v.numel() + 30) // 31
    pad = torch.zeros(n * 31)                              # the last block is padded with zeros
    pad[:v.numel()] = v
    return torch.cat([torch.full((n, 1), 448.0), pad.reshape(n, 31)], 1)


@pytest.mark.parametrize("shift", [0, -100, 100])
def test_quantize_mx_rounds_every_e4m3_boundary(ops, shift):
    """every code value, every midpoint between neighbouring codes and the f32 values on both sides of it, the subnormal range and values
    beyond 448, both signs: the codes are those of the independent rounding oracle, at block scales 2^0, 2^-100 and 2^+100"""
    blk = _probe_blocks(mr.e4m3_probes())
    want = mr.e4m3_rne_expected(blk)
    q, s = _quantize_strided(ops, torch.ldexp(blk, torch.tensor(shift)))
    assert bool((s == 127 + shift).all())
    _eq(q, want, f"probes * 2^{shift}")
    assert sorted(set((q & 0x7F).reshape(-1).tolist())) == list(range(0x7F))         # every finite code was produced


def test_quantize_mx_bf16_input_rounds_every_boundary_it_can_hold(ops):
    p = mr.e4m3_probes()
    p = p[p.bfloat16().float() == p]                                                # code values and midpoints, not their f32 neighbours
    assert p.numel() >= 127 + 126
    blk = _probe_blocks(p)
    q, s = _quantize_strided(ops, blk.bfloat16())
    assert bool((s == 127).all())
    _eq(q, mr.e4m3_rne_expected(blk), "bf16 probes")


def _nan32(neg):
    return torch.tensor([-4194304 if neg else 0x7FC00000], dtype=torch.int32).view(torch.float32)[0]


def _with_nonfinite(x):
    """f32 [6, 96]: NaN (both signs) and +-Inf among finite values, a block of NaN only, a block of Inf only, a signed zero"""
    x = x.clone()
    inf = float("inf")
    x[0, 3], x[0, 40], x[0, 95] = _nan32(False), inf, -inf
    x[1, 32], x[1, 33] = _nan32(True), _nan32(False)
    x[2, 0:32] = _nan32(False)
    x[2, 5] = _nan32(True)
    x[3, 64:96] = inf
    x[3, 64:96:3] = -inf
    x[4, 31], x[4, 32], x[4, 63], x[4, 64] = inf, -inf, _nan32(True), inf          # block edges
    x[5, 0:32] = 0.0
    x[5, 7], x[5, 9] = -0.0, inf                                                    # no finite non-zero element: byte 0
    return x


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_quantize_mx_nonfinite_rule(ops, dtype):
    """amax over the finite elements, NaN / Inf stored as 0x7F / 0xFF by their sign, the finite elements of the block as without them"""
    g = torch.Generator().manual_seed(5)
    base = (torch.randn(6, 96, generator=g) * torch.exp2(torch.randint(-20, 20, (6, 3), generator=g).float()).repeat_interleave(32, 1)).to(dtype).float()
    x32 = _with_nonfinite(base)
    x = x32.to(dtype)
    if dtype == BF:                                       # torch's f32 -> bf16 cast does not keep the sign of a NaN: write the bits
        nan = torch.isnan(x32)
        x.view(torch.int16)[nan] = torch.where(torch.signbit(x32[nan]), torch.tensor(-64), torch.tensor(0x7FC0)).to(torch.int16)
    q_ref, s_ref = quantize_mx_ref(x)
    q, s = _quantize_strided(ops, x)
    _eq(s, s_ref, "scales")
    _eq(q, q_ref, "codes")
    # and the rule itself, not only the reference's reading of it
    nf = ~torch.isfinite(x32)
    assert bool((q[nf] == torch.where(torch.signbit(x32[nf]), 0xFF, 0x7F)).all()) and not bool(((q[~nf] & 0x7F) == 0x7F).any())
    q0, s0 = quantize_mx_ref(torch.where(nf, torch.zeros_like(x32), x32))
    assert torch.equal(s, s0) and torch.equal(q[~nf], q0[~nf])
    assert s[2, 0] == 0 and s[3, 2] == 0 and s[5, 0] == 0 and q[5, 7] == 0x80 and q[5, 8] == 0x00


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("R,K", [(1, 32), (3, 96), (257, 160)])
def test_quantize_mx_strided_shapes(ops, dtype, R, K):
    """one block, a few, and 257 * 5 blocks (not a multiple of the 256 threads of a workgroup), every operand strided; signed zeros kept"""
    g = torch.Generator().manual_seed(R + K)
    x = torch.randn(R, K, generator=g) * torch.exp2(torch.randint(-30, 30, (R, K // 32), generator=g).float()).repeat_interleave(32, 1)
    x[0, 1], x[0, 2] = -0.0, 0.0
    if K > 32:
        x[R - 1, K - 32:] = -0.0                                                      # a block of negative zeros: byte 0, 0x80
    x = x.to(dtype)
    q_ref, s_ref = quantize_mx_ref(x)
    q, s = _quantize_strided(ops, x)
    _eq(s, s_ref, "scales")
    _eq(q, q_ref, "codes")
    assert q[0, 1] == 0x80 and q[0, 2] == 0x00 and (K == 32 or (bool((q[R - 1, K - 32:] == 0x80).all()) and s[R - 1, K // 32 - 1] == 0))


# ================================================================ GEMM: exact operands
@functools.lru_cache(maxsize=None)
def _case(M, N, K, vmax=8, emin=-2, emax=2, bias_max=64):
    """(x q/s/deq, w q/s/deq, integer bias, float64 x w^T): CPU tensors, computed once per shape"""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x, w = mr.mx_exact_operand(M, K, g, vmax, emin, emax), mr.mx_exact_operand(N, K, g, vmax, emin, emax)
    b = torch.randint(-bias_max, bias_max + 1, (N,), generator=g).double()
    return x, w, b, x[2] @ w[2].T


def _put(ops, t, extra_rows=2):
    """(q, s, deq) -> the operand as the view the model passes: first row at offset 3 of a buffer whose rows are 16 bytes (4 scale
    bytes) longer, `extra_rows` more rows behind it; everything around the operand holds the E4M3 NaN code / scale byte 0xFF"""
    q, s, _ = t
    R, K = q.shape
    qb = torch.full((3 + R + extra_rows, K + 16), NAN8, dtype=torch.uint8)
    sb = torch.full((3 + R + extra_rows, K // 32 + 4), 0xFF, dtype=torch.uint8)
    qb[3:3 + R, :K], sb[3:3 + R, :K // 32] = q, s
    qb, sb = qb.to(DEV), sb.to(DEV)
    return ops.MX(qb[3:, :K], sb[3:, :K // 32])


# a sparse cross of M {1, 31, 33, 127, 129, 257} x N {4, 36, 124, 132, 260} x K {128, 256, 384, 640} (K / 128 = 1, 2, 3, 5 stages: no
# prefetch, no refill, the first refill, an odd wrap of the two-slot ring) in which every value appears, the largest of each together
F32_CASES = [(1, 4, 128), (31, 36, 256), (33, 124, 384), (127, 132, 640), (129, 260, 128), (257, 4, 256), (1, 132, 384), (33, 260, 640),
             (257, 260, 640), (129, 36, 384), (127, 124, 128), (31, 132, 128)]


@pytest.mark.parametrize("M,N,K", F32_CASES)
def test_gemm_mx_f32_exact(ops, M, N, K):
    """EPI_F32 equals the float64 product bit for bit, with and without bias, into ldo = N + 12, from row-offset, column-padded operand
    views (ldx = K + 16, ldxs = K / 32 + 4) with more rows than M"""
    mr.assert_fp32_exact(K, 8, -2, 2, bias=64)
    x, w, b, prod = _case(M, N, K)
    xm, wm = _put(ops, x), _put(ops, w, extra_rows=0)
    assert xm.q.stride(0) == K + 16 and xm.s.stride(0) == K // 32 + 4 and xm.q.shape[0] == M + 2
    for bias in (None, b):
        out = torch.full((M + 2, N + 12), SENT, device=DEV)
        ops.gemm_mx(xm, wm, None if bias is None else bias.float().to(DEV), ops.EPI_F32, out, M=M, ldo=N + 12)
        ref = (prod if bias is None else prod + bias).float()
        what = f"F32 {M}x{N}x{K} bias {bias is not None}"
        _eq(out[:M, :N], ref, what)
        assert bool((out[:M, N:] == SENT).all()) and bool((out[M:] == SENT).all()), what + ": written outside [M, N]"


# (M, N, K, gate_rows or None (no gate), bias, bf16 copy)
GATE_CASES = [(21, 36, 128, 7, True, True), (21, 132, 384, 1, False, False), (21, 36, 384, 21, True, False), (130, 36, 384, 130, False, True),
              (130, 132, 128, 1, True, True), (130, 132, 384, None, True, True), (21, 36, 128, None, False, False)]


@pytest.mark.parametrize("M,N,K,gate_rows,with_bias,with_copy", GATE_CASES)
def test_gemm_mx_gate_residual_exact(ops, M, N, K, gate_rows, with_bias, with_copy):
    """out0 = residual + gate[row / gate_rows] * (x w^T + bias) with an integer residual and gates +-2^j: exact; gate rows of stride
    N + 8; the bf16 copy is the rounded new residual"""
    mr.assert_fp32_exact(K, 8, -1, 1, bias=64, gate_exp=2, res=500)
    x, w, b, prod = _case(M, N, K, 8, -1, 1)
    g = torch.Generator().manual_seed(M + N + K)
    res = torch.randint(-500, 501, (M, N), generator=g).double()
    ns = (M + gate_rows - 1) // gate_rows if gate_rows else 0
    ldo = N + 4
    out = torch.full((M + 1, ldo), SENT, device=DEV)
    out[:M, :N] = res.float().to(DEV)
    copy = torch.full((M + 1, ldo), SENT, dtype=BF, device=DEV) if with_copy else None
    lin = prod + b if with_bias else prod
    kw = {}
    if gate_rows:
        gate = torch.exp2(torch.randint(-2, 3, (ns, N), generator=g).double()) * (1 - 2 * torch.randint(0, 2, (ns, N), generator=g)).double()
        gbuf = torch.full((ns, N + 8), float("nan"), device=DEV)
        gbuf[:, :N] = gate.float().to(DEV)
        kw = dict(gate=gbuf, gate_rows=gate_rows, gate_ld=N + 8)
        lin = gate.repeat_interleave(gate_rows, 0)[:M] * lin
    ops.gemm_mx(_put(ops, x), _put(ops, w, 0), b.float().to(DEV) if with_bias else None, ops.EPI_GATE_RES, out, copy, M=M, ldo=ldo, **kw)
    what = f"GATE_RES {M}x{N}x{K} gate_rows {gate_rows} bias {with_bias}"
    _eq(out[:M, :N], (res + lin).float(), what)
    assert bool((out[:M, N:] == SENT).all()) and bool((out[M:] == SENT).all()), what + ": out0 written outside [M, N]"
    if with_copy:
        _eq(copy[:M, :N], out[:M, :N].bfloat16(), what + " bf16 copy")
        assert bool((copy[:M, N:] == SENT).all()) and bool((copy[M:] == SENT).all()), what + ": out1 written outside [M, N]"


HEAD_CFGS = [(1, 64, 64), (2, 32, 32), (8, 8, 8), (8, 72, 80)]                 # heads, head_dim, head_dim_pad: heads * head_dim % 64 == 0
TOKENS = [(8, 8), (31, 32), (33, 64), (96, 96), (77, 96)]                     # tokens, tok_pad; M = 2 * tokens: both sides of tokens < 32


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("H,Dh,Dp", HEAD_CFGS)
def test_gemm_mx_heads_exact(ops, H, Dh, Dp, K):
    """HEADS: q / k / V^T hold bf16_rne of the exact value at the position kr.heads_split_ref gives, for transpose masks 0, 0b100, 0b111;
    token and head-dim padding keep the sentinel, as under ln3d_gemm_bf16 (test_gemm_heads_split_integer_exact), and the bf16 GEMM on
    the same (bf16-exact) operands gives the same three tensors bit for bit.  A transposed output with tok_pad % 16 != 0 (tokens 8
    into 8) would store past its rows: refused, outputs untouched."""
    mr.assert_fp32_exact(K, 8, -2, 2, bias=64)
    N = 3 * H * Dh
    for tokens, tp in TOKENS:
        M = 2 * tokens
        x, w, b, prod = _case(M, N, K)
        want = kr.bf16_rne(prod + b)
        xm, wm, bd = _put(ops, x), _put(ops, w, 0), b.float().to(DEV)
        xb, wb = x[2].to(DEV, BF), w[2].to(DEV, BF)
        assert torch.equal(xb.double().cpu(), x[2])                               # the dequantized operands are bf16 values
        for mask in (0, 0b100, 0b111):
            what = f"HEADS {H}x{Dh}->{Dp} tokens {tokens}/{tp} K {K} mask {mask:03b}"
            kw = dict(M=M, tokens=tokens, tok_pad=tp, heads=H, head_dim=Dh, transpose_mask=mask, head_dim_pad=Dp)
            refused = bool(mask) and tp % 16 != 0                                 # (the layout map itself leaves the tensor there)
            shapes, which, index, untouched = kr.heads_split_ref(M, N, tokens, tp, H, Dh, Dp, 0 if refused else mask)
            outs = [torch.full(s, SENT, dtype=BF, device=DEV) for s in shapes]
            if refused:
                with pytest.raises(RuntimeError):
                    ops.gemm_mx(xm, wm, bd, ops.EPI_HEADS, *outs, **kw)
                assert all(bool((o == SENT).all()) for o in outs), what + ": refused, yet written"
                continue
            ops.gemm_mx(xm, wm, bd, ops.EPI_HEADS, *outs, **kw)
            outs_bf = [torch.full(s, SENT, dtype=BF, device=DEV) for s in shapes]
            ops.gemm(xb, wb, bd, ops.EPI_HEADS, *outs_bf, **kw)
            for wi, out in enumerate(outs):
                flat = out.double().cpu().reshape(-1)
                cols = which == wi
                _eq(flat[index[:, cols].reshape(-1)], want[:, cols], f"{what} out{wi}")
                assert bool((flat[untouched[wi]] == SENT).all()), f"{what} out{wi}: padding written"
                assert torch.equal(out, outs_bf[wi]), f"{what} out{wi}: differs from ln3d_gemm_bf16"


# ================================================================ GEMM: GELU -> MXFP8
GELU_NEAR_REL = 1e-4                          # tests/test_mxfp8_gpu.py's value for this epilogue


@pytest.mark.parametrize("K", [128, 384])
def test_gemm_mx_gelu_mx_output(ops, K):
    """exact pre-activations (integers up to 4, scales 2^-4 .. 2^-3: a standard deviation of 0.7 - 1.3, so that the GELU is on its
    curved part), the erf polynomial the only error: the MXFP8 output against the reference quantizer of the float64 GELU, with and
    without bias, out0 with ldo = N + 4, the scales as a column slice (ldos = N / 32 + 3); nothing beyond M or N written"""
    mr.assert_fp32_exact(K, 4, -4, -3, bias=2)
    for M in (1, 33, 130):
        for N in (32, 96, 160):
            x, w, b, prod = _case(M, N, K, 4, -4, -3, 2)
            xm, wm = _put(ops, x), _put(ops, w, 0)
            for bias in (None, b):
                oq = torch.full((M + 2, N + 4), SENT8, dtype=torch.uint8, device=DEV)
                os_ = torch.full((M + 2, N // 32 + 3), SENT8, dtype=torch.uint8, device=DEV)
                ops.gemm_mx(xm, wm, None if bias is None else bias.float().to(DEV), ops.EPI_GELU_ERF, oq, M=M, ldo=N + 4, out_scale=os_[:, :N // 32])
                v = mr.gelu64(prod if bias is None else prod + bias)
                print(f"GELU {M}x{N}x{K} bias {bias is not None}:")
                mr.check_mx_output(oq[:M, :N], os_[:M, :N // 32], v, 'gelu', GELU_NEAR_REL)
                assert bool((oq[:M, N:] == SENT8).all()) and bool((oq[M:] == SENT8).all()), "element bytes outside [M, N] written"
                assert bool((os_[:M, N // 32:] == SENT8).all()) and bool((os_[M:] == SENT8).all()), "scale bytes outside [M, N / 32] written"


# ================================================================ GEMM: NaN codes in the operands
@pytest.mark.parametrize("side", ["x", "w"])
def test_gemm_mx_nan_code_poisons_its_row_or_column(ops, side):
    """one element of X row 5 (K block 1) set to 0x7F, or one of W row 2 to 0xFF: that output row (column) is NaN, every other element
    still the exact product"""
    M, N, K = 40, 36, 256
    mr.assert_fp32_exact(K, 8, -2, 2)
    x, w, _, prod = _case(M, N, K)
    xq, wq = x[0].clone(), w[0].clone()
    if side == "x":
        xq[5, 32 + 7] = 0x7F
    else:
        wq[2, 100] = 0xFF
    out = torch.full((M, N), SENT, device=DEV)
    ops.gemm_mx(_put(ops, (xq, x[1], None)), _put(ops, (wq, w[1], None), 0), None, ops.EPI_F32, out, M=M)
    out = out.cpu()
    hit = torch.zeros(M, N, dtype=torch.bool)
    if side == "x":
        hit[5] = True
    else:
        hit[:, 2] = True
    print("NaN code in", side, "-> first values of the poisoned row / column:", out[hit][:8].tolist())
    _eq(out[~hit], prod.float()[~hit], f"NaN code in {side}: the other elements")
    assert bool(torch.isnan(out[hit]).all()), f"NaN code in {side}: {int((~torch.isnan(out[hit])).sum())} of {int(hit.sum())} elements are not NaN"


# ================================================================ norm + modulate -> MXFP8
NORM_NEAR_REL = 1e-6                          # tests/test_mxfp8_gpu.py's value for this kernel
NORM_D = [128, 512, 640, 1024, 1152, 1280, 1536]
NORM_ROWS = [(1, 1), (3, 1), (5, 2), (1000, 250)]         # rows, mod_rows: rows % 4 != 0 and rows % mod_rows != 0 among them


def _norm_cases():
    """a sparse cross: every width, row count, weight and modulation setting appears with both kinds"""
    for i, D in enumerate(NORM_D):
        for kind in (0, 1):
            j = i + 2 * kind
            yield D, kind, NORM_ROWS[j % 4], bool((i + kind) & 1), bool(((i >> 1) + kind) & 1)


def _norm_run(ops, x, kind, weight, mod, mod_rows):
    """x CPU f32 [rows, D] -> (q, s) CPU of rows + 1 rows (the last one the sentinel); mod: [ceil(rows / mod_rows), 6 D] or None, its
    columns [D, 2D) the shift and [4D, 5D) the scale (mod_ld = 6 D, the adaLN row stride of the model)"""
    rows, D = x.shape
    y = ops.MX(torch.full((rows + 1, D), SENT8, dtype=torch.uint8, device=DEV), torch.full((rows + 1, D // 32), SENT8, dtype=torch.uint8, device=DEV))
    kw = {}
    if mod is not None:
        md = mod.to(DEV)
        kw = dict(shift=md[:, D:2 * D], scale=md[:, 4 * D:5 * D], mod_rows=mod_rows, mod_ld=6 * D)
    ops.norm_modulate_mx(x.to(DEV), y, rows, D, kind=kind, eps=1e-6, weight=None if weight is None else weight.to(DEV), **kw)
    q, s = y.q.cpu(), y.s.cpu()
    assert bool((q[rows:] == SENT8).all()) and bool((s[rows:] == SENT8).all()), "the row after `rows` was written"
    return q, s


def _norm_ref(x, kind, weight, mod, mod_rows):
    D = x.shape[1]
    if mod is None:
        return kr.norm_modulate(x, kind, 1e-6, weight=weight)[0]
    return kr.norm_modulate(x, kind, 1e-6, weight=weight, shift=mod[:, D:2 * D], scale=mod[:, 4 * D:5 * D], mod_rows=mod_rows)[0]


@pytest.mark.parametrize("D,kind,rows_mod,with_weight,with_mod", list(_norm_cases()))
def test_norm_modulate_mx_elements(ops, D, kind, rows_mod, with_weight, with_mod):
    rows, mod_rows = rows_mod
    g = torch.Generator().manual_seed(D + kind)
    x = torch.randn(rows, D, generator=g) * 3 + 0.5
    weight = torch.randn(D, generator=g) if with_weight else None
    mod = torch.randn((rows + mod_rows - 1) // mod_rows, 6 * D, generator=g) * 0.5 if with_mod else None
    q, s = _norm_run(ops, x, kind, weight, mod, mod_rows)
    print(f"norm D {D} kind {kind} rows {rows}/{mod_rows} weight {with_weight} mod {with_mod}:")
    mr.check_mx_output(q[:rows], s[:rows], _norm_ref(x, kind, weight, mod, mod_rows), 'norm', NORM_NEAR_REL)


@pytest.mark.parametrize("with_mod", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("D", [128, 1152])
def test_norm_modulate_mx_special_rows(ops, D, kind, with_mod):
    """row 0 zeros (without modulation: scale byte 0, codes 0 / 0x80), row 1 of large magnitude (x 2^60 with |x| <= 1/8: (x - mean)^2 <=
    2^116, so the fp32 sum of D <= 1536 squares stays below 2^127 and the statistics are finite), rows 2 - 4 with one NaN, +Inf, -Inf:
    the row statistics are not finite, so every element is the NaN code and every scale byte 0; the rows around them are ordinary"""
    g = torch.Generator().manual_seed(D + kind)
    rows = 7
    x = torch.randn(rows, D, generator=g) * 3 + 0.5
    x[0] = 0.0
    x[1] = (torch.rand(D, generator=g) - 0.5) * 0.25 * 2.0 ** 60
    x[2, D // 3], x[3, 5], x[4, D - 1] = float("nan"), float("inf"), float("-inf")
    weight = torch.randn(D, generator=g)
    mod = torch.randn(4, 6 * D, generator=g) * 0.5 if with_mod else None
    q, s = _norm_run(ops, x, kind, weight, mod, 2)
    fin = torch.tensor([0, 1, 5, 6])
    print(f"norm special rows D {D} kind {kind} mod {with_mod}:")
    mr.check_mx_output(q[fin], s[fin], _norm_ref(x[fin], kind, weight, None if mod is None else mod.repeat_interleave(2, 0)[fin], 1), 'norm',
                       NORM_NEAR_REL)
    assert bool(((q[2:5] & 0x7F) == 0x7F).all()), "a row with a NaN / Inf element must be the NaN code throughout"
    assert bool((s[2:5] == 0).all()), "scale bytes of a row without a finite element"
    if not with_mod:
        assert bool((s[0] == 0).all()) and bool(((q[0] & 0x7F) == 0).all())
