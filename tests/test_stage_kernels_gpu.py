"""The glue kernels of the U-Net denoiser (csrc/unet_ops.hip), the ShapeNet and FFHQ VAE decoders (csrc/shapenet_ops.hip,
csrc/ffhq_ops.hip), the multi-view encoder (csrc/conv_ops.hip) and the DiT boundary (patch embed, final layer, per-head RMSNorm), each
against a float64 restatement (tests/kernel_refs.py) at the shapes, types and edges where they go wrong: idle lanes and waves,
rectangular images, odd token counts, saturating and cancelling inputs.  Same bounds as tests/test_glue_kernels_gpu.py: bf16 outputs
within 1 bf16 ulp of the float64 value (floor: fp32 ulps of the magnitude of the summed terms, derived per kernel in its docstring) and
at most 1 % of the elements off the correctly rounded value; fp32 outputs within a derived number of fp32 ulps of the terms; layout
and gather kernels bitwise equal to the torch expression.  Every output buffer is pre-filled with NaN and carries a NaN tail of 64
elements that must come back untouched.  None of these kernels touches the GEMM, so the tile-forcing `ops` fixture is not used.

Measured worst cases on gfx950 are noted beside each bound ("measured: ...")."""
import ctypes as C
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 64
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def o(hip_lib):
    from ln3diff_amd import ops
    return ops


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _nan_buf(n, dtype=F32):
    """(whole buffer, its first n elements): NaN everywhere, TAIL elements past the end"""
    buf = torch.full((n + TAIL,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[:n]


def _with_tail(t):
    """t (CPU) on the device, followed by a NaN tail: for kernels that work in place"""
    buf = torch.full((t.numel() + TAIL,), float("nan"), dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf, buf[:t.numel()].view(t.shape)


def _tail_untouched(*bufs):
    for b in bufs:
        assert bool(torch.isnan(b[-TAIL:]).all()), "sentinel tail overwritten"


def _bits_equal(y, ref):
    assert y.dtype == ref.dtype and y.numel() == ref.numel(), (y.dtype, ref.dtype, y.shape, ref.shape)
    v = {F32: torch.int32, BF: torch.int16}[y.dtype]
    yb, rb = y.detach().cpu().reshape(-1).view(v), ref.detach().cpu().contiguous().reshape(-1).view(v)
    if not torch.equal(yb, rb):
        i = int((yb != rb).nonzero()[0])
        raise AssertionError(f"{int((yb != rb).sum())} / {yb.numel()} elements differ; first at flat index {i}: "
                             f"{float(y.reshape(-1)[i])!r} != {float(ref.reshape(-1)[i])!r}")


def _offset_rows(x, seed):
    """every third row moved to |mean| / std = 300 (as tests/test_glue_kernels_gpu.py does)"""
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    sd = x[::3].std() if x[::3].numel() > 1 else torch.tensor(1.0)
    x[::3] += 300 * sd * torch.sign(torch.randn(x[::3].shape[0], 1, generator=g))
    return x


# ---------------------------------------------------------------- ln3d_attention_small
ATTN_DH_NK = [(1, 1), (1, 65), (40, 63), (40, 77), (63, 64), (63, 1000), (64, 64), (64, 1024), (65, 1), (65, 65), (160, 77), (160, 1024),
              (256, 63), (256, 1000)]          # every Dh with two Nk, every Nk with two Dh


def _attn_inputs(kind, B, H, Nq, Nk, Dh, g):
    """(q, k, v [B, N, H, Dh] bf16, softmax scale)"""
    scale = Dh ** -0.5
    q, k, v = torch.randn(B, Nq, H, Dh, generator=g), torch.randn(B, Nk, H, Dh, generator=g), torch.randn(B, Nk, H, Dh, generator=g)
    if kind == "dominant":            # key Nk // 2 beats every other key of every row by at least 40: the others spread over +-6
        q[..., 0] = 2.0
        k[..., 0] = 0.0
        k[:, Nk // 2, :, 0] = 52.0 / (2.0 * scale)
    elif kind == "identical":         # uniform softmax: the output is the mean of v
        k = k[:, :1].expand(B, Nk, H, Dh).clone()
    elif kind == "spread":            # integer q, k and a power-of-two scale: the fp32 scores are exact, their spread is hundreds
        q = torch.randint(-2, 3, (B, Nq, H, Dh), generator=g).float()
        k = torch.randint(-64, 65, (B, Nk, H, Dh), generator=g).float()
        scale = 0.5
    return q.to(BF), k.to(BF), v.to(BF), scale


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("B,H,Nq", [(1, 1, 1), (1, 1, 5), (2, 4, 12)])
@pytest.mark.parametrize("Dh,Nk", ATTN_DH_NK)
def test_attention_small(o, Dh, Nk, B, H, Nq, fused):
    """ln3d_attention_small (CrossAttention / QKVAttentionLegacy of the U-Net) at head sizes around the 64-lane stride and up to the
    limit 256, key counts around 64 and up to the limit 1024, 1 / 5 / 96 (batch, head, query) items (1 and 5 leave idle waves in the
    last block), q / k / v as column slices of fused [B * N, 3 * H * Dh] projections (ld = 3 H Dh) and as separate tensors
    (ld = H Dh); inputs: plain randn, one key ahead of all others by >= 40, identical keys (uniform softmax), integer scores spread
    over hundreds (most exp arguments below -87).
    Bound: 1 bf16 ulp, floor per row (kernel_refs.attention_floor, n_dot = Dh + 1: bf16 x bf16 products are exact in fp32)
      Dh+1 roundings * |scale| max_j sum_d |q_d k_jd|  +  (Nk + Nk / 64 + 4 ln Nk + 18) / 2   fp32 ulps of sum_j p_j |v_j|;
    mismatch <= 1 % for every input kind whose output has at least 200 elements and over the four kinds together (with one item
    a head is 1 - 256 elements, and one flipped rounding tie of 63 is already 1.6 %).  Measured:
    worst 0.50 of the bound, mismatch at most 4.0e-3 over the four kinds (one element of 63, 1.6 %, in the smallest single output)."""
    HD = H * Dh
    pooled = []
    for kind in ("plain", "dominant", "identical", "spread"):
        g = _gen("attn", Dh, Nk, B, H, Nq, fused, kind)
        q, k, v, scale = _attn_inputs(kind, B, H, Nq, Nk, Dh, g)
        if fused:
            ld = 3 * HD
            qsrc = torch.randn(B * Nq, ld, generator=g).to(BF)
            ksrc = qsrc if Nq == Nk else torch.randn(B * Nk, ld, generator=g).to(BF)
            qsrc[:, :HD] = q.reshape(B * Nq, HD)
            ksrc[:, HD:2 * HD] = k.reshape(B * Nk, HD)
            ksrc[:, 2 * HD:] = v.reshape(B * Nk, HD)
            qd = qsrc.to(DEV)
            kd = qd if Nq == Nk else ksrc.to(DEV)
            qv, kv, vv = qd[:, :HD], kd[:, HD:2 * HD], kd[:, 2 * HD:]
        else:
            ld = HD
            qv, kv, vv = q.reshape(B * Nq, HD).to(DEV), k.reshape(B * Nk, HD).to(DEV), v.reshape(B * Nk, HD).to(DEV)
        buf, out = _nan_buf(B * Nq * HD, BF)
        o.attention_small(qv, kv, vv, out, B, H, Nq, Nk, Dh, ld, ld, ld, scale)
        ref, mag, floor = kr.attention_small(q, k, v, scale)
        kr.assert_bf16_close(out, ref, mag * floor, floor_ulps=1, max_mismatch=0.01 if out.numel() >= 200 else 1.0,
                             what=f"attention_small Dh{Dh} Nk{Nk} items{B * H * Nq} fused{fused} {kind}")
        _tail_untouched(buf)
        pooled.append((out.cpu().reshape(-1), ref.reshape(-1), (mag * floor).reshape(-1)))
    kr.assert_bf16_close(*(torch.cat(t) for t in zip(*pooled)), floor_ulps=1, max_mismatch=0.01,
                         what=f"attention_small Dh{Dh} Nk{Nk} items{B * H * Nq} fused{fused} all kinds")


# ---------------------------------------------------------------- ln3d_triplane_axis_attention
def _axis_case(o, B, p, H, pad, spiked):
    rows, D = B * 3 * p * p, H * 64
    g = _gen("axis", B, p, H, pad, spiked)
    qkv = torch.randn(rows, 3 * D + pad, generator=g)
    if spiked:
        qkv[:, :2 * D] *= 4.0                                   # scores of std 16: a few keys carry each row
    buf, out = _nan_buf(rows * D, BF)
    o.triplane_axis_attention(qkv.to(DEV), out.view(rows, D), B, p, H)
    ref, mag, floor = kr.triplane_axis_attention(qkv, B, p, H, 64 ** -0.5)
    kr.assert_bf16_close(out, ref, mag * floor, floor_ulps=1, max_mismatch=0.01, what=f"axis_attention B{B} p{p} H{H} pad{pad} spiked{spiked}")
    _tail_untouched(buf)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("p", [1, 2, 5, 16, 31, 32])
def test_triplane_axis_attention(o, p, H, B):
    """ln3d_triplane_axis_attention: 2p keys per query from p = 1 (two keys) to 32 (all 64 lanes score), ld == 192 H with plain
    scores and ld padded by 40 with spiked ones.  Bound: 1 bf16 ulp, floor per row (kernel_refs.attention_floor with Nk = 2p,
    n_dot = 2 * 64 + 1: fp32 x fp32 products are rounded, a product and an add rounding per term); mismatch <= 1 %.
    Measured: worst 0.51 of the bound, mismatch at most 1.3e-3."""
    _axis_case(o, B, p, H, 0, False)
    _axis_case(o, B, p, H, 40, True)


def test_triplane_axis_attention_rows_beyond_the_grid_y_limit(o):
    """B = 22, p = 32: 67584 token rows.  The launch used to put the rows on gridDim.y, whose limit is 65536 (the device reports
    maxGridSize = (2147483647, 65536, 65536)); they are on gridDim.x now."""
    _axis_case(o, 22, 32, 1, 0, False)


# ---------------------------------------------------------------- ln3d_geglu, ln3d_mix_prediction
@pytest.mark.parametrize("inner", [1, 96, 1280])
@pytest.mark.parametrize("rows", [1, 37])
def test_geglu(o, rows, inner):
    """ln3d_geglu: gates swept over [-12, 12] with exact 0 and -0 and the region below -4, where 1 + erf cancels to zero in fp32; `a`
    of both signs.  Bound: 1 bf16 ulp, floor 8 fp32 ulps of |a| 0.5 |g| (1 + |erf(g / sqrt 2)|): erff within 4 ulps (the HIP
    device-function maximum), the argument's product with 1 / sqrt 2 one, the sum and the three products half an ulp each.
    Mismatch <= 1 % over gates >= -1, where 1 + erf >= 0.31 does not cancel.  Measured: worst 0.51 of the bound, mismatch 0."""
    n = rows * inner
    g = _gen("geglu", rows, inner)
    gate = torch.linspace(-12, 12, n) if n > 1 else torch.tensor([-0.0])
    gate = gate[torch.randperm(n, generator=g)].reshape(rows, inner).clone()
    if n > 2:
        gate.view(-1)[0], gate.view(-1)[n // 2] = 0.0, -0.0
    a = torch.randn(rows, inner, generator=g) * 2
    x = torch.cat([a, gate], 1).contiguous()
    buf, y = _nan_buf(n, BF)
    o.geglu(x.to(DEV), y, rows, inner)
    ref, scale = kr.geglu(x, inner)
    kr.assert_bf16_close(y, ref, scale, floor_ulps=8, max_mismatch=0.01, what=f"geglu rows{rows} inner{inner}", flips_over=gate >= -1)
    _tail_untouched(buf)


@pytest.mark.parametrize("HW", [1, 35])
def test_mix_prediction(o, HW):
    """ln3d_mix_prediction, in place on eps: logits that saturate the sigmoid both ways, 7 channels (not a power of two), x and eps of
    opposite sign with the two terms cancelling for the moderate logits.  Bound: 8 fp32 ulps of
    |c x| + s (|c x| + |eps|) (1 + |logit| / 8) (kernel_refs.mix_prediction).  Measured: 0.58 ulps."""
    N, Cc, c = 2, 7, 0.8
    g = _gen("mix", HW)
    logit = torch.tensor([-100.0, -30.0, -2.0, 0.0, 2.0, 30.0, 100.0])
    x = torch.randn(N, Cc, HW, generator=g) * 2
    s = torch.sigmoid(logit)[None, :, None]
    cancel = -(1 - s) * c * x / s.clamp(min=1e-3) * (1 + 1e-3 * torch.randn(N, Cc, HW, generator=g))
    eps = torch.where(logit.abs()[None, :, None] <= 2, cancel, -torch.sign(x) * torch.randn(N, Cc, HW, generator=g).abs())
    buf, e = _with_tail(eps)
    o.mix_prediction(e, x.to(DEV), logit.to(DEV), c, N, Cc, HW)
    kr.assert_f32_close(e, *kr.mix_prediction(eps, x, logit, c), 8, what=f"mix_prediction HW{HW}")
    _tail_untouched(buf)


# ---------------------------------------------------------------- im2col gathers (bitwise)
def _im2col_ref(xp, Ho, Wo, stride, Kpad):
    """xp: padded channel-last input [N, Hp, Wp, C] -> [N*Ho*Wo, Kpad], K index (ky*3 + kx)*C + c"""
    N, _, _, Cc = xp.shape
    taps = [xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :] for ky in range(3) for kx in range(3)]
    ref = torch.zeros(N * Ho * Wo, Kpad, dtype=xp.dtype)
    ref[:, :9 * Cc] = torch.cat(taps, -1).reshape(N * Ho * Wo, 9 * Cc)
    return ref


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("extra", [0, 24])
@pytest.mark.parametrize("Cc", [8, 16, 320])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 8), (8, 7), (32, 32)])
@pytest.mark.parametrize("stride", [1, 2])
def test_im2col3x3_strided(o, stride, H, W, Cc, extra, N):
    """ln3d_im2col3x3_strided (padding 1 on every side; Downsample.op of the U-Net with stride 2), bitwise, on rectangular and
    one-pixel images, Kpad == 9C and 9C + 24."""
    Kpad = 9 * Cc + extra
    x = torch.randn(N, H, W, Cc, generator=_gen("i2s", stride, H, W, Cc, N)).to(BF)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    buf, col = _nan_buf(N * Ho * Wo * Kpad, BF)
    o.im2col3x3_strided(x.to(DEV), col, N, H, W, Cc, stride, Kpad)
    _bits_equal(col, _im2col_ref(F.pad(x, (0, 0, 1, 1, 1, 1)), Ho, Wo, stride, Kpad))
    _tail_untouched(buf)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Cc,extra", [(8, 0), (64, 16)])
@pytest.mark.parametrize("H,W", [(2, 2), (7, 8), (8, 7), (32, 32)])
def test_im2col3x3_pad01(o, H, W, Cc, extra, N):
    """ln3d_im2col3x3_pad01 (the encoder's Downsample: zero row / column on the bottom / right only, stride 2), bitwise."""
    Kpad = 9 * Cc + extra
    x = torch.randn(N, H, W, Cc, generator=_gen("i2p", H, W, Cc, N)).to(BF)
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    buf, col = _nan_buf(N * Ho * Wo * Kpad, BF)
    o.im2col3x3_pad01(x.to(DEV), col, N, H, W, Cc, Kpad)
    _bits_equal(col, _im2col_ref(F.pad(x, (0, 0, 0, 1, 0, 1)), Ho, Wo, 2, Kpad))
    _tail_untouched(buf)


@pytest.mark.parametrize("Cc", [4, 32])
@pytest.mark.parametrize("H,W", [(9, 13), (13, 9), (64, 64)])
@pytest.mark.parametrize("plane", [0, 1, 2])
def test_im2col3x3_rollout(o, plane, H, W, Cc):
    """ln3d_im2col3x3_rollout, bitwise after the bf16 cast: [x_i | rowmean of plane (i+1) % 3 at y | colmean of plane (i+2) % 3 at x],
    the three sources and the three planes of each in disjoint value ranges, Kpad = 27C + 12."""
    Kpad = 27 * Cc + 12
    g = _gen("i2r", plane, H, W, Cc)
    off = torch.tensor([0.0, 100.0, 200.0])
    x = torch.randn(3, H, W, Cc, generator=g) + off[:, None, None, None]
    rm = 1000 + torch.rand(3, H, Cc, generator=g) + off[:, None, None]
    cm = -1000 - torch.rand(3, W, Cc, generator=g) - off[:, None, None]
    buf, col = _nan_buf(H * W * Kpad, BF)
    o.im2col3x3_rollout(x.to(DEV), rm.to(DEV), cm.to(DEV), col, plane, H, W, Cc, Kpad)
    inp = torch.cat([x[plane], rm[(plane + 1) % 3][:, None, :].expand(H, W, Cc), cm[(plane + 2) % 3][None, :, :].expand(H, W, Cc)], -1)
    _bits_equal(col, _im2col_ref(F.pad(inp[None], (0, 0, 1, 1, 1, 1)), H, W, 1, Kpad).to(BF))
    _tail_untouched(buf)


def _special_f32(n, g):
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F80FFFF, 0x3F808001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
            0x7F7F0000, 0x00008000]                                # bf16 rounding ties both ways, +-inf, +-0, the largest bf16, a subnormal
    sp = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(F32)
    x = torch.randn(n, generator=g) * 10
    idx = torch.randperm(n, generator=g)[:min(n, sp.numel())]
    x[idx] = sp[:idx.numel()]
    return x


@pytest.mark.parametrize("HW", [1, 35])
@pytest.mark.parametrize("Cc,Cpad", [(12, 12), (12, 16)])
def test_nchw_cl_layouts(o, Cc, Cpad, HW):
    """ln3d_nchw_to_cl_bf16 (channels zero-padded to Cpad) and ln3d_cl_to_nchw_f32, bitwise, with +-inf, +-0 and fp32 values on bf16
    rounding ties among the data."""
    N = 3
    x = _special_f32(N * Cc * HW, _gen("lay", Cc, Cpad, HW)).view(N, Cc, HW)
    buf, y = _nan_buf(N * HW * Cpad, BF)
    o.nchw_to_cl_bf16(x.to(DEV), y, N, Cc, HW, Cpad)
    ref = torch.zeros(N, HW, Cpad, dtype=BF)
    ref[:, :, :Cc] = x.transpose(1, 2).to(BF)
    _bits_equal(y, ref)
    cl = x.transpose(1, 2).contiguous()                            # [N, HW, C]
    buf2, back = _nan_buf(N * Cc * HW)
    o.cl_to_nchw_f32(cl.to(DEV), back, N, Cc, HW)
    _bits_equal(back, x)
    _tail_untouched(buf, buf2)


@pytest.mark.parametrize("B,S,P,Cc", [(1, 16, 4, 128), (2, 3, 2, 12), (1, 1, 1, 4), (1, 5, 3, 8)])
def test_sr_unpatchify(o, B, S, P, Cc):
    """ln3d_sr_unpatchify: `planes` bitwise, `mixed` (the short_cut's x.reshape(B, C, 3, L) view) bitwise after the bf16 cast."""
    R = S * P
    pred = torch.randn(B, 3 * S * S, P * P * Cc, generator=_gen("sru", B, S, P, Cc))
    n = B * 3 * R * R * Cc
    bp, planes = _nan_buf(n)
    bm, mixed = _nan_buf(n, BF)
    o.sr_unpatchify(pred.to(DEV), planes, mixed, B, S, P, Cc)
    ref = pred.view(B, 3, S, S, P, P, Cc).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, 3, R, R, Cc)
    _bits_equal(planes, ref)
    mref = ref.permute(0, 2, 3, 1, 4).reshape(B, R, R, Cc, 3).permute(0, 4, 1, 2, 3)       # [.., f = 3k + e] -> [b, e, Y, X, k]
    _bits_equal(mixed, mref.contiguous().to(BF))
    _tail_untouched(bp, bm)


# ---------------------------------------------------------------- bilinear resize
RESIZE_SHAPES = [(64, 64, 256, 256), (7, 7, 29, 29), (5, 9, 13, 22), (9, 5, 22, 13), (29, 13, 7, 5), (1, 1, 4, 6), (10, 10, 10, 10)]


def _ramp_noise(N, h, w, Cc, g):
    """a smooth ramp (different slopes along y and x) plus noise"""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
    return (0.7 * yy - 0.3 * xx + 2.0)[None, :, :, None] + 0.25 * torch.randn(N, h, w, Cc, generator=g)


@pytest.mark.parametrize("Cc,N", [(4, 3), (8, 1), (128, 1)])
@pytest.mark.parametrize("h,w,Ho,Wo", RESIZE_SHAPES)
def test_resize_bilinear_cl(o, h, w, Ho, Wo, Cc, N):
    """ln3d_resize_bilinear_cl on rectangular, non-dyadic, shrinking, one-pixel and identity sizes; transpose = 1 on the square ones.
    Reference: ATen's fp32 taps blended in float64 (kernel_refs.resize_bilinear).  Bound: 1 bf16 ulp, floor 4 fp32 ulps of the four
    weighted magnitudes + (src_y + src_x) amax / 4 (two weight complements, four products and three sums at half an ulp each, and
    one ulp of the source index on its weight); mismatch <= 1 %.  Measured: worst 0.50 of the bound (0.53 bf16 ulp), mismatch at most 2.7e-5."""
    x = _ramp_noise(N, h, w, Cc, _gen("rsz", h, w, Ho, Wo, Cc, N))
    ref, scale = kr.resize_bilinear(x, Ho, Wo)
    for transpose in ([False, True] if (h == w and Ho == Wo) else [False]):
        buf, y = _nan_buf(N * Ho * Wo * Cc, BF)
        o.resize_bilinear_cl(x.to(DEV), y, N, h, w, Ho, Wo, Cc, transpose=transpose)
        r, s = (ref.transpose(1, 2), scale.transpose(1, 2)) if transpose else (ref, scale)
        kr.assert_bf16_close(y, r.contiguous(), s.contiguous(), floor_ulps=4, max_mismatch=0.01,
                             what=f"resize_bilinear_cl {h}x{w}->{Ho}x{Wo} C{Cc} N{N} T{transpose}")
        _tail_untouched(buf)


@pytest.mark.parametrize("slope", [0.01, 0.2])
@pytest.mark.parametrize("Cc,N", [(4, 3), (8, 1), (128, 1)])
@pytest.mark.parametrize("h,w,Ho,Wo", RESIZE_SHAPES)
def test_resize_add_lrelu(o, h, w, Ho, Wo, Cc, N, slope):
    """ln3d_resize_add_lrelu = resize(base) + leaky_relu(t): the same sizes (10 x 10 -> 10 x 10 takes the h == Ho shortcut), t with
    exact +-0.  Bound: 6 fp32 ulps of the resize's scale + |leaky_relu(t)| (the resize's 4, the slope product and the sum).
    Measured: 1.30 ulps."""
    g = _gen("ral", h, w, Ho, Wo, Cc, N, slope)
    base = _ramp_noise(N, h, w, Cc, g)
    t = torch.randn(N, Ho, Wo, Cc, generator=g) * 3
    t[..., 0], t[..., 1] = 0.0, -0.0
    buf, out = _nan_buf(N * Ho * Wo * Cc)
    o.resize_add_lrelu(base.to(DEV), t.to(DEV), out, N, h, w, Ho, Wo, Cc, slope)
    kr.assert_f32_close(out, *kr.resize_add_lrelu(base, t, Ho, Wo, slope), 6, what=f"resize_add_lrelu {h}x{w}->{Ho}x{Wo} C{Cc} N{N} slope{slope}")
    _tail_untouched(buf)


# ---------------------------------------------------------------- sequential means
MEAN_CASES = [(H, W, Cc, N) for (H, W) in [(1, 1), (9, 13), (13, 9), (256, 256)] for Cc in [1, 4, 32, 300] for N in [1, 3]
              if not (H == 256 and Cc >= 32 and N == 3)]                     # 256 x 256 x 300 x 3 in float64 is 0.5 GB per temporary


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,Cc,N", MEAN_CASES)
def test_rollout_means(o, H, W, Cc, N, dtype):
    """ln3d_rollout_means and ln3d_rollout_means_bf16 on rectangular planes (a row mean has W terms, a column mean H), 300 channels
    (threads stride the channels), even channels centred and odd ones offset by 1000 std.  Bound: (n - 1) / 2 + 1 fp32 ulps of
    sum |x| / n for n terms summed in order (kernel_refs.mean_over).  Measured: 8.5 ulps of the 128.5 at n = 256 (fp32 planes), 0.42 ulps (bf16 planes)."""
    x = torch.randn(N, H, W, Cc, generator=_gen("rm", H, W, Cc, N))
    x[..., 1::2] += 1000.0
    x = x.to(dtype)
    br, rowm = _nan_buf(N * H * Cc)
    bc, colm = _nan_buf(N * W * Cc)
    o.rollout_means(x.to(DEV), rowm, colm, N, H, W, Cc)
    kr.assert_f32_close(rowm, *kr.mean_over(x, 2), kr.mean_ulps(W), what=f"rollout_means row {H}x{W} C{Cc} N{N} {dtype}")
    kr.assert_f32_close(colm, *kr.mean_over(x, 1), kr.mean_ulps(H), what=f"rollout_means col {H}x{W} C{Cc} N{N} {dtype}")
    _tail_untouched(br, bc)


@pytest.mark.parametrize("HW", [1, 1024])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Fr", [1, 6, 8])
def test_frame_mean(o, Fr, B, HW):
    """ln3d_frame_mean: channel-last frames -> NCHW mean; (F - 1) / 2 + 1 fp32 ulps of sum |h| / F; half of the channels offset by
    1000 std.  Measured: 1.46 ulps (F = 8, bound 4.5)."""
    Cc, S = 24, math.isqrt(HW)
    h = torch.randn(B * Fr, S, S, Cc, generator=_gen("fm", Fr, B, HW))
    h[..., 1::2] += 1000.0
    buf, out = _nan_buf(B * Cc * HW)
    o.frame_mean(h.to(DEV).permute(0, 3, 1, 2), out, B, Fr, HW, Cc)
    ref, scale = kr.mean_over(h.reshape(B, Fr, HW, Cc), 1)
    kr.assert_f32_close(out, ref.transpose(1, 2).contiguous(), scale.transpose(1, 2).contiguous(), kr.mean_ulps(Fr), what=f"frame_mean F{Fr} B{B} HW{HW}")
    _tail_untouched(buf)


# ---------------------------------------------------------------- ln3d_mv_posterior
POST = ("mean", "logvar", "z", "latent_tok", "log_q", "entropy")


def _posterior(hip_lib, h, qw, qb, eps, B, Fr, HW, E=4):
    """the raw entry point, so that the six outputs can be NaN-filled buffers with tails; h [B*F, 6E, H, W] of any strides"""
    from ln3diff_amd import _lib as L
    bufs = {k: _nan_buf(B * E * 3 * HW) for k in POST}
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                        # noqa: E731
    L.check(hip_lib.ln3d_mv_posterior(p(h), C.c_int64(h.stride(0)), C.c_int64(h.stride(3)), C.c_int64(h.stride(1)), p(qw), p(qb), p(eps),
                                      *(p(bufs[k][1]) for k in POST), B, Fr, HW, E, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "mv_posterior")
    torch.cuda.synchronize()
    _tail_untouched(*(b for b, _ in bufs.values()))
    return {k: v for k, (_, v) in bufs.items()}


@pytest.mark.parametrize("with_eps", [False, True])
@pytest.mark.parametrize("channel_last", [False, True])
@pytest.mark.parametrize("Fr", [1, 6])
def test_mv_posterior(o, hip_lib, Fr, channel_last, with_eps):
    """ln3d_mv_posterior in both layouts the header names (NCHW, s_pix = 1, and channel-last frames), F = 1 and 6, mode (eps NULL:
    z == mean bitwise, log_q has ns = 0) and sampling; quant_conv scaled so that the pre-clamp logvars cover [-100, 100] (var from
    e^-20 to e^20); every seventh pixel with eps scaled by 1e-4 (|mean| / (std |eps|) up to 1e4 and beyond: z - mean cancels).
    255 pixels (B * HW off a multiple of the 256-thread block).  Bounds: kernel_refs.mv_posterior, F / 2 + 9 fp32 ulps of the
    propagated term magnitudes for every output.  Measured (ulps): mean 2.27, logvar 0.66, z and latent_tok 1.22, log_q 0.65,
    entropy 0.66."""
    B, E, Hh, Ww = 2, 4, 15, 17
    HW = Hh * Ww
    g = _gen("mvp", Fr, channel_last, with_eps)
    h = torch.randn(B * Fr, 6 * E, Hh, Ww, generator=g) * math.sqrt(Fr)             # pooled activations of unit std
    qw, qb = torch.randn(6 * E, 2 * E, generator=g) * 0.5, torch.randn(6 * E, generator=g)
    qw[3 * E:] *= 28.0                                              # logvar moments of std ~40
    eps = None
    if with_eps:
        eps = torch.randn(B, E, 3, HW, generator=g)
        eps[..., ::7] *= 1e-4
    hd = h.to(DEV)
    if channel_last:
        hd = hd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    out = _posterior(hip_lib, hd, qw.to(DEV), qb.to(DEV), None if eps is None else eps.to(DEV), B, Fr, HW)
    r = kr.mv_posterior(h.reshape(B * Fr, 6 * E, HW), qw, qb, eps, B, Fr)
    pre = r["logvar"][1] - r["logvar"][0].abs()
    assert float(r["logvar"][0].abs().max()) > 19.99 and float(pre.max()) > 100, "the inputs do not reach the soft clamp"
    for k in POST:
        kr.assert_f32_close(out[k], *r[k], r["ulps"], what=f"mv_posterior F{Fr} cl{channel_last} eps{with_eps} {k}")
    _bits_equal(out["latent_tok"], out["z"].view(B, E, 3, HW).permute(0, 2, 3, 1).contiguous())
    if not with_eps:
        _bits_equal(out["z"], out["mean"])


def test_mv_posterior_pooled_route_equals_frame_route(o, hip_lib):
    """ln3d_frame_mean + ln3d_mv_posterior(F = 1, NCHW) gives the bits of ln3d_mv_posterior over the channel-last frames."""
    B, Fr, E, S = 2, 6, 4, 8
    HW = S * S
    g = _gen("mvp-routes")
    h = torch.randn(B * Fr, S, S, 6 * E, generator=g).to(DEV).permute(0, 3, 1, 2)
    qw, qb, eps = torch.randn(6 * E, 2 * E, generator=g).to(DEV), torch.randn(6 * E, generator=g).to(DEV), torch.randn(B, E, 3, HW, generator=g).to(DEV)
    pooled = torch.empty(B, 6 * E, S, S, device=DEV)
    o.frame_mean(h, pooled, B, Fr, HW, 6 * E)
    a = _posterior(hip_lib, h, qw, qb, eps, B, Fr, HW)
    b = _posterior(hip_lib, pooled, qw, qb, eps, B, 1, HW)
    for k in POST:
        _bits_equal(a[k], b[k])


# ---------------------------------------------------------------- DiT boundary: patch embed, final layer, per-head RMSNorm
@pytest.mark.parametrize("D", [128, 1152])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("Bx,Bn", [(1, 1), (2, 4), (3, 3)])
@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("Cc,p", [(4, 2), (16, 2), (4, 4)])
def test_patch_embed(o, Cc, p, G, Bx, Bn, with_scale, D):
    """ln3d_patch_embed: patch sizes 16 and 64 (the limit), token counts 3, 27 and 768 per sample (3 and 27 off a multiple of the 8
    tokens per block), the Bn > Bx wrap (b % Bx) on its own and with the input scale.  Bound: C p p / 2 + 2 fp32 ulps of
    sum |w s x| + |bias| + |pos| (a chain of C p p fma; the input scale; the bias and pos adds).  Measured: 4.51 ulps (C p p = 64, bound 34)."""
    S, L = G * p, G * G
    g = _gen("pe", Cc, p, G, Bx, Bn, with_scale, D)
    x = torch.randn(Bx, Cc * 3, S, S, generator=g)
    sc = 0.5 + torch.rand(Bn, generator=g) if with_scale else None
    w, bias, pos = torch.randn(D, Cc, p, p, generator=g) * 0.3, torch.randn(D, generator=g), torch.randn(3 * L, D, generator=g)
    buf, tok = _nan_buf(Bn * 3 * L * D)
    o.patch_embed(x.to(DEV), None if sc is None else sc.to(DEV), w.to(DEV), bias.to(DEV), pos.to(DEV), tok, Bx, Bn, Cc, S, p, D)
    ref, mag = kr.patch_embed(x, sc, w, bias, pos, Bn, p)
    kr.assert_f32_close(tok, ref, mag, Cc * p * p / 2 + 2, what=f"patch_embed C{Cc} p{p} G{G} Bx{Bx} Bn{Bn} scale{with_scale} D{D}")
    _tail_untouched(buf)


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("Bn,G", [(1, 1), (3, 1), (2, 16)])
@pytest.mark.parametrize("D", [128, 768, 1152])
def test_final_layer(o, D, Bn, G, p, tables):
    """ln3d_final_layer: 3 and 9 tokens (odd: the second token of the last wave is the ntok - 1 clamp) and 1536, every third token row
    at |mean| / std = 300, shift / scale read from a [Bn, 2 D + 64] buffer (mod_ld > 2 D), PixArt tables NULL and given, p 1 and 2.
    Bound: D / 128 + 8 fp32 ulps of sum_d |w_od| mag_d + |bias| (kernel_refs.final_layer).  Measured: 0.49 ulps."""
    Cc, S, L = 4, G * p, G * G
    ntok, NO, mod_ld = Bn * 3 * L, p * p * Cc, 2 * D + 64
    g = _gen("fl", D, Bn, G, p, tables)
    tokens = _offset_rows(torch.randn(ntok, D, generator=g) + 0.3, D + ntok)
    mod = torch.randn(Bn, mod_ld, generator=g) * 0.5
    st, sct = (0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)) if tables else (None, None)
    w, bias = torch.randn(NO, D, generator=g) * D ** -0.5, torch.randn(NO, generator=g)
    md = mod.to(DEV)
    buf, out = _nan_buf(Bn * Cc * 3 * S * S)
    o.final_layer(tokens.to(DEV), md[:, :D], md[:, D:2 * D], mod_ld, None if st is None else st.to(DEV), None if sct is None else sct.to(DEV),
                  w.to(DEV), bias.to(DEV), out, Bn, Cc, S, p, D)
    ref, mag = kr.final_layer(tokens, mod[:, :D], mod[:, D:2 * D], st, sct, w, bias, Bn, Cc, S, p)
    kr.assert_f32_close(out, ref, mag, D / 128 + 8, what=f"final_layer D{D} Bn{Bn} G{G} p{p} tables{tables}")
    _tail_untouched(buf)


@pytest.mark.parametrize("rows", [1, 3, 17, 1000])
@pytest.mark.parametrize("Dh,true_dim", [(64, 0), (80, 72), (80, 0), (128, 72), (128, 0)])
def test_rmsnorm_heads(o, Dh, true_dim, rows):
    """ln3d_rmsnorm_heads_bf16, in place: 16 lanes per row at Dh 64, 32 at Dh 80 (12 of them idle in the butterfly) and 128; heads of
    true width 72 stored zero-padded (the padding of x and w zero, and zero afterwards); rows * lanes off a multiple of 256; an
    all-zero row; rows scaled by 2^60 and 2^-60.  Bound: 1 bf16 ulp, floor 8 fp32 ulps of |y| (four squares and five butterfly
    levels on a positive sum: 4.5 ulps, halved by the square root; rsqrt 2; the division, the eps add and two products);
    mismatch <= 1 %.  Measured: worst 0.50 of the bound, mismatch at most 3.1e-5."""
    eps, td = 1e-5, true_dim or Dh
    g = _gen("rmsh", Dh, true_dim, rows)
    x = torch.randn(rows, Dh, generator=g)
    w = 1 + 0.2 * torch.randn(Dh, generator=g)
    x[:, td:], w[td:] = 0.0, 0.0
    if rows >= 3:
        x[1] = 0.0
        x[0] *= 2.0 ** 60
        x[2] *= 2.0 ** -60
    x = x.to(BF)
    buf, xd = _with_tail(x)
    o.rmsnorm_heads(xd, w.to(DEV), rows, Dh, eps=eps, true_dim=true_dim)
    ref, mag = kr.rmsnorm_heads(x, w, eps, true_dim)
    kr.assert_bf16_close(xd, ref, mag, floor_ulps=8, max_mismatch=0.01, what=f"rmsnorm_heads Dh{Dh} true{true_dim} rows{rows}")
    assert bool((xd[:, td:] == 0).all()) and (rows < 3 or bool((xd[1] == 0).all()))
    _tail_untouched(buf)
