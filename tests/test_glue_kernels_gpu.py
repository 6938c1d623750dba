"""The small glue kernels of include/ln3d.h, each against a float64 restatement (tests/kernel_refs.py) at the shapes, types and edges
where they go wrong.  bf16 outputs: every element within 1 bf16 ulp of the float64 value (floor: a few fp32 ulps of the magnitude of
the terms that were summed) and a bounded fraction of elements off the correctly rounded value; fp32 outputs: a few fp32 ulps of the
terms; layout / gather kernels: bitwise equal to the torch expression.  None of these kernels touches the GEMM, so the tile-forcing
`ops` fixture of test_kernels_gpu.py is not used.

Measured worst cases on gfx950 are noted beside each bound ("measured: ...")."""
import math
import zlib

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def o(hip_lib):
    from ln3diff_amd import ops
    return ops


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _offset_groups(x, groups, seed):
    """x f32 [N, HW, C] (CPU) -> the same with per-(sample, group) std in [0.5, 3] and |mean| / std of 0, 100 or 1000 (groups
    g % 8 == 1, 2), and one constant group (g % 8 == 3, the value 1.3 - not a power of two; var = 0)."""
    g = torch.Generator().manual_seed(seed)
    N, HW, C = x.shape
    cpg = C // groups
    xg = x.reshape(N, HW, groups, cpg).clone()
    for n in range(N):
        for k in range(groups):
            std = 0.5 + 2.5 * float(torch.rand(1, generator=g))
            ratio = {1: 100.0, 2: 1000.0}.get(k % 8, 0.0)
            sign = 1.0 if (n + k) % 2 else -1.0
            xg[n, :, k] = xg[n, :, k] * std + sign * ratio * std
            if k % 8 == 3:
                xg[n, :, k] = 1.3
    return xg.reshape(N, HW, C)


def _centred_groups(N, HW, C, groups, constant=True):
    """mask [N, HW, C] of the groups _offset_groups leaves near zero mean (the mismatch fraction is taken over these); constant=False
    also leaves out the constant groups"""
    off = torch.tensor([1, 2] if constant else [1, 2, 3])
    return ~torch.isin((torch.arange(C) // (C // groups)) % 8, off)[None, None, :].expand(N, HW, C)


def _centred_rows(rows, D):
    r = torch.arange(rows)
    return ((r % 3 != 0) & (r % 5 != 1))[:, None].expand(rows, D)


# ---------------------------------------------------------------- normalisations
@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("HW", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_groupnorm_swish(o, C, HW, N, swish):
    """ln3d_groupnorm_swish (ldm model.py:45-51) at every C it accepts, HW around LN3D_GN_PIXELS_PER_CHUNK (256) and groups far off
    zero mean.  Bound: 1 bf16 ulp, floor 16 fp32 ulps of (|x| + |mean|) / std * |w| + |b| (a chunk's M2 is a sequential fp32 sum of
    up to C pixels per thread, which reaches the output through rstd); mismatch <= 1 % over the centred groups.  Measured: worst 0.79
    of the bound, mismatch 1.6e-4.  The one-pass E[x^2] - mean^2 kernel failed 78 of these 82 cases (up to 119x the bound)."""
    _groupnorm_swish_case(o, C, HW, N, swish)


@pytest.mark.parametrize("C", [32, 64])
def test_groupnorm_swish_decoder_size(o, C):
    """256 x 256 pixels: 256 chunks of LN3D_GN_PIXELS_PER_CHUNK merged per group (the decoder's planes are up to 128 x 128)."""
    _groupnorm_swish_case(o, C, 256 * 256, 1, 1)


def _groupnorm_swish_case(o, C, HW, N, swish, groups=32, eps=1e-6):
    g = _gen("gn", C, HW, N, swish)
    x = _offset_groups(torch.randn(N, HW, C, generator=g), groups, C + HW + N)
    w, b = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    y = torch.empty(N * HW, C, dtype=torch.bfloat16, device=DEV)
    st = torch.full((N * groups * 2 * (1 + (HW + 255) // 256),), float("nan"), device=DEV)     # include/ln3d.h scratch size
    o.groupnorm_swish(x.to(DEV), w.to(DEV), b.to(DEV), y, st, N, HW, C, groups, eps, bool(swish))
    ref, scale = kr.groupnorm(x, w, b, groups, eps, swish)
    kr.assert_bf16_close(y, ref, scale, floor_ulps=16, max_mismatch=0.01, what=f"groupnorm_swish C{C} HW{HW} N{N} swish{swish}",
                         flips_over=_centred_groups(N, HW, C, groups))
    if not swish:     # the constant groups (var = 0) are exactly their bias: (x - mean) == 0, nothing amplified by rsqrt(eps)
        const = (torch.arange(C) // (C // groups)) % 8 == 3
        assert torch.equal(y.view(N, HW, C)[:, :, const].cpu(), b[const].to(torch.bfloat16).expand(N, HW, -1))


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("extra", ["plain", "add_row", "mod", "add_row+mod"])
@pytest.mark.parametrize("C,HW", [(320, 16), (320, 1000), (1280, 4), (1280, 100)])
def test_groupnorm_any(o, C, HW, extra, swish):
    """ln3d_groupnorm_any (the U-Net's GroupNorm; guided_diffusion/unet.py:267-273): cpg 10 and 40 (not powers of two), HW * cpg 160
    (< 256 threads) and several thousand, the same far-off-zero groups, add_row and mod_scale / mod_shift.  Pins the round-6 fix
    (two centred passes).  Bound: 1 bf16 ulp, floor 4 fp32 ulps of the terms; measured worst 0.65 of the bound.  Mismatch <= 1 % over
    the centred groups; the constant groups are left out of it: their fp32 mean is off by a rounding error that rsqrt(eps) amplifies
    to ~3e-5 absolute (within the element bound, but 2-5 % of those outputs flip, unlike ln3d_groupnorm_swish, whose pivoted sums
    give x - mean == 0 there)."""
    N, groups, eps = 2, 32, 1e-5
    g = _gen("gna", C, HW, extra, swish)
    x = _offset_groups(torch.randn(N, HW, C, generator=g), groups, C + HW)
    w, b = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    ar = torch.randn(N, C, generator=g) if "add_row" in extra else None
    ms, mh = (0.5 * torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)) if "mod" in extra else (None, None)
    y = torch.empty(N * HW, C, dtype=torch.bfloat16, device=DEV)
    dv = lambda t: None if t is None else t.to(DEV)                                                       # noqa: E731
    o.groupnorm_any(x.to(DEV), w.to(DEV), b.to(DEV), y, N, HW, C, groups, eps, bool(swish), add_row=dv(ar), mod_scale=dv(ms), mod_shift=dv(mh))
    ref, scale = kr.groupnorm(x, w, b, groups, eps, swish, add_row=ar, mod_scale=ms, mod_shift=mh)
    kr.assert_bf16_close(y, ref, scale, floor_ulps=4, max_mismatch=0.01, what=f"groupnorm_any C{C} HW{HW} {extra} swish{swish}",
                         flips_over=_centred_groups(N, HW, C, groups, constant=False))


def _offset_rows(x, seed):
    """every third row moved to |mean| / std = 300, every fifth (from row 1) to 1000 - see _centred_rows"""
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    x[::3] += 300 * x[::3].std() * torch.sign(torch.randn(x[::3].shape[0], 1, generator=g))
    x[1::5] -= 1000 * x[1::5].std()
    return x


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("D", [128, 768, 1024, 1152])
def test_layernorm_f32(o, D, affine, inplace):
    """ln3d_layernorm_f32 (CLIP final_layer_norm; in place as sgm/image_encoders.py calls it): 37 rows (not a multiple of the 4 rows
    per block), offset rows.  Bound: 8 fp32 ulps of (|x| + |mean|) / std * |w| + |b| (two fp32 reductions of D terms each feed the
    output); measured worst 2.15 ulps."""
    rows, eps = 37, 1e-5
    g = _gen("ln", D, affine, inplace)
    x = _offset_rows(torch.randn(rows, D, generator=g) * 2 + 0.5, D)
    w, b = (1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)) if affine else (None, None)
    xd = x.to(DEV)
    y = xd if inplace else torch.full((rows + 1, D), 7.0, device=DEV)
    o.layernorm_f32(xd, None if w is None else w.to(DEV), None if b is None else b.to(DEV), y, rows, D, eps)
    ref, scale = kr.layernorm(x, w, b, eps)
    kr.assert_f32_close(y[:rows], ref, scale, 8, what=f"layernorm_f32 D{D} affine{affine} inplace{inplace}")
    if not inplace:
        assert bool((y[rows] == 7.0).all())


@pytest.mark.parametrize("mod", [False, True])
@pytest.mark.parametrize("D,kind", [(512, 0), (1024, 1), (1536, 0), (1536, 1), (128, 1), (768, 0), (1152, 0), (1152, 1), (1280, 0),
                                    (1280, 1)])
def test_norm_modulate_paths(o, D, kind, mod):
    """ln3d_norm_modulate through its three template paths (<2,true> D 512 / 1024, <3,true> 1536, <3,false> 128 / 768 / 1152 / 1280),
    LayerNorm and RMSNorm * weight, offset rows, per-sample shift / scale read at (r / mod_rows) * mod_ld with tables added, and the
    rows_in -> rows_out remap (rows between the samples' blocks stay untouched).  test_kernels_gpu.py::test_norm_modulate stays as it
    is.  Bound: 1 bf16 ulp, floor 4 fp32 ulps of the terms; mismatch <= 1 % over the centred rows.  Measured worst 0.57 of the bound,
    mismatch 1.8e-4."""
    S, rows_in, rows_out, eps = 3, 11, 14, 1e-6
    rows = S * rows_in
    g = _gen("nm", D, kind, mod)
    x = _offset_rows(torch.randn(rows, D, generator=g) + 0.3, D + kind)
    weight = 1 + 0.2 * torch.randn(D, generator=g) if kind == 1 else None
    kw = {}
    ref_kw = {}
    if mod:
        mod_rows, mod_ld = rows_in, 3 * D                       # the [B, 6D]-style adaLN buffer: shift / scale are column slices
        buf = torch.randn(S, mod_ld, generator=g) * 0.5
        shift, scale = buf[:, :D], buf[:, D:2 * D]
        st, sct = 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
        bd = buf.to(DEV)
        kw = dict(shift=bd[:, :D], scale=bd[:, D:2 * D], mod_rows=mod_rows, mod_ld=mod_ld, shift_table=st.to(DEV), scale_table=sct.to(DEV))
        ref_kw = dict(shift=shift, scale=scale, mod_rows=mod_rows, shift_table=st, scale_table=sct)
    y = torch.full((S * rows_out, D), 7.0, dtype=torch.bfloat16, device=DEV)
    o.norm_modulate(x.to(DEV), y, rows, D, kind=kind, eps=eps, weight=None if weight is None else weight.to(DEV), rows_in=rows_in,
                    rows_out=rows_out, **kw)
    ref, mag = kr.norm_modulate(x, kind, eps, weight=weight, **ref_kw)
    yv = y.view(S, rows_out, D)
    kr.assert_bf16_close(yv[:, :rows_in], ref.view(S, rows_in, D), mag.view(S, rows_in, D), floor_ulps=4, max_mismatch=0.01,
                         what=f"norm_modulate D{D} kind{kind} mod{mod}", flips_over=_centred_rows(rows, D))
    assert bool((yv[:, rows_in:] == 7.0).all())


# ---------------------------------------------------------------- sampler and ODE steps (fp32, elementwise)
NS = [1, 255, 257, 12 * 32 * 32 * 3 + 5]          # never a multiple of the 256-thread block


def _rand(n, seed, s=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * s * torch.exp(torch.randn(n, generator=g))     # magnitudes spread over a few decades


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_ddpm_step(o, n, clip):
    """ln3d_ddpm_step: bound 4 fp32 ulps of the terms; measured 1.18."""
    ab, ab_prev = 0.3, 0.34
    a, b = 1 / math.sqrt(ab), math.sqrt(1 / ab - 1)
    beta = 1 - ab / ab_prev
    c1, c2, sig = math.sqrt(ab_prev) * beta / (1 - ab), math.sqrt(1 - beta) * (1 - ab_prev) / (1 - ab), 0.2
    x, eps, noise = _rand(n, 1, 2.0), _rand(n, 2), _rand(n, 3)
    xd = x.to(DEV)
    o.ddpm_step(xd, eps.to(DEV), noise.to(DEV), a, b, c1, c2, sig, clip)
    ref, mag = kr.ddpm_step(x, eps, noise, *(float(torch.tensor(v, dtype=torch.float32)) for v in (a, b, c1, c2, sig)), clip)
    kr.assert_f32_close(xd, ref, mag, 4, what=f"ddpm_step n{n} clip{clip}")


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("n", NS)
def test_ddim_step(o, n, cfg, clip, noise):
    """ln3d_ddim_step in every combination of CFG, clip (eps re-derived per branch from the clipped x0, gaussian_diffusion.py) and noise.
    Bound: 8 fp32 ulps of the terms (the re-derived eps divides a difference of two terms by b); measured 1.58."""
    ab, ab_prev, eta = 0.3, 0.45, 0.5
    a, b = 1 / math.sqrt(ab), math.sqrt(1 / ab - 1)
    sigma = eta * math.sqrt((1 - ab_prev) / (1 - ab)) * math.sqrt(1 - ab / ab_prev)
    coef = math.sqrt(1 - ab_prev - sigma ** 2)
    s = 4.5
    x, eu, ec, nz = _rand(n, 4, 2.0), _rand(n, 5), _rand(n, 6), _rand(n, 7)
    f = [float(torch.tensor(v, dtype=torch.float32)) for v in (s, a, b, math.sqrt(ab_prev), coef, sigma)]
    xd = x.to(DEV)
    o.ddim_step(xd, eu.to(DEV), ec.to(DEV) if cfg else None, nz.to(DEV) if noise else None, *f, clip)
    ref, mag = kr.ddim_step(x, eu, ec if cfg else None, nz if noise else None, *f, clip)
    kr.assert_f32_close(xd, ref, mag, 8, what=f"ddim_step n{n} cfg{cfg} clip{clip} noise{noise}")


@pytest.mark.parametrize("n", NS)
def test_edm_flow_cfg_axpby(o, n):
    """ln3d_edm_euler_step, ln3d_flow_euler_step (both halves bitwise equal), ln3d_cfg_combine_dup (both halves bitwise equal) and
    ln3d_axpby in place.  Bound: 4 fp32 ulps of the terms (edm: 8 - to_d divides x - denoised by sigma); measured 1.33 (edm),
    0.94 (flow), 0.81 (cfg), 0.92 (axpby)."""
    sigma, sigma_next, s = 2.5, 1.75, 3.0
    x, e2 = _rand(n, 8, 3.0), _rand(2 * n, 9)
    xd = x.to(DEV)
    o.edm_euler_step(xd, e2.to(DEV), sigma, sigma_next, s)
    kr.assert_f32_close(xd, *kr.edm_euler_step(x, e2, sigma, sigma_next, s), 8, what=f"edm_euler_step n{n}")

    xh = _rand(n, 10)
    x2, v2 = torch.cat([xh, xh]), _rand(2 * n, 11)
    dt = float(torch.tensor(-1 / 37, dtype=torch.float32))
    x2d = x2.to(DEV)
    o.flow_euler_step(x2d, v2.to(DEV), dt, s)
    kr.assert_f32_close(x2d, *kr.flow_euler_step(x2, v2, dt, s), 4, what=f"flow_euler_step n{n}")
    assert torch.equal(x2d[:n], x2d[n:])

    vd = v2.to(DEV)
    o.cfg_combine_dup(vd, s)
    kr.assert_f32_close(vd, *kr.cfg_combine_dup(v2, s), 4, what=f"cfg_combine_dup n{n}")
    assert torch.equal(vd[:n], vd[n:])

    xa, ya = _rand(n, 12), _rand(n, 13)
    yd = ya.to(DEV)
    o.axpby(xa.to(DEV), yd, 0.75, -1.3)
    kr.assert_f32_close(yd, *kr.axpby(xa, ya, 0.75, float(torch.tensor(-1.3, dtype=torch.float32))), 4, what=f"axpby n{n}")


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("nterms", range(8))
def test_lincomb(o, nterms, with_y):
    """ln3d_lincomb (Runge-Kutta stage combination, up to 7 stages; y NULL = 0).  Bound: nterms + 2 fp32 ulps of the terms (one
    rounding per term); measured 1.59."""
    n = 257 + 12 * 32 * 32 * 3
    y = _rand(n, 20) if with_y else None
    ks = [_rand(n, 21 + j) for j in range(nterms)]
    cs = [float(torch.tensor(c, dtype=torch.float32)) for c in (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, -0.3)[:nterms]]
    out = torch.full((n + 4,), 7.0, device=DEV)
    ref, mag = kr.lincomb(y, ks, cs, n)
    o.lincomb(None if y is None else y.to(DEV), [k.to(DEV) for k in ks], cs, out[:n])
    kr.assert_f32_close(out[:n], ref, mag, nterms + 2, what=f"lincomb nterms{nterms} y{with_y}")
    assert bool((out[n:] == 7.0).all())


@pytest.mark.parametrize("with_y1", [False, True])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4 * 1024 * 1024 + 3])
def test_err_ratio_sq(o, n, with_y1):
    """ln3d_err_ratio_sq: one workgroup, fixed order - ceil(n / 1024) sequential adds per thread, a 6-level butterfly, 16 partials in
    order, and ~7 roundings per term before that: relative error <= (ceil(n / 1024) + 6 + 16 + 7) * 2^-24 (all terms positive).
    Bitwise equal over three calls (the adaptive solver's accept / reject decision reads it).  Measured at most 0.06 of the bound."""
    err, y0 = _rand(n, 30, 1e-3), _rand(n, 31)
    y1 = _rand(n, 32) if with_y1 else None
    atol, rtol = 1e-5, 1e-3
    acc = torch.zeros(3, device=DEV)
    args = [err.to(DEV), y0.to(DEV), None if y1 is None else y1.to(DEV)]
    for i in range(3):
        o.err_ratio_sq(*args, atol, rtol, acc[i:i + 1])
    a = acc.cpu()
    assert a[0].item() == a[1].item() == a[2].item(), a
    ref = kr.err_ratio_sq(err, y0, y1, float(torch.tensor(atol, dtype=torch.float32)), float(torch.tensor(rtol, dtype=torch.float32)))
    bound = (math.ceil(n / 1024) + 6 + 16 + 7) * 2.0 ** -24
    rel = abs(a[0].item() - ref) / ref
    print(f"[kref] err_ratio_sq n{n} y1{with_y1}: rel {rel:.3g} ({rel / bound:.3g} of the bound)")
    assert rel <= bound, (rel, bound)


# ---------------------------------------------------------------- layout, gather and embedding (bitwise)
def _bits_equal(y, ref):
    assert y.dtype == ref.dtype and y.shape == ref.shape, (y.dtype, ref.dtype, y.shape, ref.shape)
    v = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[y.dtype]
    assert torch.equal(y.detach().cpu().view(v), ref.detach().cpu().view(v))


@pytest.mark.parametrize("reps", [1, 3, 7])
def test_tile_rows_and_add_table_rows(o, reps):
    per = 4 * 77 * 3
    x = torch.randn(per)
    y = torch.full((reps * per + 8,), 7.0, device=DEV)
    o.tile_rows(x.to(DEV), y, per, reps)
    _bits_equal(y[:reps * per], x.repeat(reps))
    assert bool((y[reps * per:] == 7.0).all())
    layers, B, W = reps + 2, reps, 6 * 13 - 1                  # odd layers, B and W
    t0, tables = torch.randn(B, W), torch.randn(layers, W)
    out = torch.full((layers * B * W + 8,), 7.0, device=DEV)
    o.add_table_rows(t0.to(DEV), tables.to(DEV), out, layers, B, W)
    _bits_equal(out[:-8].view(layers, B, W), tables[:, None, :] + t0[None, :, :])
    assert bool((out[-8:] == 7.0).all())


@pytest.mark.parametrize("H,W", [(7, 7), (5, 13), (16, 16), (33, 9)])
def test_planes_layout_round_trip(o, H, W):
    NP, C = 2, 32
    nchw = torch.randn(NP, 3 * C, H, W)
    cl = torch.full((NP * 3 * H * W * C + 8,), 7.0, device=DEV)
    o.planes_to_channel_last(nchw.to(DEV), cl, NP, C, H, W)
    _bits_equal(cl[:-8].view(NP, 3, H, W, C), nchw.view(NP, 3, C, H, W).permute(0, 1, 3, 4, 2).contiguous())
    assert bool((cl[-8:] == 7.0).all())
    back = torch.full((NP * 3 * C * H * W + 8,), 7.0, device=DEV)
    o.planes_to_nchw(cl, back, NP, C, H, W)
    _bits_equal(back[:-8].view(NP, 3 * C, H, W), nchw)
    assert bool((back[-8:] == 7.0).all())


@pytest.mark.parametrize("upsample", [1, 2])
@pytest.mark.parametrize("C,Kpad", [(8, 80), (16, 160), (64, 576)])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 3)])          # 1 x 1 under upsample 2: every tap at or across an edge
def test_im2col3x3(o, C, Kpad, upsample, H, W):
    N = 2
    x = torch.randn(N, H, W, C).to(torch.bfloat16)
    Ho, Wo = H * upsample, W * upsample
    col = torch.full((N * Ho * Wo * Kpad + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    o.im2col3x3(x.to(DEV), col, N, H, W, C, upsample, Kpad)
    xu = x.repeat_interleave(upsample, 1).repeat_interleave(upsample, 2)                 # nearest 2x (ldm Upsample)
    xp = torch.nn.functional.pad(xu, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ky:ky + Ho, kx:kx + Wo, :] for ky in range(3) for kx in range(3)]
    ref = torch.zeros(N * Ho * Wo, Kpad, dtype=torch.bfloat16)
    ref[:, :9 * C] = torch.cat(taps, -1).reshape(N * Ho * Wo, 9 * C)
    _bits_equal(col[:-8].view(N * Ho * Wo, Kpad), ref)
    assert bool((col[-8:] == 7.0).all())


@pytest.mark.parametrize("C,S,Kpad", [(3, 28, 640), (9, 42, 1792)])
def test_vit_patchify(o, C, S, Kpad):
    B, p = 2, 14
    G = S // p
    img = torch.randn(B, C, S, S)
    out = torch.full((B * G * G * Kpad + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    o.vit_patchify(img.to(DEV), out, B, S, p, Kpad, C)
    ref = torch.zeros(B * G * G, Kpad, dtype=torch.bfloat16)
    ref[:, :C * p * p] = img.view(B, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, C * p * p).to(torch.bfloat16)
    _bits_equal(out[:-8].view(B * G * G, Kpad), ref)
    assert bool((out[-8:] == 7.0).all())


@pytest.mark.parametrize("R", [0, 4])
def test_vit_assemble(o, R):
    B, L, D = 3, 9, 96
    patch, cls, reg, pos = torch.randn(B, L, D), torch.randn(D), torch.randn(max(R, 1), D), torch.randn(1 + L, D)
    x = torch.full((B * (1 + R + L) * D + 8,), 7.0, device=DEV)
    o.vit_assemble(patch.to(DEV), cls.to(DEV), reg.to(DEV) if R else None, pos.to(DEV), x, B, L, R, D)
    parts = [(cls + pos[0]).expand(B, 1, D)] + ([reg[:R].expand(B, R, D)] if R else []) + [patch + pos[1:]]
    _bits_equal(x[:-8].view(B, 1 + R + L, D), torch.cat(parts, 1))
    assert bool((x[-8:] == 7.0).all())


def test_embed_tokens(o):
    B, T, D, vocab = 2, 7, 64, 50
    ids = torch.tensor([[0, vocab - 1, 5, -1, vocab, vocab + 100, -2 ** 31], [3, 3, vocab - 1, 0, 7, 1, 2 ** 31 - 1]], dtype=torch.int32)
    tok, pos = torch.randn(vocab, D), torch.randn(T, D)
    out = torch.full((B * T * D + 8,), 7.0, device=DEV)
    o.embed_tokens(ids.to(DEV), tok.to(DEV), pos.to(DEV), out, B, T, D)
    _bits_equal(out[:-8].view(B, T, D), tok[ids.long().clamp(0, vocab - 1)] + pos[None])
    assert bool((out[-8:] == 7.0).all())


def test_cast_f32_bf16_specials(o):
    """Round to nearest even against torch's x.to(bfloat16): exact ties both ways, the largest bf16, the halfway point above it
    (rounds to inf), +-inf, fp32 subnormals (ties included; measured: kept, not flushed).  NaN is documented as not special-cased and
    left out."""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F80FFFF, 0x3F808001,       # ties to even, just off the tie
            0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F8000, 0x7F800000, 0xFF800000,         # largest bf16, halfway above -> inf, +-inf
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008000, 0x807FFFFF,         # subnormals (ties, largest)
            0x00800000, 0x80000000, 0x00000000, 0x3DCCCCCD]
    special = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat([special, torch.randn(1002) * 10])                                          # n % 4 == 0
    y = torch.full((x.numel() + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    o.cast_bf16(x.to(DEV), y[:x.numel()])
    _bits_equal(y[:x.numel()], x.to(torch.bfloat16))
    assert bool((y[x.numel():] == 7.0).all())


@pytest.mark.parametrize("with_b,with_sum", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("act", [0, 1])
def test_add_act_cast(o, act, with_b, with_sum):
    """identity: bitwise equal to (a + b).to(bf16); SiLU: 1 bf16 ulp of the float64 silu of the fp32 sum, floor 4 fp32 ulps of
    |a + b| (measured worst 0.5 ulp); the optional fp32 sum bitwise."""
    n = 1001
    a, b = torch.randn(n) * 4, torch.randn(n) * 4
    y = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    s = torch.full((n + 8,), 7.0, device=DEV)
    o.add_act_cast(a.to(DEV), b.to(DEV) if with_b else None, y, s if with_sum else None, n, act)
    v = a + b if with_b else a
    if act == 0:
        _bits_equal(y[:n], v.to(torch.bfloat16))
    else:
        kr.assert_bf16_close(y[:n], kr.silu64(v.double()), v.abs(), floor_ulps=4, what=f"add_act_cast silu b{with_b}")
    if with_sum:
        _bits_equal(s[:n], v)
    assert bool((y[n:] == 7.0).all()) and bool((s[n if with_sum else 0:] == 7.0).all())


@pytest.mark.parametrize("dim", [256, 320])
def test_timestep_embedding(o, dim):
    """t up to 999.  Bound: 1 bf16 ulp, floor 32 fp32 ulps of |t * freq| - the kernel's frequency exp(-ln(1e4) k / half) is an fp32
    exp of an argument up to 9.2 (~30 ulps of relative error), and cos / sin pass that on as absolute error of the size of the
    argument.  Measured worst 0.5 of the bound, mismatch 8.9e-4."""
    t = torch.tensor([0.0, 1.0, 17.5, 250.0, 500.25, 998.0, 999.0])
    B = t.numel()
    out = torch.full((B * dim + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    o.timestep_embedding(t.to(DEV), out, B, dim)
    ref, arg = kr.timestep_embedding(t, dim)
    kr.assert_bf16_close(out[:-8].view(B, dim), ref, arg, floor_ulps=32, max_mismatch=0.05, what=f"timestep_embedding dim{dim}")
    assert bool((out[-8:] == 7.0).all())


@pytest.mark.parametrize("D", [200, 300])
def test_patch_embed_triplane(o, D):
    """PatchEmbedTriplane against F.conv2d(groups=3) + the literal regroup of vit/vit_triplane.py:82-106.  out_raw: 9 fp32 ulps of the
    sum of |terms| (a chain of Cg * p * p = 16 fma + the bias); SiLU output: 1 bf16 ulp, floor 12 fp32 ulps of the same.  Measured:
    raw 2.19 ulps, SiLU 0.51 of the bound, mismatch 6.5e-5."""
    B, Cg, S, p = 2, 4, 16, 2
    G = S // p
    g = _gen("pet", D)
    lat = torch.randn(B, 3 * Cg, S, S, generator=g)
    w, bias = torch.randn(3 * D, Cg, p, p, generator=g) * 0.3, torch.randn(3 * D, generator=g)
    sc = torch.full((B * 3 * G * G * D + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    raw = torch.full((B * 3 * G * G * D + 8,), 7.0, device=DEV)
    o.patch_embed_triplane(lat.to(DEV), w.to(DEV), bias.to(DEV), sc, raw, B, Cg, S, p, D)
    ref, mag = kr.patch_embed_triplane(lat, w, bias, p, D)
    kr.assert_f32_close(raw[:-8], ref, mag, 9, what=f"patch_embed_triplane raw D{D}")
    kr.assert_bf16_close(sc[:-8], kr.silu64(ref), mag, floor_ulps=12, what=f"patch_embed_triplane silu D{D}")
    assert bool((sc[-8:] == 7.0).all()) and bool((raw[-8:] == 7.0).all())
