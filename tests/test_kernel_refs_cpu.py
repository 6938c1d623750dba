"""The float64 references and per-element bounds of tests/kernel_refs.py can fail: a correctly rounded result passes, one bf16 ulp of
error or a one-pass fp32 GroupNorm variance does not.  No GPU needed."""
import pytest
import torch

import kernel_refs as kr


def _ref(n=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float64) * torch.logspace(-3, 3, n, dtype=torch.float64)


def test_bf16_rne_matches_torch_on_fp32_values():
    x = _ref().float()
    assert torch.equal(kr.bf16_rne(x.double()), x.to(torch.bfloat16).double())
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0x7F7F8000, 0x00008000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert torch.equal(kr.bf16_rne(ties.double()), ties.to(torch.bfloat16).double())


def test_correctly_rounded_result_passes():
    ref = _ref()
    worst, mism = kr.assert_bf16_close(kr.bf16_rne(ref), ref, what="rne")
    assert worst <= 0.5 and mism == 0.0


def test_one_ulp_relative_error_fails():
    ref = _ref()
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(kr.bf16_rne(ref * (1 + 2.0 ** -7)), ref, what="ref * (1 + 2^-7)")


def test_floor_admits_cancellation_only_near_zero():
    ref = torch.tensor([1e-6, 1.0], dtype=torch.float64)
    y = ref + torch.tensor([2e-7, 0.0], dtype=torch.float64)                       # 2e-7 off a result whose terms were ~1
    kr.assert_bf16_close(y, ref, scale=torch.tensor([1.0, 1.0]), max_mismatch=1.0, what="near zero")
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(y, ref, what="no scale")


def test_f32_bound_fails_beyond_its_ulps():
    ref = _ref()
    kr.assert_f32_close(ref.float(), ref, ref.abs(), 1, what="fp32 rounding")
    with pytest.raises(AssertionError):
        kr.assert_f32_close((ref * (1 + 8 * kr.F32_EPS)).float(), ref, ref.abs(), 4, what="8 ulps")


def _one_pass_groupnorm_f32(x, w, b, groups, eps):
    """GroupNorm with var = E[x^2] - mean^2, sums accumulated in fp32 in order (the flaw of the old gn_stats_kernel)."""
    N, HW, C = x.shape
    xg = x.reshape(N, HW, groups, C // groups).permute(0, 2, 1, 3).reshape(N, groups, -1)
    cnt = xg.shape[-1]
    s = torch.cumsum(xg, -1, dtype=torch.float32)[..., -1]
    q = torch.cumsum(xg * xg, -1, dtype=torch.float32)[..., -1]
    mean = s / cnt
    var = (q / cnt - mean * mean).clamp(min=0)
    t = (xg - mean[..., None]) * torch.rsqrt(var + eps)[..., None]
    t = t.reshape(N, groups, HW, C // groups).permute(0, 2, 1, 3).reshape(N, HW, C)
    return (t * w + b).to(torch.bfloat16)


def test_one_pass_groupnorm_variance_fails_at_large_offset():
    g = torch.Generator().manual_seed(3)
    N, HW, C, G = 1, 1024, 128, 32
    x = torch.randn(N, HW, C, generator=g)
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref, scale = kr.groupnorm(x, w, b, G, 1e-6, False)
    kr.assert_bf16_close(_one_pass_groupnorm_f32(x, w, b, G, 1e-6), ref, scale, what="one-pass GN, zero mean")   # harmless at 0
    x = x + 300.0                                                                                           # |mean| / std = 300
    ref, scale = kr.groupnorm(x, w, b, G, 1e-6, False)
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(_one_pass_groupnorm_f32(x, w, b, G, 1e-6), ref, scale, what="one-pass GN, |mean| / std 300")


# ---------------------------------------------------------------- stage-kernel references: one mutant per family
def _attn_f32(q, k, v, scale, mutant=None):
    """softmax(scale q k^T) v in fp32 on bf16 inputs [B, N, H, Dh]; mutants: 'drop_last' leaves out the last key, 'norm64' divides by
    the sum over the first 64 keys only (a lane-strided reduction that forgets its second round)"""
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if mutant == "drop_last":
        e[..., -1] = 0
    den = e[..., :64].sum(-1, keepdim=True) if mutant == "norm64" else e.sum(-1, keepdim=True)
    return torch.einsum("bhqk,bkhd->bqhd", e / den, v.float()).to(torch.bfloat16)


def _attn_close(y, q, k, v, scale, what):
    ref, mag, floor = kr.attention_small(q, k, v, scale)
    kr.assert_bf16_close(y, ref, mag * floor, floor_ulps=1, what=what)


@pytest.mark.parametrize("mutant", ["drop_last", "norm64"])
def test_attention_reference_rejects_a_dropped_or_unnormalised_key(mutant):
    g = torch.Generator().manual_seed(11)
    B, H, Nq, Nk, Dh = 1, 2, 8, 65, 40
    q, k, v = (torch.randn(B, n, H, Dh, generator=g).to(torch.bfloat16) for n in (Nq, Nk, Nk))
    _attn_close(_attn_f32(q, k, v, Dh ** -0.5), q, k, v, Dh ** -0.5, "attention fp32")
    with pytest.raises(AssertionError):
        _attn_close(_attn_f32(q, k, v, Dh ** -0.5, mutant), q, k, v, Dh ** -0.5, "attention " + mutant)


def _ramp(N, h, w, C, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return (0.7 * yy - 0.3 * xx)[None, :, :, None] + 0.25 * torch.randn(N, h, w, C, generator=g)


def test_bilinear_reference_rejects_align_corners_and_swapped_axes():
    N, h, w, C, Ho, Wo = 1, 5, 9, 4, 13, 22
    x = _ramp(N, h, w, C, 5)
    nchw = x.permute(0, 3, 1, 2)
    good = torch.nn.functional.interpolate(nchw, (Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    ref, scale = kr.resize_bilinear(x, Ho, Wo)
    kr.assert_f32_close(good, ref, scale, 4, what="ATen bilinear")
    bad = torch.nn.functional.interpolate(nchw, (Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    with pytest.raises(AssertionError):
        kr.assert_f32_close(bad, ref, scale, 4, what="align_corners=True")
    # x / y swapped: the row taps taken from the column ratio and the other way round (the same thing on a square input)
    def taps(n_in, n_out, count, limit):
        i0, i1, l1, _ = kr.bilinear_taps(n_in, n_out)
        pick = torch.arange(count) % n_out
        return i0[pick].clamp(max=limit - 1), i1[pick].clamp(max=limit - 1), l1[pick].float()
    (y0, y1, ly), (x0, x1, lx) = taps(w, Wo, Ho, h), taps(h, Ho, Wo, w)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    t = lambda yi, xi: x[:, yi][:, :, xi]                                                       # noqa: E731
    swapped = (1 - ly) * ((1 - lx) * t(y0, x0) + lx * t(y0, x1)) + ly * ((1 - lx) * t(y1, x0) + lx * t(y1, x1))
    with pytest.raises(AssertionError):
        kr.assert_f32_close(swapped, ref, scale, 4, what="axes swapped")
    # non-dyadic 7 -> 29: ATen in fp32 passes, a float64 source index does not (the taps are part of the definition)
    x7 = _ramp(1, 7, 7, 4, 6) * 50
    ref7, scale7 = kr.resize_bilinear(x7, 29, 29)
    good7 = torch.nn.functional.interpolate(x7.permute(0, 3, 1, 2), (29, 29), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    kr.assert_f32_close(good7, ref7, scale7, 4, what="ATen bilinear 7 -> 29")


def test_geglu_reference_rejects_tanh_gelu():
    inner = 96
    g = torch.linspace(-12, 12, 37 * inner).reshape(37, inner)
    a = torch.randn(37, inner, generator=torch.Generator().manual_seed(2))
    x = torch.cat([a, g], 1)
    ref, scale = kr.geglu(x, inner)
    keep = g >= -1                                                       # the result itself is well conditioned there
    kr.assert_bf16_close((a * torch.nn.functional.gelu(g)).to(torch.bfloat16), ref, scale, floor_ulps=8, what="erf GELU", flips_over=keep)
    with pytest.raises(AssertionError):
        kr.assert_bf16_close((a * torch.nn.functional.gelu(g, approximate="tanh")).to(torch.bfloat16), ref, scale, floor_ulps=8,
                             what="tanh GELU", flips_over=keep)


def test_rmsnorm_heads_reference_rejects_the_stored_width():
    g = torch.Generator().manual_seed(4)
    rows, Dh, td, eps = 17, 80, 72, 1e-5
    x = torch.randn(rows, Dh, generator=g)
    x[:, td:] = 0
    x = x.to(torch.bfloat16)
    w = 1 + 0.2 * torch.randn(Dh, generator=g)
    w[td:] = 0
    ref, mag = kr.rmsnorm_heads(x, w, eps, td)

    def f32(width):
        xf = x.float()
        return (xf * torch.rsqrt((xf * xf).sum(-1, keepdim=True) / width + eps) * w).to(torch.bfloat16)
    kr.assert_bf16_close(f32(td), ref, mag, floor_ulps=8, what="rmsnorm_heads / 72")
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(f32(Dh), ref, mag, floor_ulps=8, what="rmsnorm_heads / 80")


def test_mean_reference_rejects_the_other_axis_length():
    g = torch.Generator().manual_seed(9)
    H, W, C = 9, 13, 4
    x = torch.randn(1, H, W, C, generator=g) + 1000.0
    ref, scale = kr.mean_over(x, 2)                                       # row mean: over x, W terms
    seq = torch.cumsum(x, 2, dtype=torch.float32)[:, :, -1]
    kr.assert_f32_close(seq / W, ref, scale, kr.mean_ulps(W), what="row mean / W")
    with pytest.raises(AssertionError):
        kr.assert_f32_close(seq / H, ref, scale, kr.mean_ulps(W), what="row mean / H")


def test_mix_prediction_and_posterior_references_accept_fp32_torch():
    """the two references with the longest error propagation, against a plain fp32 torch evaluation of the same formulas"""
    g = torch.Generator().manual_seed(12)
    logit = torch.tensor([-100.0, -30.0, -2.0, 0.0, 2.0, 30.0, 100.0])
    x, eps = torch.randn(2, 7, 35, generator=g), torch.randn(2, 7, 35, generator=g)
    s = torch.sigmoid(logit)[None, :, None]
    c = kr._f32(0.8)
    ref, scale = kr.mix_prediction(eps, x, logit, 0.8)
    kr.assert_f32_close((1 - s) * (c * x) + s * eps, ref, scale, 8, what="mix_prediction fp32")
    with pytest.raises(AssertionError):
        kr.assert_f32_close(s * (c * x) + (1 - s) * eps, ref, scale, 8, what="mix_prediction, s and 1 - s swapped")
    B, F_, E, HW = 2, 6, 4, 16
    h = torch.randn(B * F_, 6 * E, HW, generator=g)
    qw, qb = torch.randn(6 * E, 2 * E, generator=g), torch.randn(6 * E, generator=g)
    qw[3 * E:] *= 30
    e = torch.randn(B, E, 3, HW, generator=g)
    r = kr.mv_posterior(h, qw, qb, e, B, F_)
    avg = h.reshape(B, F_, 6 * E, HW).sum(1) / F_
    mom = (torch.einsum("goj,bgjp->bgop", qw.reshape(3, 8, 8), avg.reshape(B, 3, 8, HW)).reshape(B, 24, HW) + qb[None, :, None]).reshape(B, 8, 3, HW)
    mean, lv = mom[:, :E], 20 * torch.tanh(mom[:, E:] / 20)
    z = mean + torch.exp(0.5 * lv) * e
    ns = (z - mean) / torch.exp(lv)
    lq = -0.5 * ns * ns - 0.9189385332046727 - lv
    for name, y in (("mean", mean), ("logvar", lv), ("z", z), ("log_q", lq)):
        kr.assert_f32_close(y, *r[name], r["ulps"], what="mv_posterior fp32 " + name)
    with pytest.raises(AssertionError):
        kr.assert_f32_close(-0.5 * ((z - mean) / torch.exp(0.5 * lv)) ** 2 - 0.9189385332046727 - lv, *r["log_q"], r["ulps"], what="log_q / std")
