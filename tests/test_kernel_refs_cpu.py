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
