"""The float64 references and bounds of the bf16 GEMM and the fused attention (tests/kernel_refs.py, last section) hold for plain fp32
restatements of the same arithmetic at every shape tests/test_gemm_attn_elements_gpu.py uses, and fail for each seeded fault a
hand-scheduled kernel could have.  No GPU needed."""
import math

import pytest
import torch

import kernel_refs as kr

C = kr.GEMM_F32_ULPS
GEMM_KS = (64, 320, 1024)


def _all_gemm_shapes():
    shapes = {(M, N, K) for F, T in set(kr.TILE_SHAPE.values()) for M, N in kr.gemm_shapes(F, T) for K in GEMM_KS}
    shapes.add((512, 512, 512))
    return sorted(shapes)


def test_constant_is_four_times_the_measured_worst_and_below_every_k():
    assert C == pytest.approx(4 * max(kr.GEMM_F32_WORST_SEQ, kr.GEMM_F32_WORST_G16), rel=2e-3) and C >= 4 * kr.GEMM_F32_WORST_SEQ
    assert all(kr.gemm_ulps(K) == C for K in GEMM_KS) and kr.gemm_ulps(4) == 4.0       # the a-priori cap K binds only below K = 6


def test_fp32_restatements_pass_the_bound_at_every_gpu_shape():
    """Sequential and 16-grouped fp32 sums of the exact products: within c / 4 (the measured worst, recorded in kernel_refs.py) of the
    float64 sum at every shape, so within the bound with the factor 4 to spare; their bf16 roundings pass assert_bf16_close."""
    worst = {"sequential": 0.0, "grouped16": 0.0}
    for M, N, K in _all_gemm_shapes():
        x, w, b = kr.gemm_inputs(M, N, K)
        ref, scale = kr.gemm_lin(x, w, b)
        for name, fn in (("sequential", kr.gemm_f32_sequential), ("grouped16", kr.gemm_f32_grouped16)):
            y = fn(x, w, b)
            r = kr.assert_f32_close(y, ref, scale, kr.gemm_ulps(K), what=f"{name} {M}x{N}x{K}") / kr.F32_EPS
            worst[name] = max(worst[name], r)
            if K == 320:
                kr.assert_bf16_close(y.to(torch.bfloat16), ref, scale, floor_ulps=C, what=f"{name} bf16 {M}x{N}x{K}")
    print(f"[kref] fp32 restatements: worst sequential {worst['sequential']:.4g}, grouped16 {worst['grouped16']:.4g} ulps of the terms; c = {C}")
    assert worst["sequential"] <= kr.GEMM_F32_WORST_SEQ * 1.001 and worst["grouped16"] <= kr.GEMM_F32_WORST_G16 * 1.001
    assert 4 * max(worst.values()) <= C


def _expf(t):
    """__expf as the device computes it: exp2 of the fp32 product with log2(e)"""
    return torch.exp2(t * torch.tensor(1.4426950408889634, dtype=torch.float32))


@pytest.mark.parametrize("epilogue", [kr.EPI_SILU, kr.EPI_QUICK_GELU, kr.EPI_GELU_TANH])
def test_expf_and_tanhf_epilogues_need_no_extra_term(epilogue):
    """The fp32 formulas of csrc/common.h (x / (1 + __expf(-x)), x / (1 + __expf(-1.702 x)), 0.5 x (1 + tanhf(..))) against float64 on
    [-40, 40]: within a quarter of the SMALLEST bound an output can have (scale = |x|: 1 bf16 ulp of the value or c fp32 ulps of |x| f').
    tanh-GELU cancels 1 + tanh for x << 0, an absolute 2^-24 |x| / 2, which the fp32 term of the bound covers; nothing is added."""
    x = torch.linspace(-40, 40, 400001, dtype=torch.float32)
    if epilogue == kr.EPI_SILU:
        y = x / (1.0 + _expf(-x))
    elif epilogue == kr.EPI_QUICK_GELU:
        y = x / (1.0 + _expf(torch.tensor(-1.702, dtype=torch.float32) * x))
    else:
        y = 0.5 * x * (1.0 + torch.tanh(torch.tensor(0.7978845608028654, dtype=torch.float32) * (x + 0.044715 * x * x * x)))
    ref, slope = kr.act64(x.double(), epilogue)
    tol = torch.maximum(kr.bf16_ulp(ref), C * kr.F32_EPS * x.double().abs() * slope)
    ratio = float(((y.double() - ref).abs() / tol).max())
    print(f"[kref] epilogue {epilogue} fp32 formula: worst {ratio:.3g} of the smallest bound")
    assert ratio <= 0.25


def test_fp32_tanh_gelu_flips_only_where_the_fp32_term_is_the_bound():
    """The fp32 tanh-GELU formula applied to the float64 sum (rounded once to fp32) on the GPU file's inputs: 1 + tanh cancels for
    x << 0, so over ALL elements more than 1 % differ from the correctly rounded value, while over the elements whose bound is the bf16
    ulp (kernel_refs.ulp_dominated) next to none do - which is the population the GPU test takes that epilogue's mismatch fraction over.
    The per-element bound holds everywhere."""
    M, N, K = 255, 252, 320
    x, w, b = kr.gemm_inputs(M, N, K)
    lin = kr.gemm_lin(x, w, b)
    ref, scale = kr.gemm_ref(x, w, b, kr.EPI_GELU_TANH, lin=lin)
    t = lin[0].float()
    y = (0.5 * t * (1.0 + torch.tanh(torch.tensor(0.7978845608028654, dtype=torch.float32) * (t + 0.044715 * t * t * t)))).to(torch.bfloat16)
    over = kr.ulp_dominated(ref, scale, C)
    flips = y.double() != kr.bf16_rne(ref)
    print(f"[kref] fp32 tanh-GELU: mismatch {float(flips.double().mean()):.3g} over all, {float(flips[over].double().mean()):.3g} where the ulp is the bound")
    assert float(flips.double().mean()) > 0.01
    kr.assert_bf16_close(y, ref, scale, floor_ulps=C, max_mismatch=0.01, what="fp32 tanh-GELU", flips_over=over)
    for epi in (kr.EPI_SILU, kr.EPI_QUICK_GELU):                       # the __expf epilogues need no such care
        r2, s2 = kr.gemm_ref(x, w, b, epi, lin=lin)
        a = 1.0 if epi == kr.EPI_SILU else 1.702
        y2 = (t / (1.0 + _expf(-torch.tensor(a, dtype=torch.float32) * t))).to(torch.bfloat16)
        kr.assert_bf16_close(y2, r2, s2, floor_ulps=C, max_mismatch=0.01, what=f"fp32 epilogue {epi}")


def test_tanh_gelu_mismatch_population_is_most_of_every_gpu_shape():
    """The elements the GPU file takes the tanh-GELU mismatch fraction over (bf16 ulp >= the fp32 term) are at least two thirds of
    the output at every shape it runs, so that fraction is never taken over a handful."""
    for M, N, K in _all_gemm_shapes():
        x, w, b = kr.gemm_inputs(M, N, K)
        ref, scale = kr.gemm_ref(x, w, b, kr.EPI_GELU_TANH)
        share = float(kr.ulp_dominated(ref, scale, kr.gemm_ulps(K)).double().mean())
        assert share >= 2.0 / 3.0, (M, N, K, share)


def test_gelu_erf_polynomial_is_within_its_documented_error():
    x = torch.linspace(-10, 10, 200001, dtype=torch.float32)
    u = x.clamp(-3.9985, 3.9985)
    t = u * u
    p = torch.full_like(x, -2.556055811e-09)
    for c in (2.088922457e-07, -7.419432677e-06, 1.523832179e-04, -2.042111475e-03, 1.916284487e-02, -1.321282834e-01, 7.976111174e-01):
        p = p * t + c
    y = 0.5 * x + 0.5 * x * (u * p)
    ref, _ = kr.act64(x.double(), kr.EPI_GELU_ERF)
    assert float((y.double() - ref).abs().max()) <= kr.GELU_ERF_ABS


# ---------------------------------------------------------------- seeded GEMM faults
M0, N0, K0 = 257, 260, 320


@pytest.fixture(scope="module")
def gemm_case():
    x, w, b = kr.gemm_inputs(M0, N0, K0)
    ref, scale = kr.gemm_lin(x, w, b)
    return x, w, b, ref, scale


def _both_bounds_fail(y64, ref, scale, what):
    kr.assert_f32_close(ref.float(), ref, scale, C, what="fp32 rounding of the reference")
    with pytest.raises(AssertionError):
        kr.assert_f32_close(y64.float(), ref, scale, C, what=what)
    with pytest.raises(AssertionError):
        kr.assert_bf16_close(kr.bf16_rne(y64), ref, scale, floor_ulps=C, what=what)


def test_fault_one_k_term_dropped_from_one_element(gemm_case):
    x, w, b, ref, scale = gemm_case
    m, n = 200, 131
    prod = x[m].double() * w[n].double()
    k = int(prod.abs().argmax())
    y = ref.clone()
    y[m, n] -= prod[k]
    _both_bounds_fail(y, ref, scale, "one k term dropped")
    # the smallest non-zero term of that element is still caught by the fp32 bound
    k = int(torch.where(prod != 0, prod.abs(), torch.full_like(prod, math.inf)).argmin())
    y = ref.clone()
    y[m, n] -= prod[k]
    if abs(float(prod[k])) > C * kr.F32_EPS * float(scale[m, n]):
        with pytest.raises(AssertionError):
            kr.assert_f32_close(y.float(), ref, scale, C, what="smallest k term dropped")


def test_fault_one_k_block_dropped_from_one_tile_row(gemm_case):
    x, w, b, ref, scale = gemm_case
    y = ref.clone()
    y[129, 128:256] -= x[129, 256:320].double() @ w[128:256, 256:320].double().t()      # the last (ragged-edge) K stage of one tile row
    _both_bounds_fail(y, ref, scale, "one 64-wide K block dropped")


def test_fault_two_adjacent_columns_swapped(gemm_case):
    x, w, b, ref, scale = gemm_case
    y = ref.clone()
    y[:, [130, 131]] = ref[:, [131, 130]]
    _both_bounds_fail(y, ref, scale, "columns swapped")


def test_fault_bias_of_the_next_column(gemm_case):
    x, w, b, ref, scale = gemm_case
    y = ref - b.double() + torch.roll(b.double(), -1)
    _both_bounds_fail(y, ref, scale, "bias of column n + 1")


def test_fault_gate_row_per_token_instead_of_per_sample(gemm_case):
    x, w, b, ref, scale = gemm_case
    g = torch.Generator().manual_seed(1)
    rows = 96
    gate = torch.randn(M0, N0, generator=g)                    # a table tall enough to be indexed by token
    res = torch.randn(M0, N0, generator=g)
    ns = (M0 + rows - 1) // rows
    good, gscale = kr.gemm_ref(x, w, b, kr.EPI_GATE_RES, gate=gate[:ns], gate_rows=rows, res=res, lin=(ref, scale))
    bad, _ = kr.gemm_ref(x, w, b, kr.EPI_GATE_RES, gate=gate, gate_rows=1, res=res, lin=(ref, scale))
    _both_bounds_fail(bad, good, gscale, "gate row per token")


def test_heads_split_ref_is_the_documented_layout():
    """Against the permute / reshape statement of tests/test_kernels_gpu.py, with every destination position hit at most once."""
    B, T, tp, H, Dh, Dp = 2, 77, 128, 2, 72, 128
    M, N = B * T, 3 * H * Dh
    shapes, which, index, untouched = kr.heads_split_ref(M, N, T, tp, H, Dh, Dp, 0b100)
    val = torch.arange(M * N, dtype=torch.float64).reshape(M, N) + 1
    outs = []
    for wi in range(3):
        cols = which == wi
        dst = torch.zeros(math.prod(shapes[wi]), dtype=torch.float64)
        assert index[:, cols].reshape(-1).unique().numel() == M * int(cols.sum())
        dst[index[:, cols].reshape(-1)] = val[:, cols].reshape(-1)
        assert int(untouched[wi].sum()) == dst.numel() - M * int(cols.sum()) and float(dst[untouched[wi]].abs().max()) == 0
        outs.append(dst.reshape(shapes[wi]))
    v5 = val.reshape(B, T, 3, H, Dh)
    assert torch.equal(outs[0][:, :, :T, :Dh], v5[:, :, 0].permute(0, 2, 1, 3))
    assert torch.equal(outs[1][:, :, :T, :Dh], v5[:, :, 1].permute(0, 2, 1, 3))
    nat = torch.zeros_like(outs[2])
    nat[..., kr.vt_key_order(tp)] = outs[2]
    assert torch.equal(nat[:, :, :Dh, :T], v5[:, :, 2].permute(0, 2, 3, 1))


# ---------------------------------------------------------------- attention: an fp32 emulation passes, seeded faults fail
def _attention_fp32(q, k, v, scale, Nk, block=64, requant_q=False):
    """The kernels' arithmetic in fp32: scores in fp32, exp2 of (s * scale * log2 e - running reference), probabilities rounded to
    bf16 for the P V product, the row sum kept in fp32, one rounding of the output."""
    qf, kf, vf = q.float(), k.float()[:, :, :Nk], v.float()[:, :, :Nk]
    sl2 = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    if requant_q:                     # attn_stream / attn_kres: the scale folded into the query, rounded to bf16 once more
        qf, sl2 = (qf * sl2).to(torch.bfloat16).float(), torch.tensor(1.0)
    s = torch.einsum("bhqd,bhkd->bhqk", qf, kf)
    m = torch.full(s.shape[:-1], -3.0e38)
    l = torch.zeros_like(m)
    o = torch.zeros(*m.shape, v.shape[-1])
    for k0 in range(0, Nk, block):
        sb = s[..., k0:k0 + block]
        m_new = torch.maximum(m, sb.amax(-1) * sl2)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(sb * sl2 - m_new[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p.to(torch.bfloat16).float() @ vf[:, :, k0:k0 + block]
        m = m_new
    return (o / l[..., None]).to(torch.bfloat16)


@pytest.mark.parametrize("Nq,Nk,Dh", [(64, 65, 64), (130, 257, 64), (65, 129, 80), (33, 77, 128)])
def test_attention_fp32_emulation_passes_the_derived_bound(Nq, Nk, Dh):
    q, k, v = kr.attention_inputs(2, 3, Nq, Nk, Dh, pad_value=1e4)
    ref, S = kr.attention_ref(q[:, :, :Nq], k, v, Dh ** -0.5, Nk)
    worst = kr.assert_attention_close(_attention_fp32(q[:, :, :Nq], k, v, Dh ** -0.5, Nk), ref, S, what=f"fp32 emulation {Nq}x{Nk}x{Dh}")
    assert worst < 0.75
    kr.assert_attention_close(kr.bf16_rne(ref), ref, S, what="rounded reference")


@pytest.mark.parametrize("Nq,Nk", [(65, 256), (200, 512)])
def test_attention_with_requantised_query_needs_and_passes_its_term(Nq, Nk):
    """The streaming kernels' second rounding of the scaled query, emulated in fp32: beyond the plain bound, inside it once
    attention_q_rounding_term (derived from that rounding, not from any output) is added."""
    q, k, v = kr.attention_inputs(2, 3, Nq, Nk, 64, pad_value=1e4)
    ref, S = kr.attention_ref(q[:, :, :Nq], k, v, 0.125, Nk)
    o = _attention_fp32(q[:, :, :Nq], k, v, 0.125, Nk, requant_q=True)
    with pytest.raises(AssertionError):
        kr.assert_attention_close(o, ref, S, what="re-rounded query, plain bound")
    worst = kr.assert_attention_close(o, ref, S, what="re-rounded query", extra=kr.attention_q_rounding_term(q[:, :, :Nq], k, v, 0.125, ref, Nk))
    assert worst < 0.75
    # with the documented rounding in the reference's query, the plain bound holds again
    ref2, S2 = kr.attention_ref(kr.requantised_query(q[:, :, :Nq], 0.125), k, v, None, Nk, base2=True)
    assert kr.assert_attention_close(o, ref2, S2, what="re-rounded query in the reference, plain bound") < 0.75


@pytest.fixture(scope="module")
def attn_case():
    Nq, Nk, Dh = 65, 77, 64
    q, k, v = kr.attention_inputs(2, 3, Nq, Nk, Dh, pad_value=1e4)
    ref, S = kr.attention_ref(q[:, :, :Nq], k, v, 0.125, Nk)
    return q[:, :, :Nq], k, v, Nk, ref, S


def _attention_fails(o64, ref, S, what):
    with pytest.raises(AssertionError):
        kr.assert_attention_close(kr.bf16_rne(o64), ref, S, what=what)


def test_fault_vt_read_without_the_key_permutation(attn_case):
    q, k, v, Nk, ref, S = attn_case
    v_seen = kr.to_vt(v).transpose(-1, -2)                         # what a kernel reading the permuted V^T in natural order sees
    bad, _ = kr.attention_ref(q, k[:, :, :Nk], v_seen[:, :, :Nk], 0.125)
    _attention_fails(bad, ref, S, "V^T without the key permutation")


def test_fault_one_padding_key_included(attn_case):
    q, k, v, Nk, ref, S = attn_case
    kz = k.clone()
    kz[:, :, Nk:] = 0                                              # even with a zero key row (score 0) the sentinel value shows
    bad, _ = kr.attention_ref(q, kz, v, 0.125, Nk + 1)
    _attention_fails(bad, ref, S, "key Nk included")


def test_fault_causal_mask_off_by_one():
    N = 33
    q, k, v = kr.attention_inputs(1, 2, N, N, 64, pad_value=1e4)
    ref, S = kr.attention_ref(q[:, :, :N], k, v, 0.125, N, causal=True)
    s = torch.einsum("bhqd,bhkd->bhqk", q[:, :, :N].double(), k[:, :, :N].double()) * 0.125
    keep = torch.arange(N)[None, :] <= torch.arange(N)[:, None] + 1
    bad = torch.softmax(s.masked_fill(~keep, -math.inf), -1) @ v[:, :, :N].double()
    _attention_fails(bad, ref, S, "key <= i + 1")
    kr.assert_attention_close(kr.bf16_rne(ref), ref, S, what="causal reference")


def test_fault_probabilities_normalised_over_the_padded_keys(attn_case):
    q, k, v, Nk, ref, S = attn_case
    kz = k.clone()
    kz[:, :, Nk:] = 0
    s = torch.einsum("bhqd,bhkd->bhqk", q.double(), kz.double()) * 0.125
    e = torch.exp(s - s[..., :Nk].amax(-1, keepdim=True))
    bad = (e[..., :Nk] / e.sum(-1, keepdim=True)) @ v[:, :, :Nk].double()
    _attention_fails(bad, ref, S, "normalised by the sum over Nk_pad")


def test_selector_scores_are_one_hot_in_fp32():
    """The selector inputs of the GPU file: the selected key's score beats every other by more than 150 in the exp2 domain, so the fp32
    softmax is exactly one-hot, for every head size and for the causal map."""
    for Dh, Nk, causal in ((64, 1280, False), (72, 129, False), (80, 129, False), (128, 129, False), (64, 128, True)):
        Nq = Nk if causal else 65
        pi = kr.selector_perm(Nq, Nk, causal)
        qc, kc = kr.selector_code(pi, Dh), kr.selector_code(torch.arange(Nk), Dh)
        s = (qc @ kc.t()) * (Dh ** -0.5 * 1.4426950408889634)
        if causal:
            s = s.masked_fill(torch.arange(Nk)[None, :] > torch.arange(Nq)[:, None], -math.inf)
        top = s.gather(1, pi[:, None])
        rest = s.scatter(1, pi[:, None], -math.inf).amax(-1, keepdim=True)
        assert float((top - rest).min()) > 150, (Dh, Nk, causal)
        assert torch.equal(torch.softmax(s.float() * math.log(2.0), -1).argmax(-1), pi)


def test_selector_v_rows_are_pairwise_distinct_at_every_gpu_shape():
    """No two (b, h, key) rows of the selector's V coincide, at any attention shape of the GPU file (attn_kres at the MI355X's 256
    heads), and no head or batch repeats another: a kernel reading the wrong batch, head, key block or ring lap returns a wrong row."""
    shapes = {(B, H, c[4], c[2] or c[1]) for c in kr.attention_cases() for B, H in kr.ATTENTION_BH}
    shapes |= {(32, 8, Nk, 64) for _, Nk in kr.KRES_SHAPES}
    for B, H, Nk, Dh in sorted(shapes):
        v = kr.selector_values(B, H, Nk, Dh)
        rows = v.view(torch.int16).reshape(B * H * Nk, Dh)
        assert torch.unique(rows, dim=0).shape[0] == B * H * Nk, (B, H, Nk, Dh)
        assert bool(torch.isfinite(v.float()).all())
    q, k, v, pi = kr.selector_inputs(2, 3, 65, 256, 64, 64, 320)
    assert torch.equal(v[:, :, :256], kr.selector_values(2, 3, 256, 64)) and bool((v[:, :, 256:] == 1e4).all()) and bool((k[:, :, 256:] == 1e4).all())
