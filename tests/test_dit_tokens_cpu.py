"""The per-token criterion of tests/dit_token_refs.py checked without a GPU: the float64 oracle it stands on, the token grouping, the
health of its yardstick for every case test_dit_tokens_gpu.py runs, and - the point of it - that it REJECTS the mistakes a denoiser
forward() can make and the whole-tensor rel-L2 gates (2e-2 against fp32, 1e-3 between two dispatch forms) let through."""
import pytest
import torch
import torch.nn.functional as F

import dit_token_refs as R
from conftest import rel_l2
from oracle import dit as odit

CAP = 1.0              # the GPU tests' cap is at or below this; a defect rejected at 1.0 is rejected at any tighter cap

OKEYS = {}
for _i in R.CASE_IDS:
    OKEYS.setdefault(R.case(_i)['okey'], _i)           # one representative case per set of oracle inputs


@pytest.mark.parametrize("cid", list(OKEYS.values()), ids=list(OKEYS))
def test_yardstick_is_healthy_and_float64_oracle_agrees_with_fp32(cid):
    """For every set of oracle inputs the GPU tests use: the oracle on a float64 state dict RUNS in float64 (both modes) and equals the
    fp32 oracle to fp32 accuracy (measured: 2.4e-7 .. 3.9e-7 whole-tensor); the allowance d_t = ||y16 - y64||_t, relative to the
    token, has its median in [1e-4, 2e-2] and no token above 5e-2 (measured: medians 1.6e-4 .. 3.9e-3, worst token 9.1e-3) - synthetic
    weights that blew the operand rounding up would inflate what the criterion allows."""
    c = R.case(cid)
    y64, y16 = R.oracle_pair(cid)
    assert y64.dtype == torch.float64 and y16.dtype == torch.float64
    y32 = R.oracle_forward(c, R.synth_sd(c['kind'], c['net']), c['x_or'], c['t'], c['ctx'])
    assert y32.dtype == torch.float32 and y32.shape == y64.shape
    e = rel_l2(y32, y64)
    med, mx = R.yardstick(y16, y64, c['patch'])
    print(f"{c['okey']}: fp32 vs float64 oracle {e:.2e}; d_t / |y64|_t median {med:.2e} max {mx:.2e}")
    assert e < 2e-6, e                                  # depth-2 fp32 forward: a few fp32 ulps per element
    assert R.YARD_MEDIAN[0] <= med <= R.YARD_MEDIAN[1] and mx <= R.YARD_MAX, (med, mx)


def test_operand_rounding_mode_is_dtype_clean():
    """operand_rounding() on float64 inputs rounds THROUGH bf16 and comes back float64; on fp32 inputs it is what it always was."""
    x64 = torch.linspace(-3, 3, 1001, dtype=torch.float64)
    with odit.operand_rounding(torch.bfloat16):
        r64, r32 = odit._r(x64), odit._r(x64.float())
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32
    assert torch.equal(r64, x64.to(torch.bfloat16).double()) and torch.equal(r32.double(), r64)
    assert odit._r(x64) is x64                                                        # off: untouched
    assert odit.rms_norm(x64[None], None).dtype == torch.float64 and odit.rms_norm(x64[None].float(), None).dtype == torch.float32
    assert odit.timestep_embedding(torch.tensor([3.0], dtype=torch.float64)).dtype == torch.float64
    assert odit.timestep_embedding(torch.tensor([3])).dtype == torch.float32         # integer timesteps: fp32 as before


# ------------------------------------------------------------------------------------------------ grouping
@pytest.mark.parametrize("size", ['small', 'fused'])
def test_token_grouping_round_trips(size):
    """Perturbing ONE token of the token tensor in front of the final layer changes exactly one group of the output, the one
    token_groups() files under (sample, token // L, token % L); all others are bit-identical."""
    c = R.case(f't23d-{size}-plain')
    sd = R.to64(R.synth_sd('t23d', size))
    x, t, ctx = R.to64(c['x']), R.to64(c['t']), R.to64(c['ctx'])
    with torch.no_grad():
        h = odit.t23d_forward(sd, x, t, ctx, c['heads'], return_tokens=True)
        t_emb = odit.t_embedder(sd, t)
        y0 = odit.t23d_final(sd, h, t_emb)
        assert torch.equal(y0, odit.t23d_forward(sd, x, t, ctx, c['heads']))
        Bn, N, _ = h.shape
        L = N // 3
        g0 = R.token_groups(y0, 2)
        assert g0.shape == (Bn, 3, L, 2 * 2 * 4)
        for b, tok in ((0, 0), (1, L - 1), (1, L), (Bn - 1, N - 1), (2, L + 7)):
            h2 = h.clone()
            h2[b, tok] += 0.5
            changed = (R.token_groups(odit.t23d_final(sd, h2, t_emb), 2) != g0).any(-1)
            assert changed.sum() == 1 and bool(changed[b, tok // L, tok % L]), (b, tok, changed.nonzero())
    # the layout itself: out[b, c*3 + plane, ph*p + i, pw*p + j] is number (i*p + j)*C + c of group [b, plane, ph*g + pw]
    S = 6
    y = torch.arange(2 * 12 * S * S, dtype=torch.float64).reshape(2, 12, S, S)
    g = R.token_groups(y, 2)
    for b, cch, plane, ph, pw, i, j in ((0, 0, 0, 0, 0, 0, 0), (1, 3, 2, 2, 1, 1, 0), (0, 2, 1, 1, 2, 0, 1)):
        assert g[b, plane, ph * 3 + pw, (i * 2 + j) * 4 + cch] == y[b, cch * 3 + plane, ph * 2 + i, pw * 2 + j]
    pts = torch.randn(2, 5, 19)
    assert torch.equal(R.token_groups(pts, 1)[:, 0], pts)


# ------------------------------------------------------------------------------------------------ seeded defects
def _defective(cid, monkeypatch, patches):
    """the bf16-operand float64 oracle of the case with oracle functions replaced: what a wrong forward() would have produced"""
    for name, fn in patches.items():
        monkeypatch.setattr(odit, name, fn)
    y = R.rounded_oracle(cid)
    monkeypatch.undo()
    return y


def _judge(cid, y_bad, what):
    c = R.case(cid)
    y64, y16 = R.oracle_pair(cid)
    rho, _ = R.token_rho(y_bad, y16, y64, c['patch'])
    where, worst = R.worst_token(rho)
    whole = rel_l2(y_bad, y16)
    print(f'{what} [{cid}]: worst token {where} rho = {worst:.2f}, tokens over the cap {int((rho > CAP).sum())} of {rho.numel()}; '
          f'whole-tensor rel-L2 {whole:.2e} (passes the 2e-2 gate: {whole < 2e-2}, the 1e-3 gate: {whole < 1e-3})')
    return where, worst, whole, rho


def _sane(cid):
    """without a defect the same computation gives rho = 0 everywhere"""
    c = R.case(cid)
    y64, y16 = R.oracle_pair(cid)
    assert float(R.token_rho(y16, y16, y64, c['patch'])[0].max()) == 0.0


_block, _cross, _mlp, _ln = odit.t23d_block, odit.cross_attention, odit.fused_mlp, odit.layer_norm


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_layer_reads_its_neighbours_adaln_slice(monkeypatch, size):
    """mod[:, o6 + k*D:] with the wrong o6: layer 1 modulated by layer 0's adaLN rows.  Rejected (measured, small / fused: rho 72 /
    107 at the worst token, every token over the cap); whole-tensor rel-L2 1.97e-2 / 2.06e-2 - at the edge of the 2e-2 gate."""
    cid = f't23d-{size}-plain'

    def block(sd, p, x, t_emb, ctx, H):
        if p == 'blocks.1.':
            sd = dict(sd)
            for k in ('weight', 'bias'):
                sd[p + 'adaLN_modulation.1.' + k] = sd['blocks.0.adaLN_modulation.1.' + k]
        return _block(sd, p, x, t_emb, ctx, H)
    _sane(cid)
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'t23d_block': block}), 'layer 1 reads layer 0 adaLN')
    assert worst > CAP


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_one_sample_attends_to_anothers_context(monkeypatch, size):
    """cc['k'][i][fold:] off by one sample, in one layer: sample 0's cross-attention of layer 1 over sample 1's prompt.  Rejected
    (measured: rho 77 / 76, all tokens of sample 0 and none of the others); whole-tensor rel-L2 1.4e-2 / 1.1e-2 passes the 2e-2 gate."""
    cid = f't23d-{size}-plain'

    def cross(sd, p, x, ctx, H, dim_head=64, **kw):
        if p == 'blocks.1.cross_attn.':
            ctx = torch.cat([ctx[1:2], ctx[1:]])
        return _cross(sd, p, x, ctx, H, dim_head, **kw)
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'cross_attention': cross}), "sample 0 uses sample 1's context in layer 1")
    assert worst > CAP and where[0] == 0
    assert bool((rho[0] > CAP).all()) and float(rho[1:].max()) == 0.0


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_ragged_batch_reads_anothers_modulation_row(monkeypatch, size):
    """mod_ld = 0 where it should be nmod: sample 0 of a ragged-timestep batch modulated (blocks; the final layer keeps its own row) by
    sample 1's row.  Rejected (measured: rho 84 / 97, only tokens of sample 0); whole-tensor rel-L2 1.1e-2 / 1.2e-2 passes 2e-2."""
    cid = f't23d-{size}-modcache_ragged'

    def block(sd, p, x, t_emb, ctx, H):
        return _block(sd, p, x, torch.cat([t_emb[1:2], t_emb[1:]]), ctx, H)
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'t23d_block': block}), "sample 0 uses sample 1's modulation")
    assert worst > CAP and where[0] == 0 and float(rho[1:].max()) == 0.0


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_last_token_skips_the_mlp_gate(monkeypatch, size):
    """The last row of the last tile: the last token of the last sample adds fc2's output of layer 1 without its gate.  Rejected
    (measured: rho 770 / 871 at exactly that token, all others 0); one token of 144 / 576: whole-tensor rel-L2 3.5e-2 / 9.3e-3 - at
    the fused size the 2e-2 gate passes it, and neither says which token."""
    cid = f't23d-{size}-plain'
    gate = {}

    def block(sd, p, x, t_emb, ctx, H):
        mod = odit.linear(F.silu(t_emb), sd[p + 'adaLN_modulation.1.weight'], sd[p + 'adaLN_modulation.1.bias'])
        gate['g'] = mod.chunk(6, dim=1)[5] if p == 'blocks.1.' else None
        return _block(sd, p, x, t_emb, ctx, H)

    def mlp(sd, p, x):
        o = _mlp(sd, p, x)
        if gate['g'] is not None:
            o = o.clone()
            o[-1, -1] = o[-1, -1] / gate['g'][-1]          # the block multiplies the gate back in: this token is left ungated
        return o
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'t23d_block': block, 'fused_mlp': mlp}), 'last token skips the MLP gate')
    Bn, P, L = rho.shape
    assert worst > CAP and where == (Bn - 1, P - 1, L - 1)
    assert int((rho > 0).sum()) == 1


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_first_row_after_the_fold_gets_the_folded_constant(monkeypatch, size):
    """r0 = fold * N off by one row: the first token of the first conditional sample (sample 2 of [uc, uc, c, c]) receives, in layer
    0, the folded samples' constant cross-attention output instead of its own.  One token of 192 / 768.  Rejected (measured: rho 154 / 151 at that token, nothing outside sample 2);
    whole-tensor rel-L2 3.8e-3 / 2.1e-3 passes the 2e-2 gate."""
    cid = f't23d-{size}-cfg_fold'
    fold = R.case(cid)['fold']

    def cross(sd, p, x, ctx, H, dim_head=64, **kw):
        o = _cross(sd, p, x, ctx, H, dim_head, **kw)
        if p == 'blocks.0.cross_attn.':
            o = o.clone()
            o[fold, 0] = o[fold - 1, 0]                    # uniform keys: every query of sample fold - 1 gets this same row
        return o
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'cross_attention': cross}), 'first row after the fold gets the constant')
    assert worst > CAP and where[0] == fold
    assert float(rho[:fold].max()) == 0.0 and float(rho[fold + 1:].max()) == 0.0         # self-attention spreads it inside sample 2 only


# -- candidates for the noise floor: nearly-right constants
@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_caption_gelu_erf_for_tanh(monkeypatch, size):
    """The caption embedder with the erf GELU in place of the tanh approximation (they differ by up to 5e-4 absolute, an eighth of a
    bf16 ulp at 1).  NOT detected, rho = 0.74 / 0.88 at the worst token (whole-tensor rel-L2 1.9e-4 / 1.6e-4): below the rounding
    noise - the context is rounded to bf16 right behind this GELU.  Kept as the measured noise floor of the criterion."""
    cid = f't23d-{size}-plain'

    def cap(sd, p, c):
        h = odit.linear(c, sd[p + 'y_proj.fc1.weight'], sd[p + 'y_proj.fc1.bias'])
        return odit.linear(F.gelu(h), sd[p + 'y_proj.fc2.weight'], sd[p + 'y_proj.fc2.bias'])
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'caption_embedder': cap}), 'caption embedder erf GELU')
    assert torch.isfinite(rho).all() and 0.1 < worst <= CAP, worst              # not detected - and not nothing either


@pytest.mark.parametrize("size", ['small', 'fused'])
def test_defect_prenorm_eps(monkeypatch, size):
    """Every affine-free LayerNorm with eps 1e-5 in place of 1e-6.  NOT detected, rho = 0.40 / 0.43 at the worst token (whole-tensor
    rel-L2 4.5e-5 / 5.8e-5): the token variance is ~1, so the two differ by 4.5e-6 relative - a thousandth of a bf16 ulp."""
    cid = f't23d-{size}-plain'

    def ln(x, eps=1e-6, w=None, b=None):
        return _ln(x, 1e-5 if eps == 1e-6 else eps, w, b)
    where, worst, whole, rho = _judge(cid, _defective(cid, monkeypatch, {'layer_norm': ln}), 'pre-norm eps 1e-5')
    assert torch.isfinite(rho).all() and 0.1 < worst <= CAP, worst              # not detected - and not nothing either
