"""The oracle of the two DINOv2-based VAE decoder classes (oracle/dino_decoder.py) and the per-token / per-pixel checks built on it
(tests/dino_decoder_refs.py), without a GPU:

  * the float64 oracle reproduces every stored stage of the reference goldens, the released sizes included (3 s each in float64), and
    the reference class's own vae_reparameterization (tests/golden/shapenet_reparam_b2.npz);
  * the yardstick of every rho stage of every case lies inside the window of dit_token_refs; the stages without a bf16 operand are
    exactly the stages whose oracle d is 0;
  * every case's stated launches are what csrc/kernel_plan.h and the product's dispatch code give;
  * decode() is its stages chained, bit for bit;
  * an fp32 stand-in of the product path (the oracle under rounding, in float32) passes the GPU tests' own check functions, and every
    seeded defect is caught by them at the stage, and near the token or pixel, where it sits - or is recorded as not visible."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_decoder_refs as R
import test_dino_decoder_pixels_gpu as G
from conftest import golden, rel_l2
from ln3diff_amd.synth import synth_input
from oracle import dino_decoder as odd
from oracle import dit as odit

GOLDEN_GATE = 1e-4        # the rel-L2 the encoder oracle was held to; compared in fp16 where the golden's fp16 storage (2e-4) dominates
CAP = 1.0                 # the ceiling of every cap


def _h(x):
    return x.half().double()


# ------------------------------------------------------------------------------------------------ the float64 oracle against the goldens
GOLDENS = [('shapenet', 'shapenet_dec_small', 'shapenet_latent', 11, 128, 2), ('ffhq', 'ffhq_dec_small', 'ffhq_latent', 21, 128, 2),
           ('shapenet', 'shapenet_dec_released', 'shapenet_latent_rel', 13, 768, 12), ('ffhq', 'ffhq_dec_released', 'ffhq_latent_rel', 23, 768, 12)]
# the sub-sampling of tests/golden/make_golden_{shapenet,ffhq}_decoder.py: stage -> slices of (small, released)
SLICES = {'ldm_upsample': ((slice(None), slice(None, None, 2)), (slice(None), slice(None, None, 6), slice(None, None, 2))),
          'vit': ((slice(None), slice(None, None, 2)), (slice(None), slice(None, None, 6), slice(None, None, 2))),
          'decoder_pred': ((slice(None), slice(None, None, 4), slice(None, None, 8)), (slice(None), slice(None, None, 6), slice(None, None, 16))),
          'planes': ((slice(None), slice(None), slice(None, None, 8), slice(None, None, 8)),) * 2,
          'x0': ((slice(None), slice(None), slice(None, None, 8), slice(None, None, 8)),) * 2}


@pytest.mark.parametrize("cls,tag,lname,seed,D,heads", GOLDENS, ids=[g[1] for g in GOLDENS])
def test_float64_oracle_reproduces_every_stored_stage(cls, tag, lname, seed, D, heads):
    g = golden(tag)
    rel = 'released' in tag
    sd = R.to64(R.dec_sd(cls, D, heads))
    taps = {}
    with torch.no_grad():
        tok, planes = odd.decode(sd, cls, synth_input(lname, (1, *R.LATENT[cls]), seed).double(), heads, 256, taps)
    got = {'ldm_upsample': taps['embed'][1], 'vit': tok, 'decoder_pred': taps['decoder_pred'][1], 'planes': planes, 'x0': taps['x0'][1]}
    step = 8 if cls == 'shapenet' else 4
    for j in range(6):
        got[f"stage_{'pair' if cls == 'shapenet' else 'blk'}{j}"] = taps[f'group{j}'][1][:, ::step]
    seen = 0
    for k in g.files:
        if k not in got:
            continue
        y = got[k][SLICES[k][rel]] if k in SLICES else got[k]
        ref = torch.from_numpy(g[k]).double()
        e = rel_l2(_h(y), ref) if g[k].dtype == np.float16 else rel_l2(y, ref)
        print(f'{tag} {k}: rel-L2 {e:.2e}')
        assert e < GOLDEN_GATE, (tag, k, e)
        seen += 1
    assert seen == (4 if rel else 10) + (cls == 'ffhq')


def test_float64_oracle_decodes_a_batch_object_by_object():
    g = golden('shapenet_dec_b2')
    sd = R.to64(R.dec_sd('shapenet'))
    lat = synth_input('shapenet_latent_b2', (2, 12, 32, 32), 12).double()
    with torch.no_grad():
        tok, planes = odd.decode(sd, 'shapenet', lat, 2, 256)
        tok1, planes1 = odd.decode(sd, 'shapenet', lat[1:], 2, 256)
    assert rel_l2(_h(tok[:, ::4]), torch.from_numpy(g['vit']).double()) < GOLDEN_GATE
    assert rel_l2(_h(planes[:, ::2, ::8, ::8]), torch.from_numpy(g['planes']).double()) < GOLDEN_GATE
    assert float((tok[1:] - tok1).abs().max()) < 1e-12 and float((planes[1:] - planes1).abs().max()) < 1e-12


def test_float64_oracle_reproduces_the_reference_reparameterization():
    """the fixture is the reference class's own vae_reparameterization(tokens, False) (fp32): latent and soft-clamped log-variance"""
    g = golden('shapenet_reparam_b2')
    tok, _ = R.reparam_inputs()
    assert torch.equal(tok, torch.from_numpy(g['tokens']).float())
    y64, _ = R.reparam_pair()
    assert rel_l2(y64['latent_normalized_2Ddiffusion'], torch.from_numpy(g['latent']).double()) < 1e-6
    assert rel_l2(y64['logvar'], torch.from_numpy(g['logvar']).double()) < 1e-6
    assert torch.equal(y64['z'], y64['mean']) and y64['latent_tok'].shape == (2, 3072, 4)
    # the layout helper of the GPU test: the rows ldm_downsample wrote, back from the posterior's input
    sd = R.to64(R.dec_sd('shapenet'))
    rows = F.linear(tok.double(), sd[odd.SR + 'ldm_downsample.weight'], sd[odd.SR + 'ldm_downsample.bias'])
    assert torch.equal(R.reparam_tokens(y64['h']), rows)


# ------------------------------------------------------------------------------------------------ yardsticks
@pytest.mark.parametrize("cid", list(R.TIER_A))
def test_yardstick_of_every_stage_and_the_fp32_stages_are_those_with_d_zero(cid):
    """measured: medians 1.8e-4 (ShapeNet group5) .. 2.4e-3, worst group 5.7e-3 - no case needed another seed"""
    cls = R.TIER_A[cid]['cls']
    zero = []
    for name in R.stage_names(cls):
        _, y64, y16 = R.stage_pair(cid, name)
        k = R.stage_kind(name)
        if float((R.groups(y16, k) - R.groups(y64, k)).abs().max()) == 0.0:
            zero.append(name)
            continue
        med, mx = R.group_yardstick(y16, y64, k)
        print(f'{cid} {name}: d / |y64| per group: median {med:.2e} max {mx:.2e}')
        assert R.YARD_MEDIAN[0] <= med <= R.YARD_MEDIAN[1] and mx <= R.YARD_MAX, (cid, name, med, mx)
    assert zero == R.f32_stages(cls)
    assert set(G.MEASURED) >= {f'{cid}/{n}' for n in R.stage_names(cls) if n not in zero}


@pytest.mark.parametrize("sid", [s for s in R.SINGLES if not R.SINGLES[s].get('refused')])
def test_yardstick_of_every_single_case(sid):
    cls = R.SINGLES[sid]['cls']
    ins = R.single_inputs(sid)
    for name in R.single_stages(sid):
        if name in R.f32_stages(cls):
            continue
        use = ins
        if R.SINGLES[sid]['kind'] == 'conv':
            use = _conv_stage_inputs(sid, name, ins)
        y64, y16 = R.single_pair(sid, name, use)
        med, mx = R.group_yardstick(y16, y64, R.stage_kind(name) if name != 'cross' else 'tok')
        print(f'{sid} {name}: d / |y64| per group: median {med:.2e} max {mx:.2e}')
        assert R.YARD_MEDIAN[0] <= med <= R.YARD_MEDIAN[1] and mx <= R.YARD_MAX, (sid, name, med, mx)
        assert f'{sid}/{name}' in G.MEASURED


def _conv_stage_inputs(sid, name, ins):
    """the inputs of a stage of a conv case, the earlier stages taken from the rounded float64 oracle (the CPU's stand-in for the HIP
    outputs the GPU test feeds on)"""
    c = R.SINGLES[sid]
    up, res = (t.double() for t in ins)
    sd = R.single_sd(sid)
    if c['cls'] == 'ffhq':
        return (up, res) if name == 'x0' else (R.run_stage(sd, 'ffhq', 'x0', (up, res)).float().double(),)
    if name == 'conv0':
        return (up,)
    t0 = R.run_stage(sd, 'shapenet', 'conv0', (up,))
    if name == 'x0':
        return (res, t0)
    x0 = R.run_stage(sd, 'shapenet', 'x0', (res, t0)).float().double()
    return (x0,) if name == 'conv1' else (x0, R.run_stage(sd, 'shapenet', 'conv1', (x0,)))


# ------------------------------------------------------------------------------------------------ the stated launches
def test_every_case_states_the_launch_the_product_and_the_plan_give(tmp_path):
    from ln3diff_amd.vit import vit_triplane_ffhq as ff, vit_triplane_shapenet as sn
    # the product's dispatch: which class runs which convolution route, and how it carries the residual-stream weights
    assert 'im2col3x3_rollout' in inspect.getsource(sn.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn._conv_planes)
    assert 'conv3x3_rollout' in inspect.getsource(getattr(ff, ff.CLASS_NAME)._conv_planes)
    assert 'im2col' not in inspect.getsource(getattr(ff, ff.CLASS_NAME)._conv_x0)
    for cid, c in R.TIER_A.items():
        assert c['conv'] == ('im2col+gemm' if c['cls'] == 'shapenet' else 'fused')
        assert c['rows'] == c['B'] * 768 and c['attn'] == ('stream', 64, 256, c['B'] * 3 * R.HEADS) and c['attn'][3] < R.CUS
    assert getattr(ff, ff.CLASS_NAME)._res_w is not sn._DinoTriplaneDecoderBase._res_w            # the bf16 pair
    hi, lo = ff._pair(torch.tensor([[1.0 + 2.0 ** -10]]), torch.device('cpu'))
    assert float(hi) == 1.0 and float(lo) == 2.0 ** -10
    # the plan of csrc/kernel_plan.h: the streaming kernel (64-wide heads, 256 keys), never the K-resident one; B = 1 stays inside the
    # 128x128 tile, B = 3 leaves it
    launches = R.launch_lines()
    planned = R.plan([ln for *_, ln in launches], tmp_path)
    for (who, route, ring_stated, ln), (kernel, ring) in zip(launches, planned):
        assert kernel == 'stream' and ln[3] < R.CUS, (who, kernel)
        assert route in (None, 'stream')
        assert ring == ring_stated, (who, ln, ring)
    assert {c['ring_gemm'] for c in R.TIER_A.values()} == {False, True}
    # the fused roll-out convolution refuses what it cannot run (csrc/ffhq_ops.hip: Cout % 32): the narrow pair is a refusal there
    assert [s for s, c in R.SINGLES.items() if c.get('refused')] == ['ffhq-conv-narrow']


# ------------------------------------------------------------------------------------------------ oracle self-consistency
@pytest.mark.parametrize("cid", ['shapenet-b1', 'ffhq-b3'])
def test_decode_is_the_chained_stages_bit_for_bit(cid):
    c = R.TIER_A[cid]
    cls = c['cls']
    for dt, rounded in ((torch.float32, True), (torch.float64, False), (torch.float64, True)):
        sd = {k: v.to(dt) for k, v in R.dec_sd(cls).items()}
        taps = {}
        with torch.no_grad():
            if rounded:
                with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
                    tok, planes = odd.decode(sd, cls, R.latent(cid).to(dt), R.HEADS, R.R_TIER_A, taps)
            else:
                tok, planes = odd.decode(sd, cls, R.latent(cid).to(dt), R.HEADS, R.R_TIER_A, taps)
        out = {}
        for name in R.stage_names(cls):
            ins = R.stage_inputs(cls, taps, name)
            out[name] = R.run_stage(sd, cls, name, ins, rounded=rounded)
            want = taps['x0' if name == 'x0' else name][1]
            assert out[name].dtype == dt and torch.equal(out[name], want), (cid, name, dt, rounded)
        assert torch.equal(out['norm'], tok) and torch.equal(out['planes'], planes)
        # the skips are popped last in, first out: group 3 takes group 1's output, group 5 the tokens behind pos_embed
        push = odd.push_skip if rounded else (lambda t: t)
        with odit.operand_rounding(torch.bfloat16, kernel_arith=True) if rounded else torch.no_grad():
            assert torch.equal(taps['skip3'][0][1], push(taps['group1'][1])) and torch.equal(taps['skip4'][0][1], push(taps['group0'][1]))
            assert torch.equal(taps['skip5'][0][1], push(taps['pos'][1]))


def test_operand_rounding_was_not_extended():
    """The decoders' two special cases live in oracle.dino_decoder itself (axis_attention rounds nothing, res_linear(pair=True) is the
    bf16 pair), so oracle.dit.operand_rounding keeps its arguments and every earlier caller its bits: nothing in it reads new state."""
    assert list(inspect.signature(odit.operand_rounding.__init__).parameters) == ['self', 'dtype', 'kernel_arith', 'unfused_norms']
    assert sorted(n for n, v in vars(odit).items() if isinstance(v, list)) == ['KERNEL_ARITH', 'OPERAND_ROUND', 'UNFUSED_NORMS']
    x, w = synth_input('x', (5, 64), 1).double(), synth_input('w', (7, 64), 2).double()
    with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
        a, b = odd.res_linear(x, w, None, pair=False), odit.linear(x, w)
        p = odd.res_linear(x, w, None, pair=True)
    assert torch.equal(a, b) and not torch.equal(p, a)
    assert torch.equal(odd.res_linear(x, w, None, pair=True), F.linear(x, w))          # without rounding the pair is the weight
    exact = F.linear(x.to(torch.bfloat16).double(), w)
    assert float((p - exact).abs().max()) < 2.0 ** -15 * float((x.abs() @ w.abs().t()).max())


# ------------------------------------------------------------------------------------------------ the fp32 stand-in and the seeded defects
def _standin(cls, sd, name, ins, R_=R.R_TIER_A):
    """the product path's stand-in: the oracle under rounding, in float32"""
    return R.run_stage(sd, cls, name, tuple(t.float() for t in ins), R_)


def _rho_of(key, bad, y16, y64, kind, R_=None, cap=None):
    """through the GPU tests' own check, at the stage's own cap"""
    failures = []
    worst, at = R.judge(key, bad, y16, y64, kind, G.cap(key.split(':')[0]) if cap is None else cap, failures, R_)
    rho, _ = R.group_rho(torch.as_tensor(bad).double(), y16, y64, kind)
    return rho, worst, at, failures


def test_fp32_stand_in_passes_the_gpu_checks_at_every_stage():
    """Another correct implementation of the same arithmetic has rounding-boundary flips of its own, so it is held to the ceiling of
    the caps, not to the cap the HIP stage measured.  Measured worst rho of the stand-in: single GEMMs and convolutions 5e-5 .. 2e-3,
    fusion groups ShapeNet 0.40 .. 0.80, FFHQ 0.56 .. 0.96 - the size the HIP stages show (test_dino_decoder_pixels_gpu.MEASURED)."""
    for cid in ('shapenet-b1', 'ffhq-b1'):
        cls = R.TIER_A[cid]['cls']
        for name in R.stage_names(cls):
            ins, y64, y16 = R.stage_pair(cid, name)
            y = _standin(cls, R.dec_sd(cls), name, ins)
            assert y.dtype == torch.float32
            if name in R.f32_stages(cls):                       # a correctly rounded fp32 kernel: the float64 stage, rounded once
                y = y64.float()
                R.f32_check(cls, R.dec_sd(cls), name, ins, y if name != 'norm' else y.reshape(-1, y.shape[-1]), f'{cid}/{name} stand-in')
            else:
                _, worst, _, failures = _rho_of(f'{cid}/{name}', y, y16, y64, R.stage_kind(name), cap=CAP)
                assert not failures and worst <= CAP, failures


def _cross_defect(monkeypatch, sid, patch):
    cls = R.SINGLES[sid]['cls']
    ins = R.single_inputs(sid)
    y64, y16 = R.single_pair(sid, 'cross', ins)
    patch(monkeypatch)
    bad = _standin(cls, R.single_sd(sid), 'cross', ins)
    monkeypatch.undo()
    return _rho_of(f'{sid}/cross', bad, y16, y64, 'tok')


def _axis_variant(order=(1, 2), col_along_row=False, obj0_keys=False):
    def axis_attention(q, k, v):
        p, scale = q.shape[2], q.shape[-1] ** -0.5
        if obj0_keys:
            k, v = k[:1].expand_as(k), v[:1].expand_as(v)
        col = 'bxjhd' if col_along_row else 'bjxhd'
        out = []
        for i in range(3):
            kr, vr = k[:, (i + order[0]) % 3], v[:, (i + order[0]) % 3]
            kc, vc = k[:, (i + order[1]) % 3], v[:, (i + order[1]) % 3]
            s = torch.cat([torch.einsum('byxhd,byjhd->byxhj', q[:, i], kr), torch.einsum(f'byxhd,{col}->byxhj', q[:, i], kc)], -1) * scale
            a = torch.softmax(s, -1)
            out.append(torch.einsum('byxhj,byjhd->byxhd', a[..., :p], vr) + torch.einsum(f'byxhj,{col}->byxhd', a[..., p:], vc))
        return torch.stack(out, 1)
    return axis_attention


@pytest.mark.parametrize("cls", odd.CLASSES)
def test_defect_cross_plane_keys_from_the_wrong_planes(monkeypatch, cls):
    """planes i + 2 / i + 1 instead of i + 1 / i + 2: every token is wrong"""
    rho, worst, _, failures = _cross_defect(monkeypatch, f'{cls}-cross-b1', lambda m: m.setattr(odd, 'axis_attention', _axis_variant(order=(2, 1))))
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


@pytest.mark.parametrize("cls", odd.CLASSES)
def test_defect_column_keys_taken_along_the_row(monkeypatch, cls):
    """plane i + 2 read along its row x instead of its column x: right only where nothing distinguishes them"""
    rho, worst, _, failures = _cross_defect(monkeypatch, f'{cls}-cross-b1', lambda m: m.setattr(odd, 'axis_attention', _axis_variant(col_along_row=True)))
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


@pytest.mark.parametrize("cls", odd.CLASSES)
def test_defect_object_1_reads_object_0s_keys(monkeypatch, cls):
    rho, worst, at, failures = _cross_defect(monkeypatch, f'{cls}-cross-b2', lambda m: m.setattr(odd, 'axis_attention', _axis_variant(obj0_keys=True)))
    assert failures and at[0] == 1
    assert float(rho[0].max()) <= CAP and float((rho[1] > CAP).float().mean()) > 0.9       # object 0 is right, object 1 is not


def test_defect_ls1_not_applied_to_n(monkeypatch):
    def cross_block(sd, p, x, H):
        n = odd._ln(sd, p + 'norm1.', x)
        return odd.mlp_half(sd, p, x + n + sd[p + 'ls1.gamma'] * odd.cross_attention(sd, p + 'attn.', n, H))
    rho, worst, _, failures = _cross_defect(monkeypatch, 'shapenet-cross-b1', lambda m: m.setattr(odd, 'cross_block', cross_block))
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


def test_defect_inner_norm1_skipped(monkeypatch):
    real = odd._ln

    def _ln(sd, p, x):
        return x if p.endswith('attn.norm1.') else real(sd, p, x)
    rho, worst, _, failures = _cross_defect(monkeypatch, 'shapenet-cross-b1', lambda m: m.setattr(odd, '_ln', _ln))
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


def test_defect_skips_popped_first_in_first_out():
    """The order of the skips is wiring: a stage test hands skip_step its skip.  The wiring checks see it - the chained stages (which
    pop last in, first out) no longer equal the forward, from skip3 on - and so does the per-token check of skip3's output."""
    cid, cls = 'shapenet-b1', 'shapenet'
    sd = {k: v.float() for k, v in R.dec_sd(cls).items()}
    good, fifo = {}, {}
    with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
        raw = odd.embed(sd, cls, R.latent(cid))
        odd.vit_forward(sd, cls, raw, R.HEADS, good)
        odd.vit_forward(sd, cls, raw, R.HEADS, fifo, pop=lambda s: s.pop(0))
    names = [n for n in R.stage_names(cls) if n in good]
    first = next(n for n in names if not torch.equal(good[n][1], fifo[n][1]))
    assert first == 'skip3' and torch.equal(good['group2'][1], fifo['group2'][1])
    assert torch.equal(fifo['skip5'][0][1], good['skip3'][0][1]) and not torch.equal(fifo['skip3'][0][1], good['skip3'][0][1])
    ins, y64, y16 = R.stage_pair(cid, 'skip3')
    bad = _standin(cls, R.dec_sd(cls), 'skip3', (ins[0], fifo['skip3'][0][1]))
    rho, worst, _, failures = _rho_of(f'{cid}/skip3', bad, y16, y64, 'tok')
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


@pytest.mark.parametrize("cls", odd.CLASSES)
def test_defect_skip_linear_halves_swapped(monkeypatch, cls):
    sid = f'{cls}-skip'
    ins = R.single_inputs(sid)
    y64, y16 = R.single_pair(sid, 'skip3', ins)

    def skip_step(sd, cls_, j, x, skip):
        w, b = sd[f'{odd.VD}blocks.{j}.skip_linear.weight'], sd[f'{odd.VD}blocks.{j}.skip_linear.bias']
        Dm = x.shape[-1]
        return x + odd.res_linear(x, w[:, Dm:], b, cls_ == 'ffhq') + odd.res_linear(skip, w[:, :Dm], None, cls_ == 'ffhq')
    monkeypatch.setattr(odd, 'skip_step', skip_step)
    bad = _standin(cls, R.single_sd(sid), 'skip3', ins)
    monkeypatch.undo()
    rho, worst, _, failures = _rho_of(f'{sid}/skip3', bad, y16, y64, 'tok')
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


def test_defect_transpose_in_front_of_the_first_convolution_dropped(monkeypatch):
    cid = 'shapenet-b1'
    ins, y64, y16 = R.stage_pair(cid, 'upsample')
    monkeypatch.setattr(odd, 'upsample_t', lambda lat, R_: odit._r(odd.resize(lat, R_)))
    bad = _standin('shapenet', R.dec_sd('shapenet'), 'upsample', ins)
    monkeypatch.undo()
    rho, worst, _, failures = _rho_of(f'{cid}/upsample', bad, y16, y64, 'px', R.R_TIER_A)
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


def _conv_defect(monkeypatch, sid, name, patch):
    c = R.SINGLES[sid]
    ins = _conv_stage_inputs(sid, name, R.single_inputs(sid))
    y64, y16 = R.single_pair(sid, name, ins)
    patch(monkeypatch)
    bad = _standin(c['cls'], R.single_sd(sid), name, ins, c['R'])
    monkeypatch.undo()
    return _rho_of(f'{sid}/{name}', bad, y16, y64, 'px', c['R']), c['R']


def _rollout_variant(swap=False, edge=False):
    def rollout(x):
        B, C3, H, W = x.shape
        v = x.reshape(B, 3, C3 // 3, H, W)
        parts = []
        for i in range(3):
            rowm = v[:, (i + 1) % 3].mean(-1, keepdim=True).expand(-1, -1, -1, W)
            colm = v[:, (i + 2) % 3].mean(-2, keepdim=True).expand(-1, -1, H, -1)
            parts += [v[:, i], colm, rowm] if swap else [v[:, i], rowm, colm]
        return torch.cat(parts, 1)
    if not edge:
        return rollout

    def group_conv(sd, p, x):
        """the pooled parts padded with their edge values instead of zeros (the plane itself keeps its zero padding)"""
        if 'roll_out_convs' not in p:
            return F.conv2d(odit._r(x), odit._r(sd[p + 'weight']), sd[p + 'bias'], padding=1, groups=3)
        B, C9, H, W = x.shape
        C = C9 // 9
        v = x.reshape(B, 3, 3, C, H, W)
        plane = F.pad(v[:, :, 0].reshape(B, 3 * C, H, W), (1, 1, 1, 1)).reshape(B, 3, 1, C, H + 2, W + 2)
        pooled = F.pad(v[:, :, 1:].reshape(B, 6 * C, H, W), (1, 1, 1, 1), mode='replicate').reshape(B, 3, 2, C, H + 2, W + 2)
        xp = torch.cat([plane, pooled], 2).reshape(B, C9, H + 2, W + 2)
        return F.conv2d(odit._r(xp), odit._r(sd[p + 'weight']), sd[p + 'bias'], padding=0, groups=3)
    return group_conv


@pytest.mark.parametrize("cls,name", [('shapenet', 'conv1'), ('ffhq', 'x0'), ('ffhq', 'planes')])
def test_defect_row_and_column_means_swapped(monkeypatch, cls, name):
    (rho, worst, _, failures), _ = _conv_defect(monkeypatch, f'{cls}-conv-r8-b2', name, lambda m: m.setattr(odd, 'rollout', _rollout_variant(swap=True)))
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst


@pytest.mark.parametrize("cls,name", [('shapenet', 'conv1'), ('ffhq', 'x0'), ('ffhq', 'planes')])
def test_defect_means_padded_with_their_edge_values(monkeypatch, cls, name):
    """only the border ring reads the padding: the defect is found there, and the interior is untouched"""
    (rho, worst, at, failures), Rr = _conv_defect(monkeypatch, f'{cls}-conv-r8-b2', name,
                                                 lambda m: m.setattr(odd, 'group_conv', _rollout_variant(edge=True)))
    r = rho.reshape(2, 3, Rr, Rr)
    border = torch.zeros(Rr, Rr, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert failures and at[2] in (0, Rr - 1) or at[3] in (0, Rr - 1)
    assert float((r[..., border] > CAP).float().mean()) > 0.9 and float(r[..., ~border].max()) <= CAP


@pytest.mark.parametrize("cls,name,axis", [('shapenet', 'conv0', 2), ('shapenet', 'conv1', 3), ('ffhq', 'x0', 3), ('ffhq', 'planes', 2),
                                           ('shapenet', 'upsample', 2)])
def test_defect_confined_to_the_last_row_or_column_of_one_plane(cls, name, axis):
    """what the ::8 sampling of the goldens never looks at: row / column R - 1 of plane 1 of object 1, off by half a percent"""
    if name == 'upsample':
        cid = 'shapenet-b3'
        ins, y64, y16 = R.stage_pair(cid, name)
        key, Rr, sd = f'{cid}/{name}', R.R_TIER_A, R.dec_sd(cls)
    else:
        sid = f'{cls}-conv-r16-b2'
        ins = _conv_stage_inputs(sid, name, R.single_inputs(sid))
        y64, y16 = R.single_pair(sid, name, ins)
        key, Rr, sd = f'{sid}/{name}', R.SINGLES[sid]['R'], R.single_sd(sid)
    bad = odd.to_cl(_standin(cls, sd, name, ins, Rr)).clone()
    idx = [1, 1, slice(None), slice(None)]
    idx[axis] = Rr - 1
    bad[tuple(idx)] *= 1.005
    rho, worst, at, failures = _rho_of(key, odd.to_nchw(bad), y16, y64, 'px', Rr)
    assert failures and at[:2] == (1, 1) and at[axis] == Rr - 1
    r = rho.reshape(-1, 3, Rr, Rr).clone()
    r[tuple(idx)] = 0
    assert float(r.max()) <= CAP                               # and nowhere else


def test_defect_leaky_slope(monkeypatch):
    """0.1 for 0.01: the ShapeNet class's residual step is an fp32 stage (the bound sees it), the FFHQ class's is inside its fused
    convolution (rho sees it)"""
    sid = 'shapenet-conv-r8-b1'
    ins = _conv_stage_inputs(sid, 'x0', R.single_inputs(sid))
    monkeypatch.setattr(odd, 'SLOPE', 0.1)
    bad = _standin('shapenet', R.single_sd(sid), 'x0', ins, 32)
    badf = _standin('ffhq', R.single_sd('ffhq-conv-r8-b1'), 'x0', R.single_inputs('ffhq-conv-r8-b1'), 32)
    monkeypatch.undo()
    with pytest.raises(AssertionError, match='beyond 6 fp32 ulps'):
        R.f32_check('shapenet', R.single_sd(sid), 'x0', tuple(t.float() for t in ins), bad, 'slope 0.1')
    R.f32_check('shapenet', R.single_sd(sid), 'x0', tuple(t.float() for t in ins), _standin('shapenet', R.single_sd(sid), 'x0', ins, 32), 'slope 0.01')
    y64, y16 = R.single_pair('ffhq-conv-r8-b1', 'x0', R.single_inputs('ffhq-conv-r8-b1'))
    rho, worst, _, failures = _rho_of('ffhq-conv-r8-b1/x0', badf, y16, y64, 'px', 32)
    assert failures and float((rho > CAP).float().mean()) > 0.3, worst      # the pixels with a negative channel of any size


def test_defect_short_cut_channel_mixing_as_a_plain_reshape(monkeypatch):
    cid = 'shapenet-b1'
    ins, y64, y16 = R.stage_pair(cid, 'short_cut')

    def plain(lat):
        B, C3, h, w = lat.shape
        return lat.reshape(B, 3, C3 // 3, h * w).permute(0, 1, 3, 2)
    good_view = odd.short_cut_view(ins[0])
    monkeypatch.setattr(odd, 'short_cut_view', plain)
    bad = _standin('shapenet', R.dec_sd('shapenet'), 'short_cut', ins)
    monkeypatch.undo()
    rho, worst, _, failures = _rho_of(f'{cid}/short_cut', bad, y16, y64, 'px', 64)
    assert failures and float((rho > CAP).float().mean()) > 0.9, worst
    assert not torch.equal(plain(ins[0]).to(torch.bfloat16), good_view.to(torch.bfloat16))      # the GPU test's exact check of `mixed`


def test_defect_ffhq_latent_relayout(monkeypatch):
    """B z 3 L -> B 3 L z done as B 3 z L: the fp32 bound of the embedding sees it"""
    cid = 'ffhq-b1'
    ins, _, _ = R.stage_pair(cid, 'embed')

    def wrong(latent):
        B, C3, h, _ = latent.shape
        return latent.reshape(B, 3, C3 // 3, h * h).permute(0, 1, 3, 2).reshape(B, 3 * h * h, C3 // 3)
    good = _standin('ffhq', R.dec_sd('ffhq'), 'embed', ins)
    R.f32_check('ffhq', R.dec_sd('ffhq'), 'embed', ins, good, 'stand-in')
    tok = wrong(ins[0])
    sd = R.dec_sd('ffhq')
    bad = F.linear(tok, sd[odd.SR + 'ldm_upsample.weight'], sd[odd.SR + 'ldm_upsample.bias'])
    with pytest.raises(AssertionError, match='beyond 392 fp32 ulps'):
        R.f32_check('ffhq', sd, 'embed', ins, bad, 're-layout')


# ------------------------------------------------------------------------------------------------ what the criterion does not see
def test_defect_dropped_low_part_launch_is_seen_but_barely_in_a_fusion_group(monkeypatch):
    """The FFHQ class's second accumulating launch (the bf16 low part of a residual-stream weight) dropped: the weights fall back to a
    single bf16.  The issue expected this to hide under cap 1; measured on the CPU (fp32 stand-in against the oracle pair) it does not:
    skip3 - two bare projections, the weight rounding is as large as everything d holds - worst rho 1.70, 92 % of the tokens over 1.0;
    a whole fusion group worst 1.46 (group0) / 1.35 (group3) with 39 % / 34 % of the tokens over 1.0 and a MEDIAN of 0.96.  So the
    criterion sees the defect at every stage that has such a projection, clearly at a skip step and by a third of the tokens in a
    fusion group: a cap of 1.0 is the lowest at which a group would still show it."""
    cid = 'ffhq-b1'
    found = {}
    for name in ('skip3', 'group0', 'group3'):
        ins, y64, y16 = R.stage_pair(cid, name)
        monkeypatch.setattr(odd, 'res_linear', lambda x, w, b=None, pair=False: odit.linear(x, w, b))
        bad = _standin('ffhq', R.dec_sd('ffhq'), name, ins)
        monkeypatch.undo()
        rho, worst, _, failures = _rho_of(f'{cid}/{name}: no low part', bad, y16, y64, 'tok')
        found[name] = (worst, float((rho > CAP).float().mean()), float(rho.median()))
        assert failures
    print(found)
    assert found['skip3'][0] > 1.5 and found['skip3'][1] > 0.8
    for g in ('group0', 'group3'):
        assert 1.2 < found[g][0] < 2.0 and 0.2 < found[g][1] < 0.6 and 0.8 < found[g][2] < 1.1, found


def test_defect_single_bf16_ldm_upsample_is_seen():
    """The FFHQ embedding as one bf16 product (no low halves).  The stage has no rounding in the oracle (d = 0: rho does not exist for
    it); held to its fp32 bound it is seen - up to 2^-7 of the terms against 392 ulps = 2^-14.4 - both at the latents of
    ffhq-embed-lowhalf, whose entries all need their low half, and at the plain latents of tier A.  The issue expected it to be hidden
    at cap 1.  It is not, whichever way it is looked at: measured one stage on (group0 fed the single-bf16 embedding, d from group0's
    own oracle pair) the median rho is 1.5 and 99.5 % of the tokens are over 1.0 at the plain latents (16 and 99.7 % at the low-half
    ones) - the error rides the residual stream through the group, whose own operand rounding moves a token by less than 2^-8 of it."""
    for sid, ins in (('ffhq-embed-lowhalf', R.single_inputs('ffhq-embed-lowhalf')), ('ffhq-b1', R.stage_pair('ffhq-b1', 'embed')[0])):
        tok = odd.ffhq_tokens(ins[0])
        sd = R.dec_sd('ffhq')
        w, b = sd[odd.SR + 'ldm_upsample.weight'], sd[odd.SR + 'ldm_upsample.bias']
        xh, wh = tok.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
        xl, wl = (tok - xh).to(torch.bfloat16).float(), (w - wh).to(torch.bfloat16).float()
        if sid == 'ffhq-embed-lowhalf':                        # the case is what it says: magnitudes over 2^-6 .. 2^6, low halves needed
            assert float((xl != 0).float().mean()) > 0.95
            assert float(tok.abs().max()) > 2.0 ** 5 and float(tok.abs().median()) < 4 and float(tok.abs().min()) < 2.0 ** -5
        single = F.linear(xh, wh, b)
        with pytest.raises(AssertionError, match='beyond 392 fp32 ulps'):
            R.f32_check('ffhq', sd, 'embed', ins, single, f'{sid} single bf16')
        split = (F.linear(xh.double(), wh.double(), b.double()) + F.linear(xh.double(), wl.double()) + F.linear(xl.double(), wh.double())).float()
        R.f32_check('ffhq', sd, 'embed', ins, split, f'{sid} split product')
        # one stage on: group0 fed the single-bf16 embedding (+ pos_embed) instead of the exact one
        exact = odd.add_pos(R.to64(sd), F.linear(tok.double(), w.double(), b.double()))
        y64, y16 = R.run_stage(sd, 'ffhq', 'group0', (exact,), rounded=False), R.run_stage(sd, 'ffhq', 'group0', (exact,))
        bad = R.run_stage(sd, 'ffhq', 'group0', (odd.add_pos(R.to64(sd), single.double()),))
        rho, _ = R.group_rho(bad, y16, y64, 'tok')
        print(f'{sid}: single-bf16 embedding through group0: worst rho {float(rho.max()):.3g}, median {float(rho.median()):.3g}, over 1.0: '
              f'{float((rho > CAP).float().mean()):.3f}')
        assert float((rho > CAP).float().mean()) > 0.9
