"""Every stage of the ShapeNet and FFHQ VAE decoder classes on the HIP kernels, judged per token / per pixel against the float64 oracle
(tests/dino_decoder_refs.py, oracle/dino_decoder.py):

    rho = ||y_hip - y16|| / max(||y16 - y64||, 0.1 median)  <=  CAP          per token or (object, plane, y, x), every group counted

with the stage's input the same for the HIP stage and both oracles; the stages without a bf16 operand (d = 0) are held to first-order
fp32 bounds against float64 instead.  The wiring between the stages is checked exactly: the stage methods chained by hand give the
class's own vit_decode_backbone + vit_decode_postprocess bit for bit.

Tier A walks both decoders (D = 128, 2 heads, 12 blocks) at B = 1 and B = 3; tier B drives single stages at the smallest shapes that can
still go wrong; the ShapeNet class's vae_reparameterization is judged per encoder token (ldm_downsample) and by the fp32 bound (the
posterior)."""
import math

import pytest
import torch

import dino_decoder_refs as R
import kernel_refs as kr
from oracle import dino_decoder as odd

pytestmark = pytest.mark.gpu

# CAP: the rule of tests/test_decode_gpu.py::stage_cap - twice the worst rho measured on the MI355X, rounded up to one digit, never
# above 1.0 - per (case, stage).  Measured against the oracle pair, tile choice left to the library.  The stage kinds differ by orders of
# magnitude (tier A, B = 1 .. B = 3; tier B where it differs):
#   one GEMM on given operands (skip_linear, decoder_pred, short_cut, ldm_downsample): what is left is the fp32 summation order,
#     3e-5 .. 1.5e-4;
#   a convolution on given operands (ShapeNet conv0, FFHQ x0): 3e-4 .. 1.6e-3; one that rounds its own row / column means first
#     (ShapeNet conv1, FFHQ planes): median 8e-5, worst 2e-4 .. 0.17 - a mean that fell on the other side of a bf16 boundary is read by
#     a whole row or column of pixels;
#   a fusion group (two or three attentions and their GEMMs, each re-rounding the stream): median ShapeNet 2e-4 .. 0.13, FFHQ
#     0.09 .. 0.36; worst ShapeNet 0.42 .. 0.79, FFHQ 0.52 .. 0.95 - rounding-boundary flips, the size the fp32 stand-in of the oracle
#     shows against itself (tests/test_dino_decoder_pixels_cpu.py: ShapeNet 0.40 .. 0.80); one cross-plane block or fusion block alone
#     (tier B): 0.23 .. 0.40;
#   upsample (an fp32 blend rounded to bf16): median 0, worst 0.56 .. 0.94 - single elements on a rounding boundary, one bf16 ulp against
#     the rounding of 128 channels.
# No stage of the correct code exceeded 1.0 and none needed a rounding point beyond those oracle/dino_decoder.py names.
MEASURED = {
    'shapenet-b1/group0': 0.691, 'shapenet-b1/group1': 0.643, 'shapenet-b1/group2': 0.675, 'shapenet-b1/skip3': 6.8e-05,
    'shapenet-b1/group3': 0.421, 'shapenet-b1/skip4': 7.7e-05, 'shapenet-b1/group4': 0.641, 'shapenet-b1/skip5': 6.8e-05,
    'shapenet-b1/group5': 0.482, 'shapenet-b1/decoder_pred': 3.4e-05, 'shapenet-b1/short_cut': 7.3e-05, 'shapenet-b1/upsample': 0.564,
    'shapenet-b1/conv0': 3.5e-04, 'shapenet-b1/conv1': 0.173, 'shapenet-b3/group0': 0.742, 'shapenet-b3/group1': 0.790,
    'shapenet-b3/group2': 0.739, 'shapenet-b3/skip3': 7.3e-05, 'shapenet-b3/group3': 0.565, 'shapenet-b3/skip4': 6.8e-05,
    'shapenet-b3/group4': 0.568, 'shapenet-b3/skip5': 7.4e-05, 'shapenet-b3/group5': 0.655, 'shapenet-b3/decoder_pred': 3.7e-05,
    'shapenet-b3/short_cut': 7.2e-05, 'shapenet-b3/upsample': 0.918, 'shapenet-b3/conv0': 3.9e-04, 'shapenet-b3/conv1': 0.082,
    'ffhq-b1/group0': 0.720, 'ffhq-b1/group1': 0.846, 'ffhq-b1/group2': 0.940, 'ffhq-b1/skip3': 1.4e-04, 'ffhq-b1/group3': 0.563,
    'ffhq-b1/skip4': 1.5e-04, 'ffhq-b1/group4': 0.515, 'ffhq-b1/skip5': 1.2e-04, 'ffhq-b1/group5': 0.535,
    'ffhq-b1/decoder_pred': 3.6e-05, 'ffhq-b1/short_cut': 8.9e-05, 'ffhq-b1/upsample': 0.867, 'ffhq-b1/x0': 8.8e-04,
    'ffhq-b1/planes': 7.1e-03, 'ffhq-b3/group0': 0.949, 'ffhq-b3/group1': 0.894, 'ffhq-b3/group2': 0.859, 'ffhq-b3/skip3': 1.5e-04,
    'ffhq-b3/group3': 0.857, 'ffhq-b3/skip4': 1.4e-04, 'ffhq-b3/group4': 0.693, 'ffhq-b3/skip5': 1.4e-04, 'ffhq-b3/group5': 0.671,
    'ffhq-b3/decoder_pred': 3.5e-05, 'ffhq-b3/short_cut': 8.2e-05, 'ffhq-b3/upsample': 0.945, 'ffhq-b3/x0': 1.4e-03,
    'ffhq-b3/planes': 0.012, 'shapenet-cross-b1/cross': 0.235, 'shapenet-cross-b2/cross': 0.402, 'shapenet-skip/skip3': 6.1e-05,
    'shapenet-conv-r8-b1/conv0': 3.2e-04, 'shapenet-conv-r8-b1/conv1': 5.3e-04, 'shapenet-conv-r8-b2/conv0': 3.1e-04,
    'shapenet-conv-r8-b2/conv1': 1.9e-04, 'shapenet-conv-r16-b1/conv0': 3.9e-04, 'shapenet-conv-r16-b1/conv1': 0.078,
    'shapenet-conv-r16-b2/conv0': 3.2e-04, 'shapenet-conv-r16-b2/conv1': 2.4e-04, 'shapenet-conv-narrow/conv0': 3.4e-04,
    'shapenet-conv-narrow/conv1': 3.0e-04, 'ffhq-cross-b1/cross': 0.332, 'ffhq-cross-b2/cross': 0.256, 'ffhq-skip/skip3': 1.5e-04,
    'ffhq-conv-r8-b1/x0': 7.7e-04, 'ffhq-conv-r8-b1/planes': 5.0e-03, 'ffhq-conv-r8-b2/x0': 7.7e-04, 'ffhq-conv-r8-b2/planes': 3.0e-04,
    'ffhq-conv-r16-b1/x0': 8.6e-04, 'ffhq-conv-r16-b1/planes': 3.0e-04, 'ffhq-conv-r16-b2/x0': 1.6e-03,
    'ffhq-conv-r16-b2/planes': 0.095, 'reparam/ldm_downsample-mode': 7.4e-05, 'reparam/ldm_downsample-sampled': 7.4e-05,
}


def cap_of(measured):
    v = 2.0 * measured
    p = 10.0 ** math.floor(math.log10(v))
    return min(1.0, math.ceil(v / p - 1e-9) * p)


def cap(key):
    return cap_of(MEASURED[key])


def _rho_keys():
    keys = [f'{cid}/{n}' for cid, c in R.TIER_A.items() for n in R.stage_names(c['cls']) if n not in R.f32_stages(c['cls'])]
    for sid, c in R.SINGLES.items():
        if not c.get('refused'):
            keys += [f'{sid}/{n}' for n in R.single_stages(sid) if n not in R.f32_stages(c['cls'])]
    return keys + ['reparam/ldm_downsample-mode', 'reparam/ldm_downsample-sampled']


assert set(MEASURED) == set(_rho_keys()), set(MEASURED) ^ set(_rho_keys())
assert all(cap_of(v) <= 1.0 for v in MEASURED.values())

_DECS = {}
DEV = 'cuda'


def _dec(cls, conv_sr=None):
    key = (cls, conv_sr)
    if key not in _DECS:
        dec = R.loaded_dec(cls, conv_sr=conv_sr, R=R.R_TIER_A).cuda()
        dec._ensure_packed(torch.device(DEV))
        _DECS[key] = dec
    return _DECS[key]


def _cl(x):
    """oracle NCHW [B, 3C, R, R] -> the product's channel-last [B, 3, R, R, C] on the device"""
    return odd.to_cl(x).contiguous().to(DEV)


def _nchw(x_cl):
    return odd.to_nchw(x_cl.float()).cpu()


def _rows(x):
    """[B, L, D] fp32 -> a fresh [B*L, D] residual stream on the device"""
    return x.contiguous().reshape(-1, x.shape[-1]).to(DEV).clone()


def _embed(dec, latent):
    """the raw tokens vit_decode_backbone hands to forward_vit_decoder (and the ViT output)"""
    st = {}
    orig = dec.forward_vit_decoder

    def fwd(x, img_size=None):
        st['raw'] = x.clone()
        return orig(x, img_size)
    dec.forward_vit_decoder = fwd
    try:
        st['vit'] = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': latent.to(DEV)}, 128)
    finally:
        del dec.forward_vit_decoder
    return st


def _hip_stage(dec, cls, name, ins, R_):
    """one stage of the product on fp32 inputs from the host -> {oracle stage name: output on the host, in the oracle's layout}.  The
    ShapeNet class's conv steps give two oracle stages each: the convolution (scratch 't') and the residual step."""
    P = dec._packed
    H = P['H']
    if name == 'embed':
        return {name: _embed(dec, ins[0])['raw'].cpu()}
    if name == 'pos':
        B, L, Dm = ins[0].shape
        h = torch.empty(B * L, Dm, device=DEV)
        dec._add_pos(ins[0].contiguous().to(DEV), h)
        return {name: h.view(B, L, Dm).cpu()}
    if name.startswith('skip') or name.startswith('group') or name == 'cross':
        B, L, Dm = ins[0].shape
        h = _rows(ins[0])
        if name.startswith('skip'):
            s = ins[1].contiguous().to(DEV).to(torch.bfloat16)
            assert torch.equal(s.float().cpu(), ins[1])                     # a skip is a bf16 tensor: nothing is lost handing it over
            dec._skip_step(h, P['groups'][int(name[4:])], s.reshape(B * L, Dm).contiguous())
        elif name == 'cross':
            if cls == 'shapenet':
                dec._cross_block(h, P['groups'][0]['b1'], B, L // 3, H)
            else:
                dec._fusion(h, P['groups'][0], B, L // 3, H)
        else:
            dec._group(h, P['groups'][int(name[5:])], B, L // 3, H)
        return {name: h.view(B, L, Dm).cpu()}
    if name == 'norm':
        B, L, Dm = ins[0].shape
        out = torch.empty(B * L, Dm, device=DEV)
        dec._final_norm(_rows(ins[0]), out)
        return {name: out.view(B, L, Dm).cpu()}
    if name == 'decoder_pred':
        B, L, _ = ins[0].shape
        return {name: dec._pred(ins[0].contiguous().to(DEV)).view(B, L, -1).cpu()}
    if name == 'unpatchify':
        B, L, PC = ins[0].shape
        lo, mixed = dec._unpatchify(ins[0].reshape(B * L, PC).to(DEV).contiguous(), B)
        r = lo.shape[1]
        lo = lo.view(B, 3, r, r, -1)
        want = odd.short_cut_view(odd.to_nchw(lo)).to(torch.bfloat16)       # [B, 3, r*r, Cm]: channel 3k + e of the planes, bf16
        assert torch.equal(mixed.view(want.shape), want), 'short_cut input is not the (3k + e) channel mix of the planes'
        return {name: _nchw(lo)}
    if name == 'short_cut':
        B = ins[0].shape[0]
        mixed = odd.short_cut_view(ins[0]).to(torch.bfloat16).reshape(-1, ins[0].shape[1] // 3).contiguous().to(DEV)
        return {name: _nchw(dec._short_cut(mixed, B))}
    if name == 'upsample':
        B, C3, r, _ = ins[0].shape
        lo = _cl(ins[0]).reshape(B * 3, r, r, C3 // 3)
        return {name: _nchw(dec._upsample(lo, B, R_))}
    raise KeyError(name)


def _hip_conv(dec, cls, up, res, B, r, R_, Cm, Co, x0_in=None):
    """the two conv steps of conv_sr.  up NCHW bf16-exact fp32, res NCHW fp32 (host) -> dict of oracle stage name -> (inputs, output);
    the second step runs on x0_in (host NCHW) when given, else on the first step's own output."""
    out = {}
    ws = dec._ws
    up_d = _cl(up).to(torch.bfloat16)
    assert torch.equal(up_d.float().cpu(), odd.to_cl(up))
    res_d = _cl(res)
    x0 = dec._conv_x0(up_d, res_d, B, r, R_, Cm, Co)
    x0_h = _nchw(x0)
    if cls == 'shapenet':
        t0 = _nchw(ws.get('t', (B * 3, R_ * R_, Co), torch.float32).view(B, 3, R_, R_, Co))
        out['conv0'] = ((up,), t0)
        out['x0'] = ((res, t0), x0_h)
    else:
        out['x0'] = ((up, res), x0_h)
    x0_src = x0_h if x0_in is None else x0_in
    x0_d = ws.get('x0', (B, 3, R_, R_, Co), torch.float32)
    x0_d.copy_(_cl(x0_src))
    planes = torch.empty(B, 3, R_, R_, Co, device=DEV)
    dec._conv_planes(x0_d, planes, B, R_, Co)
    if cls == 'shapenet':
        t1 = _nchw(ws.get('t', (B * 3, R_ * R_, Co), torch.float32).view(B, 3, R_, R_, Co))
        out['conv1'] = ((x0_src,), t1)
        out['planes'] = ((x0_src, t1), _nchw(planes))
    else:
        out['planes'] = ((x0_src,), _nchw(planes))
    return out


def _judge_stage(key_prefix, cls, sd, name, ins, y_hip, pair, failures, R_):
    """rho against the oracle pair, or the fp32 bound where the stage has no bf16 operand"""
    if name in R.f32_stages(cls):
        y = y_hip.reshape(-1, y_hip.shape[-1]) if name == 'norm' else y_hip
        worst = R.f32_check(cls, sd, name, ins, y, f'{key_prefix}/{name}')
        print(f'{key_prefix}/{name}: fp32 stage, worst {worst / kr.F32_EPS:.3g} ulps of the terms')
        return
    y64, y16 = pair
    key = f'{key_prefix}/{name}'
    R.judge(key, y_hip, y16, y64, R.stage_kind(name), cap(key), failures,
            R_ if R.stage_kind(name) == 'px' else None)


# ------------------------------------------------------------------------------------------------ tier A
@pytest.mark.parametrize("cid", list(R.TIER_A))
def test_every_stage_of_the_decoder_every_group(hip_lib, cid):
    c = R.TIER_A[cid]
    cls, B = c['cls'], c['B']
    assert B * 3 * R.HEADS < torch.cuda.get_device_properties(0).multi_processor_count      # never the K-resident attention kernel
    dec, sd = _dec(cls), R.dec_sd(cls)
    failures = []
    conv_names = ('conv0', 'x0', 'conv1', 'planes')
    for name in R.stage_names(cls):
        if name in conv_names:
            continue
        ins, y64, y16 = R.stage_pair(cid, name)
        y = _hip_stage(dec, cls, name, ins, R.R_TIER_A)[name]
        _judge_stage(cid, cls, sd, name, ins, y, (y64, y16), failures, R.R_TIER_A)
    # conv_sr: the first step on the oracle's taps, the second on the tap of x0 (both oracles and the HIP step get the same x0)
    first = 'conv0' if cls == 'shapenet' else 'x0'
    up = R.stage_pair(cid, first)[0][0]
    res = R.stage_pair(cid, 'x0')[0][0 if cls == 'shapenet' else 1]
    x0_tap = R.stage_pair(cid, 'conv1' if cls == 'shapenet' else 'planes')[0][0]
    got = _hip_conv(dec, cls, up, res, B, 64, R.R_TIER_A, R.CM, R.CO, x0_in=x0_tap)
    for name, (ins, y) in got.items():
        pair = None
        if name not in R.f32_stages(cls):                    # a rho stage: its inputs are the oracle's taps, bit for bit
            taps_in, y64, y16 = R.stage_pair(cid, name)
            assert len(ins) == len(taps_in) and all(torch.equal(a, b) for a, b in zip(ins, taps_in)), name
            pair = (y64, y16)
        _judge_stage(cid, cls, sd, name, ins, y, pair, failures, R.R_TIER_A)
    assert not failures, failures


@pytest.mark.parametrize("cid", list(R.TIER_A))
def test_forward_is_exactly_the_stages_in_the_oracles_order(hip_lib, cid):
    """The stage methods chained by hand, each fed the one before it and the skips popped last in, first out, equal
    vit_decode_backbone + vit_decode_postprocess bit for bit; planes_channel_last is latent_after_vit in the other layout."""
    from ln3diff_amd import ops
    c = R.TIER_A[cid]
    cls, B = c['cls'], c['B']
    dec = _dec(cls)
    P, H = dec._packed, dec._packed['H']
    lat = R.latent(cid)
    st = _embed(dec, lat)
    blk = {}
    dec.stage_hook = lambda n, t: blk.__setitem__(n, t.clone())
    try:
        vit = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': lat.to(DEV)}, 128).clone()
    finally:
        del dec.stage_hook
    assert torch.equal(vit, st['vit']) and list(blk) == [f'blk{j}' for j in range(6)]
    ret = dec.vit_decode_postprocess(vit, {}, return_stages=True)
    want = {k: v.clone() for k, v in ret.items() if torch.is_tensor(v)}
    # ---- by hand
    L, Dm = 768, R.D
    h = torch.empty(B * L, Dm, device=DEV)
    dec._add_pos(st['raw'], h)
    bf = lambda t: t.to(torch.bfloat16)
    skips = [bf(h)]
    for j, q in enumerate(P['groups']):
        if j >= 3:
            dec._skip_step(h, q, skips.pop())
        dec._group(h, q, B, L // 3, H)
        assert torch.equal(h.view(B, L, Dm), blk[f'blk{j}']), j
        if j < 2:
            skips.append(bf(h))
    assert not skips
    tok = torch.empty(B * L, Dm, device=DEV)
    dec._final_norm(h, tok)
    assert torch.equal(tok.view(B, L, Dm), vit)
    pred = dec._pred(tok.view(B, L, Dm))
    assert torch.equal(pred.view(B, L, -1), want['decoder_pred'])
    lo, mixed = dec._unpatchify(pred, B)
    assert torch.equal(lo.view(B, 3, 64, 64, -1), want['planes_lowres'])
    res = dec._short_cut(mixed, B)
    up = dec._upsample(lo, B, R.R_TIER_A)
    x0 = dec._conv_x0(up, res, B, 64, R.R_TIER_A, R.CM, R.CO)
    if cls == 'ffhq':
        assert torch.equal(x0, want['x0'])
    planes = torch.empty(B, 3, R.R_TIER_A, R.R_TIER_A, R.CO, device=DEV)
    dec._conv_planes(x0, planes, B, R.R_TIER_A, R.CO)
    assert torch.equal(planes, want['planes_channel_last'])
    assert torch.equal(odd.to_nchw(want['planes_channel_last']), want['latent_after_vit'])
    # bf16 casts of torch and of ln3d_cast_f32_bf16 agree (the skips above were made with torch's)
    s = torch.empty(B * L, Dm, device=DEV, dtype=torch.bfloat16)
    ops.cast_bf16(h, s)
    assert torch.equal(s, bf(h))
    # end to end against the rounded oracle, for the record (not gated: see tests/test_unet_pixels_cpu.py)
    y16 = R.case_taps(cid)['planes'][1]
    print(f'{cid}: end to end planes rel-L2 against y16 {float((odd.to_nchw(planes).cpu().double() - y16).norm() / y16.norm()):.2e}')


# ------------------------------------------------------------------------------------------------ tier B
CROSS_SKIP_EMBED = [s for s, c in R.SINGLES.items() if c['kind'] in ('cross', 'skip', 'embed')]
CONVS = [s for s, c in R.SINGLES.items() if c['kind'] == 'conv']


@pytest.mark.parametrize("sid", CROSS_SKIP_EMBED)
def test_single_stage_every_token(hip_lib, sid):
    c = R.SINGLES[sid]
    cls = c['cls']
    dec, sd = _dec(cls), R.single_sd(sid)
    ins = R.single_inputs(sid)
    name = R.single_stages(sid)[0]
    y = _hip_stage(dec, cls, name, ins, None)[name]
    failures = []
    pair = None if name in R.f32_stages(cls) else R.single_pair(sid, name, ins)
    _judge_stage(sid, cls, sd, name, ins, y, pair, failures, None)
    assert not failures, failures


@pytest.mark.parametrize("sid", CONVS)
def test_conv_sr_called_directly_every_pixel_borders_included(hip_lib, sid):
    c = R.SINGLES[sid]
    cls, B, r, R_, Cm, Co = c['cls'], c['B'], c['r'], c['R'], c['Cm'], c['Co']
    dec, sd = _dec(cls, c['conv_sr']), R.single_sd(sid)
    up, res = R.single_inputs(sid)
    if c['refused']:                                         # the fused kernel takes Cout % 32 == 0 only: an error, never another route
        with pytest.raises((RuntimeError, ValueError)):
            dec._conv_x0(_cl(up).to(torch.bfloat16), _cl(res), B, r, R_, Cm, Co)
        return
    got = _hip_conv(dec, cls, up, res, B, r, R_, Cm, Co)
    failures = []
    for name, (ins, y) in got.items():
        pair = None if name in R.f32_stages(cls) else R.single_pair(sid, name, ins)
        if pair is not None:
            assert pair[0].shape[-1] == R_ and R.group_rho(y.double(), pair[1], pair[0], 'px')[0].numel() == B * 3 * R_ * R_
        _judge_stage(sid, cls, sd, name, ins, y, pair, failures, R_)
    # the whole step through _conv_sr is the two halves
    planes = torch.empty(B, 3, R_, R_, Co, device=DEV)
    dec._conv_sr(_cl(up).to(torch.bfloat16), _cl(res), planes, B, r, R_, Cm, Co)
    assert torch.equal(_nchw(planes), got['planes'][1])
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ the ShapeNet encoder side
@pytest.mark.parametrize("sampled", [False, True], ids=['mode', 'sampled'])
def test_shapenet_vae_reparameterization_per_token_and_posterior_by_the_fp32_bound(hip_lib, sampled):
    dec = _dec('shapenet')
    tok, eps = R.reparam_inputs()
    eps = eps if sampled else None
    seen = {}
    orig = dec._posterior

    def spy(h, e, num_frames):
        seen['h'] = h.clone()
        return orig(h, e, num_frames)
    dec._posterior = spy
    try:
        ret = dec.vae_reparameterization(tok.to(DEV), sampled, eps=eps)
    finally:
        del dec._posterior
    y64, y16 = R.reparam_pair(None if eps is None else eps.double())
    h = seen['h'].cpu()
    assert h.shape == y64['h'].shape == (2, 24, 32, 32)
    failures = []
    key = f"reparam/ldm_downsample-{'sampled' if sampled else 'mode'}"
    R.judge(key, R.reparam_tokens(h), R.reparam_tokens(y16['h']), R.reparam_tokens(y64['h']), 'tok', cap(key), failures)
    assert not failures, failures
    # the posterior on the HIP path's own h: fp32, held to the bound of its kernel test
    sd = R.dec_sd('shapenet')
    qw = sd[odd.SR + 'quant_conv.weight'].reshape(24, 8)
    ref = kr.mv_posterior(h.reshape(2, 24, 1024), qw, sd[odd.SR + 'quant_conv.bias'], eps, 2, 1)
    out = dict(mean=ret['posterior'].mean, logvar=ret['posterior'].logvar, z=ret['latent_normalized_2Ddiffusion'].reshape(2, 4, 3, 1024),
               latent_tok=ret['latent_normalized'], log_q=ret['log_q'], entropy=ret['normal_entropy'])
    for k, y in out.items():
        kr.assert_f32_close(y, *ref[k], ref['ulps'], what=f'reparam {k} sampled={sampled}')
    assert torch.equal(ret['log_q_2Ddiffusion'].reshape(2, 4, 3, 1024), ret['log_q'])
    if not sampled:
        assert torch.equal(out['z'], out['mean'])
    # and the oracle's own posterior of that h agrees with the kernel reference (the two restatements are one)
    mine = odd.posterior(R.to64(sd), h.double(), None if eps is None else eps.double())
    for k in ('mean', 'logvar', 'z', 'log_q', 'entropy', 'latent_tok'):
        assert float((mine[k] - ref[k][0]).abs().max()) <= 1e-12 * (1 + float(ref[k][0].abs().max())), k
