"""Every stage of the multi-view VAE encoder on the HIP kernels, judged per pixel against the float64 oracle
(tests/encoder_pixel_refs.py):

    rho = ||y_hip - y16|| / max(||y16 - y64||, 0.1 median)  <=  CAP          per (frame, y, x), every pixel counted

with the stage's input x_in the same for the HIP stage and both oracles.  Every stage is launched through Encoder._run_step, a spy on
ConvStack.self_attend asserts the path attn1 and attn2 took (head size, tokens per sequence, the `padded` flag that selects o1p / o2p),
the packed shortcuts are the stated form, and - for the three walked networks - the steps chained by hand equal forward_frames bit
for bit: the stages are right per pixel and the forward is exactly those stages in the oracle's order."""
import math

import pytest
import torch

import encoder_pixel_refs as R
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu

# CAP.  The rule of tests/test_unet_pixels_gpu.py (cap_of): twice the worst measured rho, rounded up to one digit, never above 1.0,
# per (case, stage), because the stage kinds differ by orders of magnitude.  A conv alone (conv_in, a Downsample) has no rounding
# inside it: what is left is the fp32 summation order, rho 5e-5 .. 2e-4.  A ResnetBlock rounds its activation twice behind a GroupNorm:
# the median pixel stays at 3e-5 .. 2e-4, the worst is a pixel under a bf16 operand that fell on the other side of a rounding boundary,
# 0.10 .. 0.96 (the more pixels and the narrower the block, the likelier and the larger: 0.96 at 36 864 pixels x 32 channels, where
# two ResnetBlocks are chained).  The transformer re-rounds its token stream nine times: median 0.4 .. 0.5, worst 0.63 .. 0.84.  That
# is the size the oracle shows against itself at fp32 working precision, stage by stage (tests/test_encoder_pixels_cpu.py: 0.49 / 0.75 /
# 0.96 for the three down0, 0.72 .. 0.78 for mid_attn_1).  No case needed a rounding point beyond those oracle.dit.operand_rounding
# names, no stage exceeded 1.0 and none needed a change in the product.
# measured: worst rho of every (case, stage) on gfx950 (MI355X), tile choice left to the library
MEASURED = {
    'rel64/conv_in': 5.8e-05, 'rel64/down0': 0.655, 'rel64/down0_ds': 1.2e-04, 'rel64/down1': 0.237, 'rel64/down1_ds': 1.4e-04,
    'rel64/down2': 0.264, 'rel64/down2_ds': 1.6e-04, 'rel64/down3': 0.172, 'rel64/mid_block_1': 0.253, 'rel64/mid_attn_1': 0.718,
    'rel64/mid_block_2': 0.331, 'rel64/conv_out': 0.096, 'ch32-128/conv_in': 8.9e-05, 'ch32-128/down0': 0.858,
    'ch32-128/down0_ds': 1.2e-04, 'ch32-128/down1': 0.382, 'ch32-128/down1_ds': 1.2e-04, 'ch32-128/down2': 0.185,
    'ch32-128/down2_ds': 1.4e-04, 'ch32-128/down3': 0.314, 'ch32-128/mid_block_1': 0.130, 'ch32-128/mid_attn_1': 0.723,
    'ch32-128/mid_block_2': 0.262, 'ch32-128/conv_out': 0.062, 'dh48-rect/conv_in': 4.7e-05, 'dh48-rect/down0': 0.963,
    'dh48-rect/down0_ds': 1.2e-04, 'dh48-rect/down1': 0.564, 'dh48-rect/down1_ds': 1.1e-04, 'dh48-rect/down2': 0.401,
    'dh48-rect/down2_ds': 1.3e-04, 'dh48-rect/down3': 0.406, 'dh48-rect/mid_block_1': 0.101, 'dh48-rect/mid_attn_1': 0.790,
    'dh48-rect/mid_block_2': 0.240, 'dh48-rect/conv_out': 0.046, 'f9-6x6': 0.728, 'f1-16x16': 0.635, 'f2-8x16': 0.788,
    'f8-8x8': 0.675, 'obj3-f5': 0.700, 'dh16': 0.838, 'dh80': 0.628, 'dh128': 0.733, 'dh12': 0.701, 'depth2': 0.791,
    'ds-8x24-c32': 8.4e-05, 'ds-16x16-c256': 1.6e-04, 'cin3': 4.9e-05, 'cin10': 5.9e-05, 'cin16': 6.6e-05, 'out-24': 0.197,
}


def cap_of(measured):
    v = 2.0 * measured
    p = 10.0 ** math.floor(math.log10(v))
    return min(1.0, math.ceil(v / p - 1e-9) * p)


assert set(MEASURED) == set(R.ids()) and all(cap_of(v) <= 1.0 for v in MEASURED.values())

_MODELS = {}
RAISES = 'tokens per sequence need the MFMA attention kernels'


def _enc(cfg_name):
    if cfg_name not in _MODELS:
        m = R.build_enc(cfg_name)
        m.load_state_dict(R.cfg_sd(cfg_name), strict=True)
        _MODELS[cfg_name] = m.cuda()
    return _MODELS[cfg_name]


def _cl(x):
    """NCHW -> channel-last rows [N*H*W, C] on the device"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous().cuda()


def _nchw(h, N, H, W):
    return h.reshape(N, H, W, -1).permute(0, 3, 1, 2).cpu()


def _step(enc, name, x_in):
    """one step on an NCHW fp32 input from the host -> its NCHW output on the host"""
    N, _, H, W = x_in.shape
    h, H, W = enc._run_step(name, x_in.cuda() if name == 'conv_in' else _cl(x_in), N, H, W)
    return _nchw(h, N, H, W)


def _spy(monkeypatch, enc):
    """records (head size, sequences, tokens, padded) of every ConvStack.self_attend of the encoder's runner (packed by now: a pack made
    later would bring a new runner)"""
    cs = enc._cs
    log, orig = [], cs.self_attend

    def self_attend(a_bf, q_qkv, B, L, heads, dh, tag):
        o, padded = orig(a_bf, q_qkv, B, L, heads, dh, tag)
        log.append((dh, B, L, padded))
        return o, padded
    monkeypatch.setattr(cs, 'self_attend', self_attend)
    return log


def _stated_attention(cid):
    """what the spy must have seen for one mid_attn_1 of a case: attn1 then attn2, once per transformer block"""
    c, cfg = R.CASES[cid], R.case_cfg(cid)
    one = [(cfg['d_head'], c['objects'], c['attn1'][0], c['attn1'][1] != 'small'), (cfg['d_head'], c['N'], c['attn2'][0], c['attn2'][1] != 'small')]
    return one * cfg['depth']


def _judge(key, y_hip, y16, y64, failures):
    rho, d = R.pixel_rho(y_hip.double(), y16, y64)
    where, worst = R.worst_pixel(rho)
    cap = cap_of(MEASURED[key])
    print(f'{key}: worst pixel (frame, pixel) = {where}, rho = {worst:.4g}; median rho {float(rho.median()):.3g}; d median '
          f'{float(d.median()):.3e}; pixels {rho.numel()} (measured: worst {MEASURED[key]}, cap {cap:g})')
    assert torch.isfinite(rho).all()
    if not worst <= cap:
        failures.append((key, where, worst, cap))


@pytest.mark.parametrize("cid", R.WALKED)
def test_every_stage_of_the_network_every_pixel(hip_lib, monkeypatch, cid):
    c, cfg = R.CASES[cid], R.case_cfg(cid)
    pairs = {name: R.stage_pair(cid, name) for name in R.stage_names(cid)}
    enc = _enc(c['cfg'])
    P = enc._ensure_packed(torch.device('cuda'))
    log = _spy(monkeypatch, enc)
    assert enc.steps() == oenc.stages(cfg) == list(pairs)
    skips = {q['c1']['cin']: 'centre' if 'kpad' in q['skip'] else 'gemm'
             for q in [q for d in P['down'] for q in d['blocks']] + [P['mid1'], P['mid2']] if 'skip' in q}
    assert skips == c['skips'], skips
    assert P['conv_in']['cin'] == (cfg['in_channels'] + 7) // 8 * 8
    failures = []
    for name, (x_in, y64, y16) in pairs.items():
        del log[:]
        y = _step(enc, name, x_in)
        assert log == (_stated_attention(cid) if name == 'mid_attn_1' else []), (name, log)
        _judge(f'{cid}/{name}', y, y16, y64, failures)
    assert not failures, failures


@pytest.mark.parametrize("cid", R.SINGLES)
def test_single_stage_every_pixel(hip_lib, monkeypatch, cid):
    c = R.CASES[cid]
    name = c['stage']
    ok = 'dh12' if c['raises'] else cid                     # the valid case run straight after the one that raises
    x_in, y64, y16 = R.stage_pair(ok, R.CASES[ok]['stage'])
    enc = _enc(c['cfg'])
    enc._ensure_packed(torch.device('cuda'))
    log = _spy(monkeypatch, enc)
    if c['raises']:
        assert R.CASES[ok]['cfg'] == c['cfg']
        with pytest.raises(ValueError, match=RAISES):
            _step(enc, name, R.case_input(cid))
        assert log == []                                    # raised in front of attn1's launch
    y = _step(enc, name, x_in)
    assert log == (_stated_attention(ok) if name == 'mid_attn_1' else []), (cid, log)
    failures = []
    _judge(ok, y, y16, y64, failures)
    assert not failures, failures


def test_stated_attention_kernels_are_the_plan_at_this_cu_count(hip_lib, tmp_path):
    """The launches the cases state, from csrc/kernel_plan.h at the CU count of the device the tests run on: the streaming / ring kernels
    the oracle restates, never the K-resident one (sequences * heads stays below the CU count)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    launches = R.enc_launches(cus)
    assert {r for _, r, _ in launches} == set(R.ROUTES)
    for (who, route, ln), (kernel, _) in zip(launches, R.plan([ln for _, _, ln in launches], tmp_path)):
        if route != 'small':
            assert ln[3] < cus, (who, ln)
            assert kernel != 'kres' and R.ROUTE_OF_KERNEL[kernel] == route, (who, ln, kernel, route)


@pytest.mark.parametrize("cid", R.WALKED)
def test_forward_is_exactly_the_steps_in_the_oracles_order(hip_lib, cid):
    """The HIP steps chained by hand, each fed the step before it, equal forward_frames bit for bit, and the `stages=` copies are the step
    outputs; forward(x) is ln3d_frame_mean of forward_frames, and its num_frames argument changes the pooling only.  The end-to-end rho
    against y16 is printed for the record, not gated (see tests/test_unet_pixels_cpu.py)."""
    from ln3diff_amd import ops
    c, cfg = R.CASES[cid], R.case_cfg(cid)
    enc = _enc(c['cfg'])
    x = R.case_input(cid).cuda()
    N, _, H, W = x.shape
    st = {}
    want = enc.forward_frames(x, stages=st).clone()
    assert list(st) == enc.steps()[:-1]
    h = x
    for name in enc.steps():
        h, H, W = enc._run_step(name, h, N, H, W)
        got = h.view(N, H, W, -1).permute(0, 3, 1, 2)
        assert torch.equal(got, want if name == 'conv_out' else st[name]), name       # compared before the next step adds onto h in place
    Fr = cfg['num_frames']
    hf = enc.forward_frames(x)                              # the NCHW view of channel-last memory forward() pools
    assert torch.equal(hf, want)
    pooled = enc(x)
    ref = torch.empty(N // Fr, *want.shape[1:], device='cuda')
    ops.frame_mean(hf, ref, N // Fr, Fr, want.shape[2] * want.shape[3], want.shape[1])
    assert pooled.shape == ref.shape and torch.equal(pooled, ref)
    mean = want.reshape(N // Fr, Fr, *want.shape[1:]).mean(1)
    assert float((pooled - mean).abs().max()) <= 1e-6 * float(mean.abs().max())
    if N == 12:                                             # one pool over both objects' frames: the attention still groups Fr
        p12 = enc(x, num_frames=12)
        ref12 = torch.empty(1, *want.shape[1:], device='cuda')
        ops.frame_mean(hf, ref12, 1, 12, want.shape[2] * want.shape[3], want.shape[1])
        assert torch.equal(p12, ref12) and torch.equal(enc.forward_frames(x), want)
    y16 = R.net_taps(cid)['conv_out'][1]
    y64 = R.run(cid, None, R.case_input(cid), rounded=False, whole=True)
    rho, _ = R.pixel_rho(want.cpu().double(), y16, y64)
    print(f'{cid}: end to end against y16 (not gated): median rho {float(rho.median()):.2f} worst {float(rho.max()):.2f}')


def test_one_frame_per_object_is_the_per_frame_transformer_bit_for_bit(hip_lib, monkeypatch):
    """Encoder(num_frames=1): attn1's sequences are the frames.  An encoder built for 6 frames with the same weights and its frame count
    forced to 1 gives the same bits, and both attentions of the block then take the same launch."""
    cid = 'f1-16x16'
    x_in = R.case_input(cid)
    sd1, sd6 = R.cfg_sd('f1'), R.cfg_sd('ch32')
    assert sd1.keys() == sd6.keys() and all(torch.equal(sd1[k], sd6[k]) for k in sd1)
    y1 = _step(_enc('f1'), 'mid_attn_1', x_in)
    e6 = _enc('ch32')
    e6._ensure_packed(torch.device('cuda'))
    log = _spy(monkeypatch, e6)
    monkeypatch.setattr(e6, 'num_frames', 1)
    y6 = _step(e6, 'mid_attn_1', x_in)
    assert torch.equal(y1, y6)
    assert log == [(64, 2, 256, True), (64, 2, 256, True)]
