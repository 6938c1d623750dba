"""The released multi-view VAE encoder on the GPU: its new kernels (pad-(0,1,0,1) im2col, fused posterior), the joint attention over
all frames of an object at the released token counts, parity of every stage against the reference goldens
(tests/golden/make_golden_encoder.py), and the AE / reconstruction paths end to end."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conftest import golden, load_synth, rel_l2

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16)


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("H,C", [(256, 64), (128, 128), (64, 256), (64, 8), (10, 16)])
def test_im2col_pad01_is_pad_then_unfold(hip_lib, H, C):
    """The encoder's Downsample gather against F.pad(x, (0, 1, 0, 1)) + unfold(3, stride 2): bit for bit (a gather), padding
    columns zero."""
    from ln3diff_amd import ops
    N, W = 2, H
    g = torch.Generator().manual_seed(H * 3 + C)
    x = _bf(torch.randn(N, H, W, C, generator=g)).cuda()
    Kpad = (9 * C + 63) // 64 * 64
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    col = torch.full((N * Ho * Wo, Kpad), 7.0, device='cuda', dtype=torch.bfloat16)
    ops.im2col3x3_pad01(x, col, N, H, W, C, Kpad)
    xp = Fn.pad(x.permute(0, 3, 1, 2).float(), (0, 1, 0, 1))
    u = Fn.unfold(xp, 3, stride=2)                                            # [N, C*9, L], rows (c, ky, kx)
    assert u.shape[-1] == Ho * Wo
    ref = u.view(N, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(N * Ho * Wo, 9 * C)
    assert torch.equal(col[:, :9 * C].float(), ref)
    assert not col[:, 9 * C:].float().any()


def _posterior_ref(h_frames, F, qw, qb, eps):
    """fp32 torch restatement of pool -> quant_conv -> [B, 8, 3, HW] view -> DiagonalGaussianDistribution(soft_clamp=True)."""
    N, Cm, H, W = h_frames.shape
    B = N // F
    hm = h_frames.reshape(B, F, Cm, H, W).sum(1) / F
    mo = Fn.conv2d(hm, qw.view(Cm, Cm // 3, 1, 1), qb, groups=3).reshape(B, Cm // 3, 3, H * W)
    mean, logvar = mo[:, :4], mo[:, 4:]
    pre = logvar
    logvar = torch.tanh(logvar / 20.0) * 20.0
    std, var = torch.exp(0.5 * logvar), torch.exp(logvar)
    z = mean if eps is None else mean + std * eps
    ns = (z - mean) / var
    log_q = -0.5 * ns * ns - 0.5 * math.log(2 * math.pi) - logvar
    ent = logvar + 0.5 * (math.log(2 * math.pi) + 1)
    return dict(mean=mean, logvar=logvar, z=z, log_q=log_q, entropy=ent, latent_tok=z.permute(0, 2, 3, 1).reshape(B, 3 * H * W, 4),
                pre=pre)


def test_posterior_kernel_against_torch(hip_lib):
    from ln3diff_amd import ops
    B, F, H, W, Cm = 2, 6, 32, 32, 24
    g = torch.Generator().manual_seed(5)
    h_cl = (torch.randn(B * F, H, W, Cm, generator=g) * 2.0).cuda()
    h = h_cl.permute(0, 3, 1, 2)                                              # NCHW view of channel-last memory (Encoder.forward_frames)
    qw = (torch.randn(Cm, 8, generator=g) * 0.5).cuda()
    qb = (torch.randn(Cm, generator=g) * 0.1)
    # logvar moments (output channels 12..23) of very different sizes: the soft clamp at |logvar| >> 20 and the plain range
    qb[12:18] += torch.tensor([80.0, -70.0, 45.0, -45.0, 0.0, 5.0])
    qb = qb.cuda()
    eps = torch.randn(B, 4, 3, H * W, generator=g).cuda()
    for e in (None, eps):
        got = ops.mv_posterior(h, qw, qb, e, B, F)
        ref = _posterior_ref(h.contiguous(), F, qw, qb, e)
        assert ref['pre'].abs().max() > 60 and ref['logvar'].abs().max() < 20
        for k in ('mean', 'logvar', 'z', 'entropy', 'latent_tok'):
            assert rel_l2(got[k], ref[k]) < 1e-5, (k, rel_l2(got[k], ref[k]))
        # log_q divides (z - mean) by var = exp(logvar): at logvar -20 one ulp of z is a visible fraction of z - mean
        assert rel_l2(got['log_q'], ref['log_q']) < 1e-3, rel_l2(got['log_q'], ref['log_q'])
    mode = ops.mv_posterior(h, qw, qb, None, B, F)
    assert torch.equal(mode['z'], mode['mean'])
    # the pooled NCHW route (ln3d_frame_mean, then F = 1) gives the same bits as pooling inside the posterior
    pooled = torch.empty(B, Cm, H, W, device='cuda')
    ops.frame_mean(h, pooled, B, F, H * W, Cm)
    assert rel_l2(pooled, h.contiguous().reshape(B, F, Cm, H, W).mean(1)) < 1e-6
    p1 = ops.mv_posterior(pooled, qw, qb, eps, B, 1)
    pf = ops.mv_posterior(h, qw, qb, eps, B, F)
    for k in pf:
        assert torch.equal(p1[k], pf[k]), k


@pytest.mark.parametrize("F,B", [(6, 2), (40, 1)])
def test_joint_attention_at_released_token_counts(hip_lib, F, B):
    """attn1 of SpatialTransformer3D attends over all F * 1024 tokens of an object (6 144 at the released 6 views, 40 960 at 40) with
    8 heads of 64: ln3d_attention_bf16 takes it as it is (Nk a multiple of 256 -> the streaming kernel).  Against fp32 torch on the
    same bf16 operands, on a subset of the queries (every query block is represented)."""
    from ln3diff_amd import ops
    Hh, Dh, N = 8, 64, F * 1024
    g = torch.Generator().manual_seed(F)
    q = _bf(torch.randn(B, Hh, N, Dh, generator=g)).cuda()
    k = _bf(torch.randn(B, Hh, N, Dh, generator=g)).cuda()
    v = _bf(torch.randn(B, Hh, N, Dh, generator=g) + torch.arange(Dh) / Dh).cuda()
    k[:, :, N - 5] = q[:, :, 3] * 4.0                                         # a late spiked key: the online-softmax rebase
    vt = v.transpose(-1, -2)[..., ops.vt_key_order(N, 'cuda')].contiguous()
    out = torch.full((B, N, Hh * Dh), float('nan'), device='cuda', dtype=torch.bfloat16)
    ops.attention(q, k, vt, out, B, Hh, N, N, N, N, Dh)
    assert torch.isfinite(out.float()).all()
    sel = torch.cat([torch.arange(0, N, 97, device='cuda'), torch.tensor([3, N - 1], device='cuda')])
    s = torch.einsum('bhqd,bhkd->bhqk', q[:, :, sel].float(), k.float()) / 8.0
    ref = torch.einsum('bhqk,bhkd->bhqd', torch.softmax(s, -1), v.float()).permute(0, 2, 1, 3).reshape(B, len(sel), Hh * Dh)
    e = rel_l2(out[:, sel].float(), ref)
    print(f'joint attention F={F} ({N} tokens): rel-L2 {e:.2e}')
    assert e < 1e-2, e


# ----------------------------------------------------------------------------- modules
def _encoder():
    from ln3diff_amd.vit.mv_encoder import create_encoder
    enc = create_encoder()
    load_synth(enc, 0)
    return enc.cuda()


def _decoder():
    from test_fullsize_gpu import _tiny_decoder
    return _tiny_decoder()[1]


def _input(name, shape, seed):
    from ln3diff_amd.synth import synth_input
    return synth_input(name, shape, seed).cuda()


def test_frame_coupling_and_object_independence(hip_lib):
    """Changing frame 0 of object 0 changes frame 5's joint attention output (attn1 sees all frames) but not frame 5's convolution
    stages before it, and leaves object 1 bit for bit alone."""
    enc = _encoder()
    x = _input('mv_b2', (12, 10, 64, 64), 8)
    x2 = x.clone()
    x2[0] += 0.5
    s1, s2 = {}, {}
    h1 = enc.forward_frames(x, stages=s1).clone()
    h2 = enc.forward_frames(x2, stages=s2).clone()
    assert torch.equal(s1['mid_block_1'][5], s2['mid_block_1'][5])
    assert not torch.equal(s1['mid_attn_1'][5], s2['mid_attn_1'][5])
    for k in s1:
        assert torch.equal(s1[k][6:], s2[k][6:]), k
    assert torch.equal(h1[6:], h2[6:]) and not torch.equal(h1[5], h2[5])


def test_small_case_every_stage_vs_reference_golden(hip_lib):
    import json
    g = golden('encoder_mv_small')
    steps = {k: tuple(v) for k, v in json.loads(bytes(g['stage_steps']).decode()).items()}
    enc, dec = _encoder(), _decoder()
    x = _input('mv_small', (6, 10, 64, 64), 7)
    st = {}
    hf = enc.forward_frames(x, stages=st)
    errs = {}
    for k, (c, s) in steps.items():
        errs[k] = rel_l2(st[k][:, ::c, ::s, ::s].cpu(), torch.from_numpy(g['stage_' + k]).float())
    errs['conv_out'] = rel_l2(hf.cpu(), g['conv_out'])
    h = enc(x)
    errs['h'] = rel_l2(h.cpu(), g['h'])
    r = dec.vae_reparameterization(h, False)
    errs['mode_latent'] = rel_l2(r['latent_normalized_2Ddiffusion'].cpu(), g['mode_latent'])
    torch.manual_seed(int(g['sample_seed']))
    rs = dec.vae_reparameterization(hf, True, num_frames=6)
    errs['sample_latent'] = rel_l2(rs['latent_normalized_2Ddiffusion'].cpu(), g['sample_latent'])
    errs['sample_tokens'] = rel_l2(rs['latent_normalized'].cpu(), g['sample_tokens'])
    errs['sample_log_q'] = rel_l2(rs['log_q'].cpu(), g['sample_log_q'])
    errs['sample_entropy'] = rel_l2(rs['normal_entropy'].cpu(), g['sample_entropy'])
    print('small-case rel-L2:', {k: f'{v:.2e}' for k, v in errs.items()})
    # measured on MI355X: the bf16 conv chain grows 2.3e-3 (conv_in) -> 1.0e-2 (conv_out); pooled h 6.8e-3, latents <= 5.8e-3
    for k, e in errs.items():
        assert e < (1.5e-2 if k in steps or k == 'conv_out' else 1e-2), (k, e)


def test_two_objects_vs_reference_golden(hip_lib):
    g = golden('encoder_mv_b2')
    enc, dec = _encoder(), _decoder()
    h = enc(_input('mv_b2', (12, 10, 64, 64), 8))
    assert h.shape == (2, 24, 8, 8)
    e_h = rel_l2(h.cpu(), g['h'])
    e_z = rel_l2(dec.vae_reparameterization(h, False)['latent_normalized_2Ddiffusion'].cpu(), g['mode_latent'])
    e_obj = [rel_l2(h[b].cpu(), g['h'][b]) for b in range(2)]
    print(f'B=2 x F=6: h {e_h:.2e} (per object {e_obj[0]:.2e} / {e_obj[1]:.2e}), latent {e_z:.2e}')
    assert e_h < 1e-2 and e_z < 1e-2 and max(e_obj) < 1e-2


def test_released_size_vs_reference_golden(hip_lib):
    """B = 1, F = 6 at 256 x 256 (6 144 jointly attended tokens): pooled h, the posterior mean, and encoder_vae with the reference's
    seeded CPU-generator sample."""
    from ln3diff_amd.nsr.script_util import AE
    from ln3diff_amd.vit.mv_encoder import RELEASED_DINO_VERSION
    g = golden('encoder_mv_released')
    enc, dec = _encoder(), _decoder()
    x = _input('mv_released', (6, 10, 256, 256), 9)
    ae = AE(enc, dec, 32, dino_version=RELEASED_DINO_VERSION)
    h = ae(img=x, behaviour='enc')
    e_h = rel_l2(h.cpu(), g['h'])
    r = dec.vae_reparameterization(h, False)
    e_mean = rel_l2(r['latent_normalized_2Ddiffusion'].cpu(), g['mode_latent'])
    e_tok = rel_l2(r['latent_normalized'].cpu(), torch.from_numpy(g['mode_tokens']).float())
    e_lq = rel_l2(r['log_q'].cpu(), torch.from_numpy(g['mode_log_q']).float())
    torch.manual_seed(int(g['sample_seed']))
    rs = ae(img=x, behaviour='encoder_vae')
    e_s = rel_l2(rs['latent_normalized_2Ddiffusion'].cpu(), g['sample_latent'])
    e_slq = rel_l2(rs['log_q'].cpu(), torch.from_numpy(g['sample_log_q']).float())
    print(f'released size rel-L2: h {e_h:.2e} mean {e_mean:.2e} tokens {e_tok:.2e} log_q {e_lq:.2e} sample {e_s:.2e} sample log_q {e_slq:.2e}')
    assert rs['latent_normalized_2Ddiffusion'].shape == (1, 12, 32, 32) and rs['latent_normalized'].shape == (1, 3072, 4)
    # measured on MI355X: h 6.9e-3, mean 5.8e-3, log_q 1.4e-3, sampled latent 1.2e-3 (the unit-variance noise dominates it)
    for e in (e_h, e_mean, e_tok, e_lq, e_s, e_slq):
        assert e < 1e-2, e


def _two_route_difference(d_head):
    """An encoder with 8 heads of d_head on 2 objects x 5 frames at 64 x 64: 8 x 8 middle tokens per frame, so attn1 attends 320 joint
    tokens (the MFMA attention kernels) and attn2 64 (ln3d_attention_small).  -> rel-L2 between that forward and the same forward with
    the threshold raised so that attn1 runs on ln3d_attention_small too."""
    from ln3diff_amd import convstack
    from ln3diff_amd.vit.mv_encoder import MVEncoderGSDynamicInp
    enc = MVEncoderGSDynamicInp(double_z=True, resolution=64, in_channels=10, ch=32, ch_mult=[1, 2, 4, 4], num_res_blocks=1, num_frames=5,
                                dropout=0.0, attn_resolutions=[], out_ch=3, z_channels=12, attn_kwargs={'n_heads': 8, 'd_head': d_head})
    load_synth(enc, 0)
    enc = enc.cuda()
    x = _input('mv_heads', (10, 10, 64, 64), 12)
    y_mfma = enc.forward_frames(x).clone()
    saved = convstack.MFMA_MIN_TOKENS
    convstack.MFMA_MIN_TOKENS = 1 << 30
    try:
        y_small = enc.forward_frames(x).clone()
    finally:
        convstack.MFMA_MIN_TOKENS = saved
    assert torch.isfinite(y_mfma).all() and not torch.equal(y_mfma, y_small)        # two routes did run
    return rel_l2(y_mfma, y_small)


def test_head_size_48_takes_the_padded_output_projection(hip_lib):
    """d_head = 48 runs on the MFMA route in 64-wide zero-padded heads, so attn1's output has 8 x 64 columns and meets the zero-padded
    copy of to_out; the unpadded 384-column weight would raise on the GEMM's K mismatch.  (ch = 32 also makes down.1's nin_shortcut a
    1x1 with 32 input channels, below the GEMM's K step: it runs as the centre tap of a 3x3.)  The two routes must agree as closely as
    they do at the released d_head = 64, which needs no padded copy: _two_route_difference(64) measured 2.770e-3 on an MI355X (2.725e-3
    with weight seed 1; d_head = 48 itself: 2.636e-3).  The gate is twice the d_head = 64 figure, one factor of two for the different
    weights the seeded filler gives another width."""
    e = _two_route_difference(48)
    print(f'd_head 48: MFMA route vs attention_small route rel-L2 {e:.3e}')
    assert e < 2 * 2.770e-3, e                 # 2 x the measured d_head = 64 figure


# ----------------------------------------------------------------------------- end to end
def _ae():
    from ln3diff_amd.nsr.script_util import AE
    from ln3diff_amd.vit.mv_encoder import RELEASED_DINO_VERSION
    return AE(_encoder(), _decoder(), 32, dino_version=RELEASED_DINO_VERSION)


def test_enc_dec_equals_encoder_vae_then_decode(hip_lib):
    from ln3diff_amd.synth import orbit_cameras
    ae = _ae()
    x = _input('mv_released', (6, 10, 256, 256), 9)
    eps = torch.randn(1, 4, 3, 1024, generator=torch.Generator().manual_seed(3))
    cams = orbit_cameras(2).cuda()
    gen = torch.Generator(device='cuda').manual_seed(1)
    j, u = torch.rand(2, 32 * 32, 64, device='cuda', generator=gen), torch.rand(2 * 32 * 32, 64, device='cuda', generator=gen)
    a = ae(img=x, c=cams, behaviour='enc_dec', eps=eps, jitter=j, u_fine=u)
    lat = ae(img=x, behaviour='encoder_vae', eps=eps)
    b = ae(c=cams, latent=lat, behaviour='decode_after_vae', jitter=j, u_fine=u)
    assert torch.equal(a['image_raw'], b['image_raw']) and torch.equal(a['latent_after_vit'], b['latent_after_vit'])
    assert torch.isfinite(a['image_raw']).all() and a['image_raw'].shape == (2, 3, 32, 32)
    # enc -> dec: the pooled route gives the same latent (the frame mean is the same arithmetic in both kernels)
    w = ae(img=x, behaviour='enc_dec_wo_triplane', eps=eps)
    d = ae(latent=ae(img=x, behaviour='enc'), behaviour='dec_wo_triplane', eps=eps)
    assert torch.equal(w['latent_normalized_2Ddiffusion'], lat['latent_normalized_2Ddiffusion'])
    assert torch.equal(d['latent_normalized_2Ddiffusion'], lat['latent_normalized_2Ddiffusion'])
    assert torch.equal(d['latent_after_vit'], b['latent_after_vit'])


def test_reconstruct_writes_latents_and_frames(hip_lib, tmp_path):
    from ln3diff_amd.pipeline import reconstruct
    from ln3diff_amd.synth import orbit_cameras
    ae = _ae()
    x = _input('mv_released', (6, 10, 256, 256), 9)
    cams = orbit_cameras(3).cuda()
    outs = []
    for run in range(2):
        torch.manual_seed(0)
        outs.append(reconstruct(ae, x, cams, latent_dir=str(tmp_path / f'run{run}'), ins_names=['obj']))
    z = np.load(tmp_path / 'run0' / 'obj' / 'latent.npy')
    assert z.shape == (12, 32, 32)
    assert np.array_equal(z, outs[0]['latent']['latent_normalized_2Ddiffusion'][0].cpu().numpy())
    assert np.array_equal(z, np.load(tmp_path / 'run1' / 'obj' / 'latent.npy'))
    a, b = outs
    assert a['image_raw'].shape == (1, 3, 3, 32, 32) and torch.isfinite(a['image_raw']).all()
    for k in ('image_raw', 'image_depth'):
        assert torch.equal(a[k], b[k]), k
    assert os.path.isdir(tmp_path / 'run1' / 'obj')
