"""The ShapeNet VAE decoder class on the GPU: its new kernels against fp32 torch, parity of every stage with the reference class
(tests/golden/make_golden_shapenet_decoder.py) at a reduced width and at the released size, object independence, repeatability and
the ShapeNet launcher flags end to end."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conftest import golden, rel_l2

pytestmark = pytest.mark.gpu

CFG = 'shapenet_tuneray_aug_resolution_64_64_nearestSR'
# rel-L2 gates, about 1.5x the measured values (MI355X; reduced / released size): ldm_upsample 2.1e-4 (the goldens hold fp16),
# ViT out 2.7e-3, decoder_pred 3.6e-3, planes 4.1e-3, rendered RGB 2.4e-4, depth 1.4e-5, 64^3 grid sigma 2.5e-4 / rgb 2.9e-4
GATES = dict(ldm_upsample=3.5e-4, vit=4.5e-3, decoder_pred=5.5e-3, planes=6.5e-3, image_raw=4e-4, image_depth=3e-5, grid_sigma=4e-4,
             grid_rgb=4.5e-4)


def _dec(D, heads):
    from ln3diff_amd.nsr.triplane import Triplane
    from ln3diff_amd.synth import synth_vit_state_dict
    from ln3diff_amd.vit.vit_triplane_shapenet import RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn, DinoVisionTransformer, \
        shapenet_rendering_kwargs
    tp = Triplane(img_resolution=128, rendering_kwargs=shapenet_rendering_kwargs(CFG, 0.6, 1.8), decoder_output_dim=32)
    dec = RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn(DinoVisionTransformer(D, 12, heads), tp, False)
    sd = synth_vit_state_dict({k: tuple(v.shape) for k, v in dec.state_dict().items()}, 0)      # as the generator
    sd['triplane_decoder.decoder.net.2.bias'] = sd['triplane_decoder.decoder.net.2.bias'].clone()
    sd['triplane_decoder.decoder.net.2.bias'][0] += 4.0
    dec.load_state_dict(sd, strict=True)
    return dec.cuda()


def _latent(name, shape, seed):
    from ln3diff_amd.synth import synth_input
    return synth_input(name, shape, seed).cuda()


def _decode(dec, latent, stages=None):
    st = {}
    if stages is not None:
        orig = dec.forward_vit_decoder

        def fwd(x, img_size=None):
            st['ldm_upsample'] = x.clone()
            return orig(x, img_size)
        dec.forward_vit_decoder = fwd
    vit = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': latent}, 128)
    if stages is not None:
        del dec.forward_vit_decoder
    ret = dec.vit_decode_postprocess(vit, {}, return_stages=True)
    st['vit'] = vit
    return st, ret


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,p,H", [(1, 16, 12), (2, 16, 2), (1, 5, 1), (3, 32, 3)])
def test_axis_attention_against_torch(hip_lib, B, p, H):
    from ln3diff_amd import ops
    D, N = H * 64, p * p
    g = torch.Generator().manual_seed(B * 100 + p)
    qkv = torch.randn(B * 3 * N, 3 * D + 8, generator=g).cuda()[:, :3 * D + 8]
    out = torch.empty(B * 3 * N, D, device='cuda', dtype=torch.bfloat16)
    ops.triplane_axis_attention(qkv, out, B, p, H)
    x = qkv[:, :3 * D].view(B, 3, p, p, 3, H, 64)
    q, k, v = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]                     # [B, 3, p, p, H, 64]
    ref = torch.empty(B, 3, p, p, H, 64, device='cuda')
    for i in range(3):
        kr, vr = k[:, (i + 1) % 3], v[:, (i + 1) % 3]                                 # row y of plane i+1: [B, y, j, H, 64]
        kc, vc = k[:, (i + 2) % 3].transpose(1, 2), v[:, (i + 2) % 3].transpose(1, 2)  # column x of plane i+2: [B, x, j, H, 64]
        kk = torch.cat([kr[:, :, None].expand(B, p, p, p, H, 64), kc[:, None].expand(B, p, p, p, H, 64)], 3)   # [B, y, x, 2p, H, 64]
        vv = torch.cat([vr[:, :, None].expand(B, p, p, p, H, 64), vc[:, None].expand(B, p, p, p, H, 64)], 3)
        s = torch.einsum('byxhd,byxjhd->byxhj', q[:, i], kk) / 8.0
        ref[:, i] = torch.einsum('byxhj,byxjhd->byxhd', s.softmax(-1), vv)
    assert rel_l2(out.float(), ref.reshape(B * 3 * N, D)) < 4e-3


@pytest.mark.parametrize("B,S,P,C", [(1, 16, 4, 128), (2, 3, 2, 12)])
def test_sr_unpatchify_against_torch(hip_lib, B, S, P, C):
    from ln3diff_amd import ops
    R = S * P
    pred = torch.randn(B, 3 * S * S, P * P * C, device='cuda')
    planes = torch.empty(B, 3, R, R, C, device='cuda')
    mixed = torch.empty(B, 3, R, R, C, device='cuda', dtype=torch.bfloat16)
    ops.sr_unpatchify(pred, planes, mixed, B, S, P, C)
    ref = torch.einsum('ndhwpqc->ndchpwq', pred.view(B, 3, S, S, P, P, C)).reshape(B, 3 * C, R, R)     # unpatchify_triplane
    assert torch.equal(planes, ref.view(B, 3, C, R, R).permute(0, 1, 3, 4, 2))
    mref = ref.reshape(B, C, 3, R * R).permute(0, 2, 3, 1).reshape(B, 3, R, R, C)                        # short_cut's view
    assert torch.equal(mixed, mref.to(torch.bfloat16))


@pytest.mark.parametrize("h,Ho,C,tr", [(64, 256, 128, True), (64, 256, 32, False), (7, 29, 4, True), (10, 10, 8, False)])
def test_resize_kernels_against_interpolate(hip_lib, h, Ho, C, tr):
    from ln3diff_amd import ops
    N = 3
    x = torch.randn(N, h, h, C, device='cuda')
    y = torch.empty(N, Ho, Ho, C, device='cuda', dtype=torch.bfloat16)
    ops.resize_bilinear_cl(x, y, N, h, h, Ho, Ho, C, transpose=tr)
    xin = x.permute(0, 3, 1, 2)
    if tr:
        xin = xin.transpose(2, 3)
    ref = Fn.interpolate(xin, size=(Ho, Ho), mode='bilinear', align_corners=False, antialias=True).permute(0, 2, 3, 1)
    assert rel_l2(y.float(), ref) < 4e-3
    t = torch.randn(N, Ho, Ho, C, device='cuda')
    out = torch.empty_like(t)
    ops.resize_add_lrelu(x, t, out, N, h, h, Ho, Ho, C, 0.01)
    ref2 = Fn.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Ho), mode='bilinear', align_corners=False, antialias=True).permute(0, 2, 3, 1) \
        + Fn.leaky_relu(t, 0.01)
    assert rel_l2(out, ref2) < 1e-5


@pytest.mark.parametrize("H,W,C", [(256, 256, 32), (9, 13, 4)])
def test_rollout_means_and_im2col_against_torch(hip_lib, H, W, C):
    from ln3diff_amd import ops
    x = torch.randn(3, H, W, C, device='cuda')
    rowm, colm = torch.empty(3, H, C, device='cuda'), torch.empty(3, W, C, device='cuda')
    ops.rollout_means(x, rowm, colm, 3, H, W, C)
    assert rel_l2(rowm, x.mean(2)) < 1e-6 and rel_l2(colm, x.mean(1)) < 1e-6
    Kpad = (27 * C + 63) // 64 * 64
    col = torch.full((H * W, Kpad), 5.0, device='cuda', dtype=torch.bfloat16)
    for i in range(3):
        ops.im2col3x3_rollout(x, rowm, colm, col, i, H, W, C, Kpad)
        roll = torch.cat([x[i], rowm[(i + 1) % 3][:, None].expand(H, W, C), colm[(i + 2) % 3][None].expand(H, W, C)], -1)   # [H, W, 3C]
        u = Fn.unfold(roll.permute(2, 0, 1)[None], 3, padding=1)[0]                           # [(3C, ky, kx), HW]
        ref = u.view(3 * C, 9, H * W).permute(2, 1, 0).reshape(H * W, 27 * C)
        assert torch.equal(col[:, :27 * C], ref.to(torch.bfloat16))
        assert not col[:, 27 * C:].float().any()


# ----------------------------------------------------------------------------- parity with the reference class
def test_reduced_width_every_stage(hip_lib):
    g = golden('shapenet_dec_small')
    dec = _dec(128, 2)
    st, ret = _decode(dec, _latent('shapenet_latent', (1, 12, 32, 32), 11), stages=True)
    errs = {'ldm_upsample': rel_l2(st['ldm_upsample'][:, ::2], torch.from_numpy(g['ldm_upsample']).float()),
            'vit': rel_l2(st['vit'][:, ::2], torch.from_numpy(g['vit']).float()),
            'decoder_pred': rel_l2(ret['decoder_pred'][:, ::4, ::8], torch.from_numpy(g['decoder_pred']).float()),
            'planes': rel_l2(ret['latent_after_vit'][:, :, ::8, ::8], torch.from_numpy(g['planes']).float())}
    print('shapenet reduced', errs)
    for k, gate in GATES.items():
        if k in errs:
            assert errs[k] < gate, errs


def test_b2_objects_decode_independently(hip_lib):
    g = golden('shapenet_dec_b2')
    dec = _dec(128, 2)
    lat = _latent('shapenet_latent_b2', (2, 12, 32, 32), 12)
    st, ret = _decode(dec, lat)
    e_vit = rel_l2(st['vit'][:, ::4], torch.from_numpy(g['vit']).float())
    e_pl = rel_l2(ret['latent_after_vit'][:, ::2, ::8, ::8], torch.from_numpy(g['planes']).float())
    print('shapenet b2', e_vit, e_pl)
    assert e_vit < GATES['vit'] and e_pl < GATES['planes']
    _, r1 = _decode(dec, lat[1:2].contiguous())
    assert torch.equal(r1['planes_channel_last'][0], ret['planes_channel_last'][1])


def test_released_size_parity_render_and_grid(hip_lib):
    g = golden('shapenet_dec_released')
    dec = _dec(768, 12)
    st, ret = _decode(dec, _latent('shapenet_latent_rel', (1, 12, 32, 32), 13), stages=True)
    errs = {'ldm_upsample': rel_l2(st['ldm_upsample'][:, ::6, ::2], torch.from_numpy(g['ldm_upsample']).float()),
            'vit': rel_l2(st['vit'][:, ::6, ::2], torch.from_numpy(g['vit']).float()),
            'decoder_pred': rel_l2(ret['decoder_pred'][:, ::6, ::16], torch.from_numpy(g['decoder_pred']).float()),
            'planes': rel_l2(ret['latent_after_vit'][:, :, ::8, ::8], torch.from_numpy(g['planes']).float())}
    cams = torch.from_numpy(g['cams']).cuda()
    res, rk = 128, dec.rendering_kwargs
    torch.manual_seed(int(g['render_seed']))
    jitter = torch.rand(1, res * res, rk['depth_resolution'], 1)
    u_fine = torch.rand(res * res, rk['depth_resolution_importance'])
    r = dec.triplane_decode(ret, cams, jitter=jitter, u_fine=u_fine)
    errs['image_raw'] = rel_l2(r['image_raw'], torch.from_numpy(g['image_raw']).float())
    errs['image_depth'] = rel_l2(r['image_depth'], torch.from_numpy(g['image_depth']).float())
    grid = dec.triplane_decode_grid(ret, 64)
    errs['grid_sigma'] = rel_l2(grid['sigma'][:, ::2, ::2, ::2], torch.from_numpy(g['grid_sigma']).float())
    errs['grid_rgb'] = rel_l2(grid['rgb'][:, ::4, ::4, ::4], torch.from_numpy(g['grid_rgb'][..., :3]).float())   # 32-wide decoder: rgb = first 3
    print('shapenet released', json.dumps(errs))
    for k, gate in GATES.items():
        assert errs[k] < gate, errs


def test_decode_is_bitwise_repeatable(hip_lib):
    dec = _dec(768, 12)
    lat = _latent('shapenet_latent_rel', (1, 12, 32, 32), 13)
    a = _decode(dec, lat)[1]['planes_channel_last'].clone()
    b = _decode(dec, lat)[1]['planes_channel_last']
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- end to end
def test_car_launcher_flags_end_to_end(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    small = ("--num_samples 1 --image_size 32 --num_views 2 --create_dit false --trainer_name vpsde_crossattn --num_channels 128 "
             "--num_res_blocks 1 --num_heads 4 --channel_mult 1,2 --attention_resolutions 32,16 --denoise_in_channels 12 "
             "--denoise_out_channels 12 --roll_out false --predict_v true --pred_type v --mixed_prediction true --use_ddim true "
             "--timestep_respacing ddim3 --decoder_in_chans 32 --out_chans 96 --decoder_output_dim 32 --arch_decoder vitb --vae_p 2 "
             "--cfg shapenet_tuneray_aug_resolution_64_64_nearestSR --ray_start 0.6 --ray_end 1.8")
    cls = " --ae_classname vit.vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn"
    args = create_argparser(False).parse_known_args((small + cls + f" --logdir {tmp_path}/s").split())[0]
    lat = run(args)
    frames = np.load(tmp_path / "s" / "frames_rank0.npy")
    assert lat.shape == (1, 12, 32, 32) and frames.shape == (2, 3, 32, 32) and np.isfinite(frames).all()
    assert (tmp_path / "s" / "sample0_view0.ppm").exists()
    # the same flags without the class: today's path (the Objaverse decoder class), unchanged
    args = create_argparser(False).parse_known_args((small + f" --logdir {tmp_path}/o").split())[0]
    lat_o = run(args)
    assert torch.equal(lat_o, lat)
    fo = np.load(tmp_path / "o" / "frames_rank0.npy")
    assert fo.shape == frames.shape and not np.array_equal(fo, frames)
