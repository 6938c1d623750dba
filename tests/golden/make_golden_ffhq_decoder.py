#!/usr/bin/env python
"""Golden vectors of the FFHQ VAE decoder class (vit/vit_triplane.py
VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final, the
`--ae_classname` of sample_ffhq_t23d.sh), run from the reference checkout through ref_shims in the build container.

    python tests/golden/make_golden_ffhq_decoder.py

The launcher's `vit_decoder` is torch.hub facebookresearch/dinov2 `dinov2_vitb14`, which is not installed: the `_RefDino` stand-in of
make_golden_shapenet_decoder.py is used, and the reference class is built around it unchanged.  Weights come from
ln3diff_amd.synth.synth_vit_state_dict by state-dict name (seed 0; sigma bias + 4): every tensor the reference initialises to zero
(pos_embed, the skip_linear projections) is random there, so that parity is not vacuous (asserted below).  Inputs from seeded CPU
generators.  Outputs only (fp16 and sub-sampled where large; the slices are in main()):
  ffhq_dec_small.npz       D = 128 (2 heads), B = 1: ldm_upsample, each fusion block, ViT out, decoder_pred, x0, planes
  ffhq_dec_released.npz    D = 768, B = 1: ldm_upsample, ViT out, decoder_pred, x0, latent_after_vit (sub-sampled), the ffhq preset's
                           renders at 64 x 64 and 128 x 128 (one view, seeded ray noise) and a 16^3 grid query
  render_preset_ffhq48.npz the ffhq preset (48 + 48 samples, ray limits 2.25 / 3.3, box_warp 1) on synthetic planes through the
                           reference's Triplane alone: image_raw / image_depth / weights_samples at 64 x 64
  ffhq_rendering_kwargs.json   rendering_options_defaults(opts) for --cfg ffhq
Every decoder .npz carries the state-dict manifest; it is asserted equal to the package class's.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden_shapenet_decoder as sn  # noqa: E402  (installs ref_shims; _RefDino, save, manifest_json)

from ln3diff_amd.synth import synth_vit_state_dict, synth_input, orbit_cameras  # noqa: E402

torch.set_grad_enabled(False)
CAM_RADIUS = 2.7
LAUNCHER_FLAGS = dict(cfg='ffhq')
CLASS = 'VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final'


def ref_rendering_kwargs():
    from nsr import script_util as su
    d = {}
    d.update(su.encoder_and_nsr_defaults())
    d.update(su.loss_defaults())
    d.update(LAUNCHER_FLAGS)
    return su.rendering_options_defaults(types.SimpleNamespace(**d))


def ref_triplane():
    from nsr.triplane import Triplane
    with contextlib.redirect_stdout(io.StringIO()):
        tp = Triplane(25, 128, 3, rendering_kwargs=ref_rendering_kwargs(), out_chans=96, triplane_size=224, decoder_in_chans=32,
                      decoder_output_dim=32, sr_kwargs={}, bcg_synthesis_kwargs={}, lrm_decoder=False)
    assert tp.superresolution is None                         # --sr_training False
    return tp


def build_ref(D, heads):
    from vit import vit_triplane as vt
    with contextlib.redirect_stdout(io.StringIO()):
        dec = getattr(vt, CLASS)(sn._RefDino(D, heads), ref_triplane(), False, vae_p=1, ldm_z_channels=4, ldm_embed_dim=4)
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    sd = synth_vit_state_dict(shapes, 0)          # pos_embed 0.02 N, LayerScale gammas 1 + 0.1 N
    sd['triplane_decoder.decoder.net.2.bias'] = sd['triplane_decoder.decoder.net.2.bias'].clone()
    sd['triplane_decoder.decoder.net.2.bias'][0] += 4.0
    for k, v in sd.items():
        if k.endswith('pos_embed') or 'skip_linear' in k:
            assert v.float().abs().max() > 0, k + ' is zero: parity through it would be vacuous'
    dec.load_state_dict(sd, strict=True)
    return dec.eval(), shapes


def pkg_manifest(D, heads):
    from ln3diff_amd.vit import vit_triplane_ffhq as ff
    from ln3diff_amd.nsr.triplane import Triplane
    tp = Triplane(img_resolution=128, rendering_kwargs=ff.ffhq_rendering_kwargs('ffhq'), decoder_output_dim=32)
    dec = getattr(ff, CLASS)(ff.DinoVisionTransformer(D, 12, heads), tp, False)
    return {k: tuple(v.shape) for k, v in dec.state_dict().items()}


def staged(dec, latent):
    """vit_decode_backbone + vit_decode_postprocess of the reference with the stage outputs recorded by forward hooks."""
    st = {}
    cs = dec.superresolution['conv_sr']
    hooks = [dec.superresolution['ldm_upsample'].register_forward_hook(lambda m, i, o: st.__setitem__('ldm_upsample', o.clone())),
             dec.decoder_pred.register_forward_hook(lambda m, i, o: st.__setitem__('decoder_pred', o.clone())),
             cs.conv3D_1.register_forward_hook(lambda m, i, o: st.__setitem__('x0', i[0].clone()))]
    for j, blk in enumerate(dec.vit_decoder.blocks):
        hooks.append(blk.register_forward_hook(lambda m, i, o, j=j: st.__setitem__(f'blk{j}', o.clone())))
    with contextlib.redirect_stdout(io.StringIO()):
        vit = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': latent}, 128)
        ret = dec.vit_decode_postprocess(vit, {})
    for h in hooks:
        h.remove()
    st['vit'] = vit
    return st, ret


def render(dec_or_tp, planes, cams, res, seed):
    tp = getattr(dec_or_tp, 'triplane_decoder', dec_or_tp)
    tp.neural_rendering_resolution = res
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return tp(planes, cams, neural_rendering_resolution=res, return_raw_only=True)


def main():
    rk = ref_rendering_kwargs()
    with open(os.path.join(HERE, 'ffhq_rendering_kwargs.json'), 'w') as f:
        json.dump({'flags': LAUNCHER_FLAGS, 'rendering_kwargs': rk}, f, indent=1, sort_keys=True)

    # reduced width, B = 1, every stage
    dec, shapes = build_ref(128, 2)
    assert shapes == pkg_manifest(128, 2), "state-dict manifest differs from the package class (D = 128)"
    latent = synth_input('ffhq_latent', (1, 12, 16, 16), 21)
    st, ret = staged(dec, latent)
    arrs = {f'stage_{k}': v.reshape(1, 768, -1)[:, ::4].half() for k, v in st.items() if k.startswith('blk')}
    sn.save('ffhq_dec_small', ldm_upsample=st['ldm_upsample'][:, ::2].half(), vit=st['vit'][:, ::2].half(),
            decoder_pred=st['decoder_pred'][:, ::4, ::8].half(), x0=st['x0'][:, :, ::8, ::8].half(),
            planes=ret['latent_after_vit'][:, :, ::8, ::8].half(), manifest=sn.manifest_json(shapes), **arrs)

    # released size
    dec, shapes = build_ref(768, 12)
    assert shapes == pkg_manifest(768, 12), "state-dict manifest differs from the package class (D = 768)"
    nparam = sum(int(np.prod(s)) for s in shapes.values())
    print(f'== FFHQ decoder: {len(shapes)} tensors, {nparam} parameters')
    latent = synth_input('ffhq_latent_rel', (1, 12, 16, 16), 23)
    st, ret = staged(dec, latent)
    cams = orbit_cameras(8, radius=CAM_RADIUS)[[2]]
    r64 = render(dec, ret['latent_after_vit'], cams, 64, 0)
    r128 = render(dec, ret['latent_after_vit'], cams, 128, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        grid = dec.triplane_decode_grid(ret, 16)
    sn.save('ffhq_dec_released', ldm_upsample=st['ldm_upsample'][:, ::6, ::2].half(), vit=st['vit'][:, ::6, ::2].half(),
            decoder_pred=st['decoder_pred'][:, ::6, ::16].half(), x0=st['x0'][:, :, ::8, ::8].half(),
            planes=ret['latent_after_vit'][:, :, ::8, ::8].half(),
            image_raw64=r64['image_raw'].half(), image_depth64=r64['image_depth'], image_raw128=r128['image_raw'].half(),
            image_depth128=r128['image_depth'], cams=cams, cam_radius=np.array(CAM_RADIUS), render_seed=np.array(0),
            grid_sigma=grid['sigma'].half(), grid_rgb=grid['rgb'].half(), manifest=sn.manifest_json(shapes), n_params=np.array(nparam))

    # the renderer preset alone, on synthetic planes (fp16: the planes are the test's input as stored)
    tp = dec.triplane_decoder
    planes = synth_input('ffhq_preset_planes', (1, 96, 64, 64), 25).half().float()
    r = render(tp, planes, cams, 64, 1)
    sn.save('render_preset_ffhq48', planes=planes.half(), cams=cams, render_seed=np.array(1), image_raw=r['image_raw'],
            image_depth=r['image_depth'], weights_samples=r['weights_samples'].half(),
            dec_state=np.frombuffer(json.dumps({k: v.tolist() for k, v in tp.decoder.state_dict().items()}).encode(), dtype=np.uint8))


if __name__ == '__main__':
    main()
