#!/usr/bin/env python
"""Golden vectors of the ShapeNet VAE decoder class (vit/vit_triplane.py RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn, the
`--ae_classname` of sample_shapenet_{car,chair,plane}_t23d.sh), run from the reference checkout through ref_shims in the build
container.

    python tests/golden/make_golden_shapenet_decoder.py

The launchers' `vit_decoder` is torch.hub facebookresearch/dinov2 `dinov2_vitb14`, which is not installed: `_RefDino` below follows its
published module layout and eval-mode block (x + ls1 * attn(norm1(x)), x + ls2 * mlp(norm2(x)); exact softmax attention).  The
reference class is then built around it unchanged (it regroups the blocks, swaps in its cross-plane attention and adds the skips).
Weights come from ln3diff_amd.synth.synth_vit_state_dict by state-dict name (seed 0; sigma bias + 4); inputs from seeded CPU generators.  Outputs only (fp16 and sub-sampled where large; the slices are in main()):
  shapenet_dec_small.npz     D = 128 (2 heads), B = 1: every stage (ldm_upsample, each block pair, ViT out, decoder_pred, planes)
  shapenet_dec_b2.npz        D = 128, B = 2: ViT out and planes, each object run through the reference alone (its batched cross-plane
                             attention re-orders query rows across objects when B > 1; decoding is per object)
  shapenet_dec_released.npz  D = 768, B = 1: ldm_upsample, ViT out, decoder_pred, latent_after_vit (sub-sampled), the shapenet64
                             render at 128 x 128 (one view, seeded ray noise) and a 64^3 grid query (sub-sampled)
  shapenet_reparam_b2.npz    D = 128, B = 2: vae_reparameterization(tokens, sample_posterior=False) of the reference class: the encoder
                             tokens [2, 256, 384] (fp16-exact values, stored as fp16), the mode latent [2, 12, 32, 32] and the
                             soft-clamped log-variance [2, 4, 3, 1024] in fp32 (`--reparam-only` writes this file alone)
  shapenet_rendering_kwargs.json   rendering_options_defaults(opts) for the ShapeNet launchers' --cfg / --ray_start / --ray_end
Every .npz carries the state-dict manifest; it is asserted equal to the package class's.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()
ref_shims.ref_dit_modules()

from ln3diff_amd.synth import synth_vit_state_dict, synth_input, orbit_cameras  # noqa: E402

torch.set_grad_enabled(False)
CAM_RADIUS = 1.2
LAUNCHER_FLAGS = dict(cfg='shapenet_tuneray_aug_resolution_64_64_nearestSR', ray_start=0.6, ray_end=1.8)


# ----------------------------------------------------------------------------- dinov2 ViT (hub) stand-in, eval mode
class _LayerScale(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(D))

    def forward(self, x):
        return x * self.gamma


class _MemEffAttention(nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.num_heads = heads
        self.qkv, self.proj = nn.Linear(D, 3 * D), nn.Linear(D, D)

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        return self.proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, C))


class _Mlp(nn.Module):
    def __init__(self, D, I):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(D, I), nn.GELU(), nn.Linear(I, D)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(D, eps=1e-6), _MemEffAttention(D, heads), _LayerScale(D)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(D, eps=1e-6), _Mlp(D, 4 * D), _LayerScale(D)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class _RefDino(nn.Module):
    def __init__(self, D, heads, P=14, img=518):
        super().__init__()
        self.embed_dim = D
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img // P) ** 2 + 1, D))
        self.mask_token = nn.Parameter(torch.zeros(1, D))
        self.patch_embed = nn.Module()
        self.patch_embed.proj = nn.Conv2d(3, D, P, P)
        self.patch_embed.patch_size = (P, P)
        self.blocks = nn.ModuleList([_Block(D, heads) for _ in range(12)])
        self.norm = nn.LayerNorm(D, eps=1e-6)


def ref_rendering_kwargs():
    from nsr import script_util as su
    d = {}
    d.update(su.encoder_and_nsr_defaults())
    d.update(su.loss_defaults())
    d.update(LAUNCHER_FLAGS)
    return su.rendering_options_defaults(types.SimpleNamespace(**d))


def build_ref(D, heads):
    from vit import vit_triplane as vt
    from nsr.triplane import Triplane
    with contextlib.redirect_stdout(io.StringIO()):
        tp = Triplane(25, 128, 3, rendering_kwargs=ref_rendering_kwargs(), out_chans=96, triplane_size=224, decoder_in_chans=32,
                      decoder_output_dim=32, sr_kwargs={}, bcg_synthesis_kwargs={}, lrm_decoder=False)
        dec = vt.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn(_RefDino(D, heads), tp, False, vae_p=2, ldm_z_channels=4, ldm_embed_dim=4)
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    sd = synth_vit_state_dict(shapes, 0)          # pos_embed 0.02 N, LayerScale gammas 1 + 0.1 N
    sd['triplane_decoder.decoder.net.2.bias'] = sd['triplane_decoder.decoder.net.2.bias'].clone()
    sd['triplane_decoder.decoder.net.2.bias'][0] += 4.0
    dec.load_state_dict(sd, strict=True)
    return dec.eval(), shapes


def pkg_manifest(D, heads):
    from ln3diff_amd.vit.vit_triplane_shapenet import RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn, DinoVisionTransformer, \
        shapenet_rendering_kwargs
    from ln3diff_amd.nsr.triplane import Triplane
    tp = Triplane(img_resolution=128, rendering_kwargs=shapenet_rendering_kwargs(**LAUNCHER_FLAGS), decoder_output_dim=32)
    dec = RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn(DinoVisionTransformer(D, 12, heads), tp, False)
    return {k: tuple(v.shape) for k, v in dec.state_dict().items()}


def manifest_json(shapes):
    return np.frombuffer(json.dumps({k: list(v) for k, v in sorted(shapes.items())}).encode(), dtype=np.uint8)


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()}
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print(f'  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)')


def staged(dec, latent):
    """vit_decode_backbone + vit_decode_postprocess of the reference with the stage outputs recorded by forward hooks."""
    st = {}
    hooks = [dec.superresolution['ldm_upsample'].register_forward_hook(lambda m, i, o: st.__setitem__('ldm_upsample', o.clone())),
             dec.decoder_pred.register_forward_hook(lambda m, i, o: st.__setitem__('decoder_pred', o.clone()))]
    for j, blk in enumerate(dec.vit_decoder.blocks):
        hooks.append(blk.register_forward_hook(lambda m, i, o, j=j: st.__setitem__(f'pair{j}', o.clone())))
    with contextlib.redirect_stdout(io.StringIO()):
        vit = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': latent}, 128)
        ret = dec.vit_decode_postprocess(vit, {})
    for h in hooks:
        h.remove()
    st['vit'] = vit
    return st, ret


def reparam_fixture():
    """the encoder side of the class: ldm_downsample -> unpatchify3D -> quant_conv posterior, mode"""
    dec, shapes = build_ref(128, 2)
    assert shapes == pkg_manifest(128, 2), "state-dict manifest differs from the package class (D = 128)"
    tokens = synth_input('shapenet_enc_tokens', (2, 256, 384), 91).half()
    with contextlib.redirect_stdout(io.StringIO()):
        r = dec.vae_reparameterization(tokens.float(), False)
    save('shapenet_reparam_b2', tokens=tokens, latent=r['latent_normalized_2Ddiffusion'], logvar=r['posterior'].logvar,
         manifest=manifest_json(shapes))


def main():
    if '--reparam-only' in sys.argv:
        return reparam_fixture()
    reparam_fixture()
    rk = ref_rendering_kwargs()
    with open(os.path.join(HERE, 'shapenet_rendering_kwargs.json'), 'w') as f:
        json.dump({'flags': LAUNCHER_FLAGS, 'rendering_kwargs': rk}, f, indent=1, sort_keys=True)

    # reduced width, B = 1, every stage (fp16, sub-sampled as SMALL_STEPS says, so that each file stays well under 1 MiB)
    dec, shapes = build_ref(128, 2)
    assert shapes == pkg_manifest(128, 2), "state-dict manifest differs from the package class (D = 128)"
    latent = synth_input('shapenet_latent', (1, 12, 32, 32), 11)
    st, ret = staged(dec, latent)
    arrs = {f'stage_{k}': v.reshape(1, 768, -1)[:, ::8].half() for k, v in st.items() if k.startswith('pair')}
    save('shapenet_dec_small', ldm_upsample=st['ldm_upsample'][:, ::2].half(), vit=st['vit'][:, ::2].half(),
         decoder_pred=st['decoder_pred'][:, ::4, ::8].half(), planes=ret['latent_after_vit'][:, :, ::8, ::8].half(),
         manifest=manifest_json(shapes), **arrs)

    # reduced width, B = 2 (each object through the reference alone)
    lat2 = synth_input('shapenet_latent_b2', (2, 12, 32, 32), 12)
    outs = [staged(dec, lat2[b:b + 1]) for b in range(2)]
    save('shapenet_dec_b2', vit=torch.cat([o[0]['vit'] for o in outs])[:, ::4].half(),
         planes=torch.cat([o[1]['latent_after_vit'] for o in outs])[:, ::2, ::8, ::8].half(), manifest=manifest_json(shapes))

    # released size
    dec, shapes = build_ref(768, 12)
    assert shapes == pkg_manifest(768, 12), "state-dict manifest differs from the package class (D = 768)"
    nparam = sum(int(np.prod(s)) for s in shapes.values())
    print(f'== ShapeNet decoder: {len(shapes)} tensors, {nparam} parameters')
    latent = synth_input('shapenet_latent_rel', (1, 12, 32, 32), 13)
    st, ret = staged(dec, latent)
    cams = orbit_cameras(8, radius=CAM_RADIUS)[[2]]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        r = dec.triplane_decode(ret, cams)
        grid = dec.triplane_decode_grid(ret, 64)
    save('shapenet_dec_released', ldm_upsample=st['ldm_upsample'][:, ::6, ::2].half(), vit=st['vit'][:, ::6, ::2].half(),
         decoder_pred=st['decoder_pred'][:, ::6, ::16].half(), planes=ret['latent_after_vit'][:, :, ::8, ::8].half(),
         image_raw=r['image_raw'].half(), image_depth=r['image_depth'], cams=cams, cam_radius=np.array(CAM_RADIUS), render_seed=np.array(0),
         grid_sigma=grid['sigma'][:, ::2, ::2, ::2].half(), grid_rgb=grid['rgb'][:, ::4, ::4, ::4].half(),
         manifest=manifest_json(shapes), n_params=np.array(nparam))


if __name__ == '__main__':
    main()
