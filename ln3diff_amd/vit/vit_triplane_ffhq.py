"""The FFHQ VAE decoder class (latent [B,12,16,16] -> planes [B,96,256,256] -> renders / grids) on the HIP path.

Mirrors `VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final` of the
reference (vit/vit_triplane.py:516-800, with the parts of its base ViTTriplaneDecomposed :130 that the decode path reaches), same class
name and state-dict keys, so that sample_ffhq_t23d.sh's `--ae_classname` and its checkpoint
(checkpoints/ffhq/model_joint_denoise_rec_model1580000.pt) load.  No FFHQ checkpoint was available when this was written: parity is
against the reference class with synthetic weights (tests/golden/make_golden_ffhq_decoder.py), the released file was never loaded.

Sizes (the launcher passes --arch_decoder vitb, --out_chans 96, --decoder_in_chans 32, --overwrite_diff_inp_size 16 and leaves
--vae_p / --ldm_z_channels at create_3DAE_model's defaults 1 / 4): token_size 16, vae_p 1, so h = vae_p * token_size = 16,
L = h * h = 256 tokens per plane, z = 4: latent [B, 3z = 12, 16, 16] -> [B, 3L = 768, z = 4].
  ldm_upsample   Linear(vae_p^2 * z = 4 -> 768) on each token (no patch embedding) + pos_embed [1, 768, 768]
  vit_decoder    12 DINOv2 ViT-B/14 blocks in 6 TriplaneFusionBlockv3 (vit/vision_transformer.py:1871-1953), tokens viewed as
                 B x 3 planes x 256: two plain DINOv2 blocks over every plane, then `fusion`, a
                 Conv3DCrossAttentionBlockXformerMHA without MLP: x <- x + proj(CA(norm1(x))); CA lets plane i's token (y, x) attend
                 to row y of plane i+1 and column x of plane i+2 with separate wq / w_kv (ln3d_triplane_axis_attention).  UViT long
                 skips feed blocks 3 - 5: x <- x + skip_linear([x, skip]).  GEMM operands are bf16; the weights of the projections
                 that write the residual stream are carried as a bf16 pair (_res_gemm).
  decoder_pred   Linear 768 -> 4*4*128, unpatchify_triplane p = 4 -> [B, 3*128, 64, 64]
  conv_sr        RodinConv3D4X_lite_mlp_as_residual (vision_transformer.py:1047-1151), both convs RodinRollOutConv3D_GroupConv:
                   res = bilinear_256(short_cut(x viewed [B, 3, L, 128] across the plane groups))
                   x0  = res + lrelu(rollout_groupconv3x3(bilinear_256(x^T)))          (x^T: the reference's permute(0, 1, 3, 2))
                   x   = x0 + lrelu(rollout_groupconv3x3(x0))     (plane i reads [x_i | row means of i+1 | column means of i+2])
                 each one launch of the fused implicit-GEMM kernel ln3d_conv3x3_rollout_bf16 per object (C = 128, then C = 32).

The class derives from vit_triplane_shapenet._DinoTriplaneDecoderBase and supplies its `superresolution` entries, its packing, one
fusion block (_group) and the two convolutions (_conv_sr); the per-plane DINOv2 block is dit_models_xformers.vit_block_hip with
_res_gemm as its projection onto the residual stream.

Not built: the encoder side (vae_reparameterization, vit_decode: ldm_downsample / quant_conv / quant_mlp / after_vit_conv exist as
parameters so that checkpoints load strictly, their behaviour raises NotImplementedError), Triplane.superresolution (--sr_training
False; `sr_w_code = w_avg` is carried in the dict and nothing reads it), background tri-planes.  pos_embed is created as zeros (the
reference fills it with a 2-D sin-cos table before the checkpoint overwrites it).  Batches decode each object independently; the
reference's batched cross-plane attention re-orders query rows across objects when B > 1, so only B = 1 agrees with it element for
element.
"""
import torch
import torch.nn as nn

from .. import ops
from ..dit.dit_models_xformers import bf16, f32
from ..nsr.triplane import Triplane
from .vit_triplane_shapenet import (_DinoTriplaneDecoderBase, DinoVisionTransformer, dinov2_vitb14,  # noqa: F401 (dinov2_vitb14: the launcher's)
                                    _XYGridAttn, _RollOutConv3D, _RENDERING_BASE, _ln, _pack_dino)

CLASS_NAME = 'VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final'

# nsr/script_util.py rendering_options_defaults, --cfg ffhq (:433-489): 48 + 48 samples, numeric ray limits, box_warp 1.  No
# white_back key: the ray marcher's default (white) holds, as in the reference.  The launcher passes no --ray_start / --ray_end: the
# preset's own numbers hold.  superresolution_module / superresolution_noise_mode / focal / bg_depth_resolution are carried and unread
# (--sr_training False builds no SR module, there is no background model).
FFHQ_CFGS = {
    'ffhq': dict(superresolution_module='nsr.superresolution.SuperresolutionHybrid8XDC', superresolution_noise_mode='random', focal=4.2647,
                 depth_resolution=48, depth_resolution_importance=48, bg_depth_resolution=16, ray_start=2.25, ray_end=3.3, box_warp=1,
                 avg_camera_radius=2.7, avg_camera_pivot=[0, 0, 0.2]),
}


def ffhq_rendering_kwargs(cfg):
    """rendering_kwargs of the FFHQ launcher's --cfg; an unknown --cfg raises ValueError."""
    if cfg not in FFHQ_CFGS:
        raise ValueError(f"--cfg {cfg}: the FFHQ decoder class is built with the presets {sorted(FFHQ_CFGS)}")
    rk = dict(_RENDERING_BASE)
    rk.update(FFHQ_CFGS[cfg])
    return rk


# ----------------------------------------------------------------------------- parameter containers (reference key layout)
class Conv3DCrossAttentionBlockXformerMHA(nn.Module):           # has_mlp False: norm1 + attn only
    def __init__(self, dim, num_heads, **_):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _XYGridAttn(dim, num_heads)


class TriplaneFusionBlockv3(nn.Module):
    """`fusion_blk_depth` DINOv2 blocks over each plane, then one cross-plane attention block."""

    def __init__(self, vit_blks, num_heads, embed_dim, use_fusion_blk=True, **_):
        super().__init__()
        assert use_fusion_blk
        self.num_branches = 3
        self.vit_blks = vit_blks
        self.fusion = Conv3DCrossAttentionBlockXformerMHA(embed_dim, num_heads)


class RodinConv3D4X_lite_mlp_as_residual(nn.Module):
    def __init__(self, in_chans, out_chans, input_resolution=256, interp_mode='bilinear', bcg_triplane=False):
        super().__init__()
        assert interp_mode == 'bilinear' and in_chans != out_chans and not bcg_triplane
        self.input_resolution, self.out_chans, self.interp_mode = input_resolution, out_chans, interp_mode
        self.conv3D_0 = _RollOutConv3D(in_chans, out_chans)
        self.conv3D_1 = _RollOutConv3D(out_chans, out_chans)
        self.short_cut = nn.Linear(in_chans // 3, out_chans // 3)


# ----------------------------------------------------------------------------- the decoder class
def _pair(w, dev):                               # (bf16(w), bf16(w - bf16(w))): see _res_gemm
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    return bf16(hi, dev), bf16(w - hi.float(), dev)


class VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final(_DinoTriplaneDecoderBase):
    def __init__(self, vit_decoder: DinoVisionTransformer, triplane_decoder: Triplane, cls_token=False, use_fusion_blk=True,
                 fusion_blk_depth=2, channel_multiplier=4, fusion_blk=TriplaneFusionBlockv3, ldm_z_channels=4, ldm_embed_dim=4, vae_p=1,
                 **kwargs):
        super().__init__(vit_decoder, triplane_decoder, cls_token, use_fusion_blk, fusion_blk_depth, fusion_blk, channel_multiplier,
                         ldm_z_channels, ldm_embed_dim, vae_p)

    def _sr_modules(self, D, out_chans):
        vae_p, z, cm = self.vae_p, self.ldm_z_channels, self.channel_multiplier
        quant_mlp = nn.Module()                         # vision_transformer.Mlp(2z, out_features = 2 * embed): fc1 2z -> 2z, fc2
        quant_mlp.fc1, quant_mlp.fc2 = nn.Linear(2 * z, 2 * z), nn.Linear(2 * z, 2 * self.ldm_embed_dim)
        return dict(
            after_vit_conv=nn.Conv2d(2 * out_chans, 2 * out_chans, 3, padding=1),
            quant_conv=nn.Conv2d(2 * out_chans, 2 * out_chans, 1),
            ldm_downsample=nn.Linear(384, vae_p * vae_p * 3 * z * 2),
            ldm_upsample=nn.Linear(vae_p * vae_p * z, D),
            quant_mlp=quant_mlp,
            conv_sr=RodinConv3D4X_lite_mlp_as_residual(int(out_chans * cm), int(out_chans)))

    # ------------------------------------------------------------------ packing
    _res_w = staticmethod(_pair)             # with _res_gemm below

    def _pack_group(self, fb, dev):
        ca = fb.fusion
        return {'vit': [_pack_dino(b, dev, self._res_w) for b in fb.vit_blks],
                'ca_n': _ln(ca.norm1, dev), 'ca_qkv_w': bf16(torch.cat([ca.attn.wq.weight, ca.attn.w_kv.weight], 0), dev),
                'ca_qkv_b': f32(torch.cat([ca.attn.wq.bias, ca.attn.w_kv.bias], 0), dev),
                'ca_o_w': self._res_w(ca.attn.proj.weight, dev), 'ca_o_b': f32(ca.attn.proj.bias, dev)}

    def _pack_sr(self, P, dev):
        sr = self.superresolution
        P['up_w32'], P['up_b'] = f32(sr['ldm_upsample'].weight, dev), f32(sr['ldm_upsample'].bias, dev)
        cs = sr['conv_sr']

        def rollout_conv(conv):                  # [Cout, 3C, 3, 3] groups = 3 -> [3, Cout/3, 27C] in (ky, kx, part, c) order
            w = conv.weight.detach().float()
            g = w.shape[0] // 3
            return bf16(w.permute(0, 2, 3, 1).reshape(3, g, 9 * w.shape[1]), dev), f32(conv.bias.reshape(3, g), dev)
        P['c0'] = rollout_conv(cs.conv3D_0.roll_out_convs)
        P['c1'] = rollout_conv(cs.conv3D_1.roll_out_convs)

    # ------------------------------------------------------------------ ViT pieces
    @staticmethod
    def _res_gemm(a, w, bias, x, **gate):
        """x += gate * (a @ w^T + bias) with the weight carried as a bf16 pair (hi, lo), w = hi + lo up to 2^-17: two accumulating
        launches of the GEMM.  The projections that write the residual stream (attention proj, fc2, the fusion proj, skip_linear) are
        carried this way: measured on the released size with synthetic weights, rounding every ViT weight to one bf16 accounts for
        4.1e-3 of the 4.9e-3 rel-L2 between a single-bf16 path and fp32 at the ViT output (all activation roundings together 2.7e-3),
        and the rounding of these projections lands on the stream directly.  The ShapeNet class keeps single-bf16 weights (the base
        class's one-launch _res_gemm)."""
        ops.gemm(a, w[0], bias, ops.EPI_GATE_RES, x, **gate)
        ops.gemm(a, w[1], None, ops.EPI_GATE_RES, x, **gate)

    def _group(self, x, q, B, N, H):
        for qb in q['vit']:
            self._plane_block(x, qb, B, N, H)
        self._fusion(x, q, B, N, H)

    def _fusion(self, x, q, B, N, H):
        """Conv3DCrossAttentionBlockXformerMHA, has_mlp False: x += proj(axis_attn([wq ; w_kv] norm1(x)))."""
        ws, P = self._ws, self._packed
        M, D = x.shape
        h = ws.get('h', (M, D), torch.bfloat16)
        ops.norm_modulate(x, h, M, D, kind=0, eps=1e-6, weight=q['ca_n'][0], shift=q['ca_n'][1], scale=P['zeros'], mod_rows=M, mod_ld=0)
        qkv = ws.get('ca_qkv', (M, 3 * D), torch.float32)
        ops.gemm(h, q['ca_qkv_w'], q['ca_qkv_b'], ops.EPI_F32, qkv)
        o = ws.get('o', (M, D), torch.bfloat16)
        ops.triplane_axis_attention(qkv, o, B, int(round(N ** 0.5)), H, scale=(D // H) ** -0.5)
        self._res_gemm(o, q['ca_o_w'], q['ca_o_b'], x)

    def _conv_sr(self, up, res, planes_cl, B, r, R, Cm, Co):
        """Both roll-out convolutions as one launch of the fused implicit-GEMM kernel per object; names the stage 'x0' [B, 3, R, R, 32]."""
        x0 = self._conv_x0(up, res, B, r, R, Cm, Co)
        self._conv_planes(x0, planes_cl, B, R, Co)
        return {'x0': x0}

    def _conv_x0(self, up, res, B, r, R, Cm, Co):
        """x0 = resize(res) + lrelu(conv3D_0(roll-out of the bf16 planes `up`))"""
        ws, P = self._ws, self._packed
        rowm = ws.get('rowm0', (B, 3, R, Cm), torch.float32)
        colm = ws.get('colm0', (B, 3, R, Cm), torch.float32)
        ops.rollout_means(up, rowm, colm, B * 3, R, R, Cm)
        x0 = ws.get('x0', (B, 3, R, R, Co), torch.float32)
        for b in range(B):
            ops.conv3x3_rollout(up[b], rowm[b], colm[b], P['c0'][0], P['c0'][1], res[b], x0[b], R, R, Cm, Co, 0.01)
        return x0

    def _conv_planes(self, x0, planes_cl, B, R, Co):
        """planes = x0 + lrelu(conv3D_1(roll-out of x0))"""
        ws, P = self._ws, self._packed
        rowm1 = ws.get('rowm1', (B, 3, R, Co), torch.float32)
        colm1 = ws.get('colm1', (B, 3, R, Co), torch.float32)
        ops.rollout_means(x0, rowm1, colm1, B * 3, R, R, Co)
        for b in range(B):
            ops.conv3x3_rollout(x0[b], rowm1[b], colm1[b], P['c1'][0], P['c1'][1], x0[b], planes_cl[b], R, R, Co, Co, 0.01)

    # ------------------------------------------------------------------ reference-named stages
    @torch.no_grad()
    def vit_decode_backbone(self, latent, img_size=None):
        if isinstance(latent, dict):
            latent = latent['latent_normalized_2Ddiffusion'] if 'latent_normalized' not in latent else latent['latent_normalized']
        if not latent.is_cuda:
            raise RuntimeError("ln3diff_amd decoder runs on the HIP device only (no CPU fallback)")
        self._ensure_packed(latent.device)
        B, z = latent.shape[0], self.ldm_z_channels
        L = 3 * (self.vae_p * self.token_size) ** 2
        if latent.ndim != 3:                                  # [B, 3z, h, h] = B z 3 L/3 -> B 3 L/3 z: a layout copy of 12 KB per object
            latent = latent.reshape(B, latent.shape[1] // 3, 3, L // 3).permute(0, 2, 3, 1).reshape(B, L, -1)
        if tuple(latent.shape) != (B, L, self.vae_p ** 2 * z):
            raise ValueError(f"latent.shape: {tuple(latent.shape)}, expected {(B, L, self.vae_p ** 2 * z)}")
        P, D = self._packed, self._packed['D']
        # K = z = 4 is far below the GEMM's K granularity of 64, so the padding carries an fp32-grade product for free: with
        # x = xh + xl and w = wh + wl split into bf16 halves, [xh | xh | xl] . [wh | wl | wh] = x . w up to the 2^-16 xl . wl term
        # (a single-bf16 product would miss the fp32 Linear by 2^-9 per operand, ten times the ShapeNet class's ldm_upsample gate)
        K = latent.shape[2]
        kp = (3 * K + 63) // 64 * 64
        lat = latent.reshape(B * L, K).float()
        xh = lat.to(torch.bfloat16)
        xb = self._ws.get('lat_bf', (B * L, kp), torch.bfloat16, zero=True)
        xb[:, :K], xb[:, K:2 * K], xb[:, 2 * K:3 * K] = xh, xh, lat - xh.float()
        if 'up_wp' not in P:
            w = P['up_w32']
            wh = w.to(torch.bfloat16)
            P['up_wp'] = torch.zeros(D, kp, device=latent.device, dtype=torch.bfloat16)
            P['up_wp'][:, :K], P['up_wp'][:, K:2 * K], P['up_wp'][:, 2 * K:3 * K] = wh, w - wh.float(), wh
        tok = self._ws.get('up_out', (B * L, D), torch.float32)
        ops.gemm(xb, P['up_wp'], P['up_b'], ops.EPI_F32, tok)
        return self.forward_vit_decoder(tok.view(B, L, D), img_size)

    # ------------------------------------------------------------------ the encoder side is not part of this package
    def vae_reparameterization(self, latent, sample_posterior=True, **kwargs):
        raise NotImplementedError("the FFHQ VAE encoder side (ldm_downsample / quant_conv posterior) is not built; its parameters exist so "
                                  "that checkpoints load strictly.  Decode a latent with vit_decode_backbone + vit_decode_postprocess")

    vae_encode = vae_reparameterization

    def vit_decode(self, latent, img_size, sample_posterior=True, **kwargs):
        return self.vae_reparameterization(latent, sample_posterior)
