"""The ShapeNet VAE decoder class (latent [B,12,32,32] -> planes [B,96,256,256] -> renders / grids) on the HIP path.

Mirrors `RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn` of the reference (vit/vit_triplane.py:802-1121, with the parts of its
base ViTTriplaneDecomposed :130 that the decode path reaches), same class name and state-dict keys, so that the ShapeNet launchers'
`--ae_classname vit.vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn` and their checkpoints load.

Network (launchers: --arch_decoder vitb, DINOv2 ViT-B/14 from torch.hub, --out_chans 96, --decoder_in_chans 32):
  ldm_upsample   PatchEmbedTriplane 12 -> 3 x 768 tokens (ln3d_patch_embed_triplane) + pos_embed [1, 768, 768]
  vit_decoder    12 DINOv2 blocks in 6 pairs (TriplaneFusionBlockv4_nested_init_from_dino, vit/vision_transformer.py:2062), tokens
                 viewed as B x 3 planes x 256.  Block 0 of a pair: per-plane self-attention + MLP.  Block 1: its `attn` is a whole
                 Conv3DCrossAttentionBlockXformerMHANested (norm1 + wq / w_kv / proj) whose output includes its own input, so
                 x <- x + ls1 * (n + CA(norm1'(n))), n = norm1(x); the cross-plane attention lets plane i's token (y, x) attend to row y
                 of plane i+1 and column x of plane i+2 (ln3d_triplane_axis_attention).  UViT long skips feed pairs 3 - 5:
                 x <- x + skip_linear([x, skip]).
  decoder_pred   Linear 768 -> 4*4*128, unpatchify_triplane p = 4 -> [B, 3*128, 64, 64]
  conv_sr        RodinConv3D4X_lite_mlp_as_residual_lite (vision_transformer.py:1202 and its base :1047):
                   res = bilinear_256(short_cut(x viewed [B, 3, L, 128] across the plane groups))
                   x0  = res + lrelu(groupconv3x3(bilinear_256(x^T)))                  (x^T: the reference's permute(0, 1, 3, 2))
                   x   = x0 + lrelu(rollout_groupconv3x3(x0))     (plane i reads [x_i | row means of i+1 | column means of i+2])
Everything runs channel-last; the convolutions are im2col gathers + the MFMA GEMM, one object plane at a time.

This module also holds what this class shares with the FFHQ decoder class (vit_triplane_ffhq.py): the DINOv2 parameter containers and
`_DinoTriplaneDecoderBase` (constructor, packing, forward_vit_decoder, head and tail of vit_decode_postprocess).  The per-plane DINOv2
block is dit_models_xformers.vit_block_hip, the MLP half of the cross-plane block its vit_mlp_hip; the renderer and posterior seams
are the mixins of vit_triplane.py.

Not built: the encoder side (`ldm_downsample` is applied by vae_reparameterization, the ShapeNet VAE encoder itself is not part of
this package), Triplane.superresolution (every launcher passes --sr_training False; `sr_w_code = w_avg` is carried in the dict and
nothing reads it).  Batches decode each object independently; the reference's batched cross-plane attention re-orders query rows
across objects when B > 1, so only B = 1 agrees with it element for element.
"""
import torch
import torch.nn as nn

from .. import ops, _cache
from ..dit.dit_models_xformers import Workspace, bf16, f32, gate_res_gemm, vit_block_hip, vit_mlp_hip
from ..nsr.triplane import Triplane
from .vit_triplane import PatchEmbedTriplane, DiagonalGaussianDistribution, _RendererSeams, _PosteriorSeams

# nsr/script_util.py rendering_options_defaults with the defaults of encoder_and_nsr_defaults() + loss_defaults() (c_scale 1,
# density_reg 0, density_reg_p_dist 0.004, reg_type 'l1'), and the --cfg presets of the ShapeNet launchers (:679-700).  The
# ray limits come from --ray_start / --ray_end, box_warp = ray_end - ray_start.
_RENDERING_BASE = dict(image_resolution=256, disparity_space_sampling=False, clamp_mode='softplus', c_gen_conditioning_zero=True, c_scale=1,
                       superresolution_noise_mode='none', density_reg=0.0, density_reg_p_dist=0.004, reg_type='l1', decoder_lr_mul=1,
                       decoder_activation='sigmoid', sr_antialias=True, return_triplane_features=False, return_sampling_details_flag=False,
                       superresolution_module='utils.torch_utils.components.NearestConvSR')
SHAPENET_CFGS = {
    'shapenet_tuneray_aug_resolution_64_64_nearestSR': dict(depth_resolution=64, depth_resolution_importance=64, white_back=True,
                                                            avg_camera_radius=1.2, avg_camera_pivot=[0, 0, 0],
                                                            superresolution_module='utils.torch_utils.components.NearestConvSR'),
}


def shapenet_rendering_kwargs(cfg, ray_start, ray_end):
    """rendering_kwargs of a ShapeNet launcher's --cfg / --ray_start / --ray_end; an unknown --cfg raises ValueError."""
    if cfg not in SHAPENET_CFGS:
        raise ValueError(f"--cfg {cfg}: the ShapeNet decoder class is built with the presets {sorted(SHAPENET_CFGS)}")
    rk = dict(_RENDERING_BASE)
    rk.update(SHAPENET_CFGS[cfg])
    rk.update(ray_start=float(ray_start), ray_end=float(ray_end), box_warp=float(ray_end) - float(ray_start))
    return rk


# ----------------------------------------------------------------------------- parameter containers (DINOv2 / reference key layout)
class _Gamma(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(D))


class _Attn(nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.num_heads = heads
        self.qkv, self.proj = nn.Linear(D, 3 * D), nn.Linear(D, D)


class _Mlp(nn.Module):
    def __init__(self, D, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(D, I), nn.Linear(I, D)


class _DinoBlock(nn.Module):                  # dinov2 NestedTensorBlock: norm1, attn, ls1, norm2, mlp, ls2
    def __init__(self, D, heads):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(D, eps=1e-6), _Attn(D, heads), _Gamma(D)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(D, eps=1e-6), _Mlp(D, 4 * D), _Gamma(D)


class _PatchEmbed(nn.Module):
    def __init__(self, D, P):
        super().__init__()
        self.proj = nn.Conv2d(3, D, P, P)


class DinoVisionTransformer(nn.Module):
    """Container of torch.hub facebookresearch/dinov2 `dinov2_vit{s,b,l}14` (no registers), the module the reference's ShapeNet
    launchers pass as `vit_decoder` (nsr/script_util.py:1383-1392).  Only its blocks, norm and (replaced) pos_embed are used."""

    def __init__(self, embed_dim=768, depth=12, num_heads=12, patch_size=14, img_size=518):
        super().__init__()
        self.embed_dim, self.num_heads, self.patch_size = embed_dim, num_heads, patch_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img_size // patch_size) ** 2 + 1, embed_dim))
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        self.patch_embed = _PatchEmbed(embed_dim, patch_size)
        self.blocks = nn.ModuleList([_DinoBlock(embed_dim, num_heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)


def dinov2_vitb14(**kw):
    return DinoVisionTransformer(768, 12, 12, **kw)


class _XYGridAttn(nn.Module):                # xformer_Conv3D_Aware_CrossAttention_xygrid
    def __init__(self, D, heads):
        super().__init__()
        self.num_heads = heads
        self.wq, self.w_kv, self.proj = nn.Linear(D, D), nn.Linear(D, 2 * D), nn.Linear(D, D)


class Conv3DCrossAttentionBlockXformerMHANested(nn.Module):
    def __init__(self, dim, num_heads, **_):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _XYGridAttn(dim, num_heads)


class TriplaneFusionBlockv4_nested_init_from_dino(nn.Module):
    """Two DINOv2 blocks; the second block's attention is replaced by the cross-plane block, initialised from its qkv / proj."""

    def __init__(self, vit_blks, num_heads, embed_dim, use_fusion_blk=True, **_):
        super().__init__()
        assert use_fusion_blk and len(vit_blks) == 2
        self.num_branches = 3
        self.vit_blks = vit_blks
        ca = Conv3DCrossAttentionBlockXformerMHANested(embed_dim, num_heads)
        qkv = vit_blks[1].attn.qkv
        with torch.no_grad():
            ca.attn.proj.load_state_dict(vit_blks[1].attn.proj.state_dict())
            ca.attn.wq.weight.copy_(qkv.weight[:embed_dim])
            ca.attn.w_kv.weight.copy_(qkv.weight[embed_dim:])
            ca.attn.wq.bias.copy_(qkv.bias[:embed_dim])
            ca.attn.w_kv.bias.copy_(qkv.bias[embed_dim:])
        del self.vit_blks[1].attn
        self.vit_blks[1].attn = ca


class _RollOutInplaneConv(nn.Module):         # RodinRollOut_GroupConv_noConv3D
    def __init__(self, cin, cout):
        super().__init__()
        self.roll_out_inplane_conv = nn.Conv2d(cin, cout, 3, padding=1, groups=3)


class _RollOutConv3D(nn.Module):              # RodinRollOutConv3D_GroupConv
    def __init__(self, cin, cout):
        super().__init__()
        self.roll_out_convs = nn.Conv2d(3 * cin, cout, 3, padding=1, groups=3)


class RodinConv3D4X_lite_mlp_as_residual_lite(nn.Module):
    def __init__(self, in_chans, out_chans, input_resolution=256, interp_mode='bilinear'):
        super().__init__()
        assert interp_mode == 'bilinear' and in_chans != out_chans
        self.input_resolution, self.out_chans, self.interp_mode = input_resolution, out_chans, interp_mode
        self.conv3D_0 = _RollOutInplaneConv(in_chans, out_chans)
        self.conv3D_1 = _RollOutConv3D(out_chans, out_chans)
        self.short_cut = nn.Linear(in_chans // 3, out_chans // 3)


# ----------------------------------------------------------------------------- what the two DINO-based decoder classes share
def _ln(m, dev):
    return f32(m.weight, dev), f32(m.bias, dev)


def _pack_mlp(b, dev, res_w=bf16):
    """MLP half of a DINOv2 block as vit_mlp_hip's operands; res_w packs the weight of the GEMM that writes the residual stream."""
    return {'n2': _ln(b.norm2, dev), 'fc1_w': bf16(b.mlp.fc1.weight, dev), 'fc1_b': f32(b.mlp.fc1.bias, dev),
            'fc2_w': res_w(b.mlp.fc2.weight, dev), 'fc2_b': f32(b.mlp.fc2.bias, dev), 'ls2': f32(b.ls2.gamma, dev)}


def _pack_dino(b, dev, res_w=bf16):
    """A whole DINOv2 block as vit_block_hip's operands."""
    return {'n1': _ln(b.norm1, dev), 'qkv_w': bf16(b.attn.qkv.weight, dev), 'qkv_b': f32(b.attn.qkv.bias, dev),
            'o_w': res_w(b.attn.proj.weight, dev), 'o_b': f32(b.attn.proj.bias, dev), 'ls1': f32(b.ls1.gamma, dev), **_pack_mlp(b, dev, res_w)}


class _DinoTriplaneDecoderBase(_RendererSeams, _cache.PackedWeights, nn.Module):
    """Latent tokens -> DINOv2 blocks in fusion groups with UViT long skips -> decoder_pred -> unpatchify -> conv_sr -> tri-planes.
    A subclass gives its `superresolution` entries (_sr_modules), packs its token embedding, fusion groups and conv_sr convolutions
    (_pack_sr, _pack_group), runs one fusion group (_group) and the two convolutions of conv_sr (_conv_sr = _conv_x0 + _conv_planes);
    `_res_w` / `_res_gemm` are how it carries and applies the weights of the projections that write the residual stream.  Every step of
    the forward is a method of its own (_add_pos, _skip_step, _group, _final_norm, _pred, _unpatchify, _short_cut, _upsample), so that a
    test can drive one step on an input of its choice; forward_vit_decoder and vit_decode_postprocess are those steps in order."""
    _res_w = staticmethod(bf16)
    _res_gemm = staticmethod(gate_res_gemm)

    def __init__(self, vit_decoder, triplane_decoder, cls_token, use_fusion_blk, fusion_blk_depth, fusion_blk, channel_multiplier,
                 ldm_z_channels, ldm_embed_dim, vae_p):
        super().__init__()
        assert not cls_token and fusion_blk_depth == 2
        self.cls_token, self.vae_p, self.token_size, self.plane_n = cls_token, vae_p, 16, 3
        self.ldm_z_channels, self.ldm_embed_dim, self.channel_multiplier = ldm_z_channels, ldm_embed_dim, channel_multiplier
        self.superresolution = nn.ModuleDict({})
        self.vit_decoder, self.triplane_decoder = vit_decoder, triplane_decoder
        self.patch_size = vit_decoder.patch_size
        D = vit_decoder.embed_dim
        out_chans = getattr(triplane_decoder, "out_chans", 3 * triplane_decoder.decoder_in_chans)     # --out_chans 96
        self.unpatchify_out_chans = out_chans
        self.decoder_pred = nn.Linear(D, 4 ** 2 * int(out_chans // 3 * channel_multiplier))
        self.vit_decoder.pos_embed = nn.Parameter(torch.zeros(1, 3 * self.token_size ** 2, D))
        blks = vit_decoder.blocks
        assert len(blks) == 12, 'ViT-B by default'
        nh = blks[0].attn.num_heads
        self.vit_decoder.blocks = nn.ModuleList([fusion_blk(blks[i:i + fusion_blk_depth], nh, D, use_fusion_blk)
                                                 for i in range(0, len(blks), fusion_blk_depth)])
        self.register_buffer('w_avg', torch.zeros([512]))
        self.rendering_kwargs = triplane_decoder.rendering_kwargs
        self.superresolution.update(self._sr_modules(D, out_chans))
        self.reparameterization_soft_clamp = True
        for blk in self.vit_decoder.blocks[len(self.vit_decoder.blocks) // 2:]:       # create_uvit_arch
            blk.skip_linear = nn.Linear(2 * D, D)
            nn.init.constant_(blk.skip_linear.weight, 0)
            nn.init.constant_(blk.skip_linear.bias, 0)
        self._ws = None

    # ------------------------------------------------------------------ packing
    def _pack(self, P, dev):
        vd, cs = self.vit_decoder, self.superresolution['conv_sr']
        D = vd.embed_dim
        P.update({'D': D, 'H': vd.blocks[0].vit_blks[0].attn.num_heads, 'pos': f32(vd.pos_embed.reshape(-1), dev), 'groups': []})
        for fb in vd.blocks:
            q = self._pack_group(fb, dev)
            if hasattr(fb, 'skip_linear'):
                w = fb.skip_linear.weight
                q['skip_wx'], q['skip_ws'] = self._res_w(w[:, :D], dev), self._res_w(w[:, D:], dev)
                q['skip_b'] = f32(fb.skip_linear.bias, dev)
            P['groups'].append(q)
        P['norm'] = _ln(vd.norm, dev)
        P['dp_w'], P['dp_b'] = bf16(self.decoder_pred.weight, dev), f32(self.decoder_pred.bias, dev)
        P['sc_w'], P['sc_b'] = bf16(cs.short_cut.weight, dev), f32(cs.short_cut.bias, dev)
        P['zeros'] = torch.zeros(D, device=dev)
        self._pack_sr(P, dev)
        self._ws = Workspace(dev)

    # ------------------------------------------------------------------ ViT pieces
    def _plane_block(self, x, q, B, N, H):
        """DINOv2 block over each plane's N tokens (objects x planes = B*3 attention batches)."""
        vit_block_hip(self._ws, x, q, B * 3, N, H, self._packed['zeros'], 1e-6, ops.EPI_GELU_ERF, res_gemm=self._res_gemm)

    def _add_pos(self, x, h):
        """h [B*L, D] <- x [B, L, D] + pos_embed"""
        B, L, D = x.shape
        ops.add_table_rows(x.contiguous().float(), self._packed['pos'], h, 1, B, L * D)

    def _skip_step(self, h, q, skip):
        """h += skip_linear([h, skip]) as two projections onto the residual stream; skip: the bf16 copy of an earlier token state"""
        M, D = h.shape
        xb = self._ws.get('skip_x', (M, D), torch.bfloat16)
        ops.cast_bf16(h, xb)
        self._res_gemm(xb, q['skip_wx'], q['skip_b'], h)
        self._res_gemm(skip, q['skip_ws'], None, h)

    def _final_norm(self, h, out):
        M, D = h.shape
        ops.layernorm_f32(h, self._packed['norm'][0], self._packed['norm'][1], out, M, D, 1e-6)

    @torch.no_grad()
    def forward_vit_decoder(self, x, img_size=None):
        """x [B, 3*256, D] (ldm_upsample output) -> + pos_embed -> 6 fusion groups with UViT skips -> norm; returns f32 [B, 3*256, D].
        `stage_hook(name, tensor)`, when set on the instance, sees the token state after each fusion group (tests)."""
        if not x.is_cuda:
            raise RuntimeError("ln3diff_amd decoder runs on the HIP device only (no CPU fallback)")
        self._ensure_packed(x.device)
        P, ws = self._packed, self._ws
        B, L, D = x.shape
        H, N, M = P['H'], L // 3, B * L
        h = ws.get('x', (M, D), torch.float32)
        self._add_pos(x, h)
        groups = P['groups']
        hook = self.__dict__.get('stage_hook')
        skips = []

        def push():
            s = ws.get(f'skip{len(skips)}', (M, D), torch.bfloat16)
            ops.cast_bf16(h, s)
            skips.append(s)
        push()
        for j, q in enumerate(groups):
            if j >= len(groups) // 2:
                self._skip_step(h, q, skips.pop())
            self._group(h, q, B, N, H)
            if j < len(groups) // 2 - 1:
                push()
            if hook is not None:
                hook(f'blk{j}', h.view(B, L, D))
        out = torch.empty(B, L, D, device=x.device, dtype=torch.float32)
        self._final_norm(h, out)
        return out

    # ------------------------------------------------------------------ the steps of vit_decode_postprocess in front of conv_sr
    def _pred(self, latent_from_vit):
        """decoder_pred: f32 tokens [B, L, D] -> f32 [B*L, 16*Cm]"""
        P, ws = self._packed, self._ws
        B, L, D = latent_from_vit.shape
        xb = ws.get('tok_bf', (B * L, D), torch.bfloat16)
        ops.cast_bf16(latent_from_vit.contiguous(), xb)
        pred = ws.get('pred', (B * L, P['dp_w'].shape[0]), torch.float32)
        ops.gemm(xb, P['dp_w'], P['dp_b'], ops.EPI_F32, pred)
        return pred

    def _unpatchify(self, pred, B):
        """unpatchify_triplane (p = 4): -> the low-resolution planes f32 [B*3, r, r, Cm] and short_cut's view of them, bf16 [B*3*r*r, Cm]"""
        ws = self._ws
        S, p, Cm = self.token_size, 4, self._packed['dp_w'].shape[0] // 16
        r = S * p
        lo = ws.get('lo', (B * 3, r, r, Cm), torch.float32)
        mixed = ws.get('mixed', (B * 3 * r * r, Cm), torch.bfloat16)
        ops.sr_unpatchify(pred, lo, mixed, B, S, p, Cm)
        return lo, mixed

    def _short_cut(self, mixed, B):
        P = self._packed
        r, Co = self.token_size * 4, P['sc_w'].shape[0]
        res = self._ws.get('res', (B, 3, r, r, Co), torch.float32)
        ops.gemm(mixed, P['sc_w'], P['sc_b'], ops.EPI_F32, res)
        return res

    def _upsample(self, lo, B, R):
        """the transposed planes (the reference's permute(0, 1, 3, 2)) resized to R x R, bf16: the first convolution's operand"""
        _, r, _, Cm = lo.shape
        up = self._ws.get('up', (B, 3, R, R, Cm), torch.bfloat16)
        ops.resize_bilinear_cl(lo, up, B * 3, r, r, R, R, Cm, transpose=True)
        return up

    @torch.no_grad()
    def vit_decode_postprocess(self, latent_from_vit, ret_dict: dict, want_nchw=True, return_stages=False):
        """decoder_pred -> unpatchify_triplane (p = 4) -> conv_sr.  Adds 'planes_channel_last' [B, 3, R, R, 32] (the renderer's layout),
        'latent_after_vit' [B, 96, R, R] (want_nchw), 'sr_w_code' and 'cls_token' (None) to ret_dict; return_stages also adds
        'decoder_pred' [B, 768, 2048], the low-resolution planes 'planes_lowres' [B, 3, 64, 64, 128] (channel-last) and whatever stages
        the class's _conv_sr names."""
        P = self._packed
        B, L, D = latent_from_vit.shape
        dev = latent_from_vit.device
        cs = self.superresolution['conv_sr']
        S, p, Cm = self.token_size, 4, P['dp_w'].shape[0] // 16
        r, R, Co = S * p, cs.input_resolution, cs.out_chans // 3
        pred = self._pred(latent_from_vit)
        lo, mixed = self._unpatchify(pred, B)
        res = self._short_cut(mixed, B)
        up = self._upsample(lo, B, R)
        planes_cl = torch.empty(B, 3, R, R, Co, device=dev, dtype=torch.float32)
        stages = self._conv_sr(up, res, planes_cl, B, r, R, Cm, Co)
        ret_dict.update(dict(cls_token=None, planes_channel_last=planes_cl,
                             sr_w_code=self.w_avg.reshape(1, 1, -1).expand(B, 1, self.w_avg.numel())))
        if want_nchw:
            nchw = torch.empty(B, 3 * Co, R, R, device=dev, dtype=torch.float32)
            ops.planes_to_nchw(planes_cl, nchw, B, Co, R, R)
            ret_dict['latent_after_vit'] = nchw
        if return_stages:
            ret_dict['decoder_pred'] = pred.view(B, L, -1).clone()
            ret_dict['planes_lowres'] = lo.view(B, 3, r, r, Cm).clone()
            ret_dict.update({k: v.clone() for k, v in stages.items()})
        return ret_dict


# ----------------------------------------------------------------------------- the decoder class
class RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn(_PosteriorSeams, _DinoTriplaneDecoderBase):
    def __init__(self, vit_decoder: DinoVisionTransformer, triplane_decoder: Triplane, cls_token=False, use_fusion_blk=True,
                 fusion_blk_depth=2, fusion_blk=TriplaneFusionBlockv4_nested_init_from_dino, channel_multiplier=4, ldm_z_channels=4,
                 ldm_embed_dim=4, vae_p=2, **kwargs):
        assert vae_p == 2
        super().__init__(vit_decoder, triplane_decoder, cls_token, use_fusion_blk, fusion_blk_depth, fusion_blk, channel_multiplier,
                         ldm_z_channels, ldm_embed_dim, vae_p)

    def _sr_modules(self, D, out_chans):
        vae_p, z, cm = self.vae_p, self.ldm_z_channels, self.channel_multiplier
        return dict(
            ldm_downsample=nn.Linear(384, vae_p * vae_p * 3 * z * 2),
            ldm_upsample=PatchEmbedTriplane(vae_p * self.token_size, vae_p, 3 * self.ldm_embed_dim, D),
            quant_conv=nn.Conv2d(2 * 3 * z, 2 * self.ldm_embed_dim * 3, kernel_size=1, groups=3),
            conv_sr=RodinConv3D4X_lite_mlp_as_residual_lite(int(out_chans * cm), int(out_chans)))

    # ------------------------------------------------------------------ packing
    def _pack_group(self, fb, dev):
        b0, b1 = fb.vit_blks[0], fb.vit_blks[1]
        ca = b1.attn
        g1 = b1.ls1.gamma.detach().float()
        q1 = {'n1': _ln(b1.norm1, dev), 'n1g': (f32(b1.norm1.weight.detach().float() * g1, dev), f32(b1.norm1.bias.detach().float() * g1, dev)),
              'ca_n': _ln(ca.norm1, dev), 'qkv_w': bf16(torch.cat([ca.attn.wq.weight, ca.attn.w_kv.weight], 0), dev),
              'qkv_b': f32(torch.cat([ca.attn.wq.bias, ca.attn.w_kv.bias], 0), dev),
              'o_w': bf16(ca.attn.proj.weight, dev), 'o_b': f32(ca.attn.proj.bias, dev), 'ls1': f32(g1, dev), **_pack_mlp(b1, dev)}
        return {'b0': _pack_dino(b0, dev), 'b1': q1}

    def _pack_sr(self, P, dev):
        sr = self.superresolution
        P['pe_w'], P['pe_b'] = f32(sr['ldm_upsample'].proj.weight, dev), f32(sr['ldm_upsample'].proj.bias, dev)
        cs = sr['conv_sr']

        def group_conv(conv):                    # [Cout, Cin/3, 3, 3] groups = 3 -> per group [Cout/3, Kpad] in (ky, kx, c) order
            w = conv.weight.detach().float()
            g = w.shape[0] // 3
            k = 9 * w.shape[1]
            kpad = (k + 63) // 64 * 64
            out = []
            for d in range(3):
                m = torch.zeros(g, kpad)
                m[:, :k] = w[d * g:(d + 1) * g].permute(0, 2, 3, 1).reshape(g, k).cpu()
                out.append((bf16(m, dev), f32(conv.bias[d * g:(d + 1) * g], dev)))
            return out, kpad
        P['c0'], P['c0_kpad'] = group_conv(cs.conv3D_0.roll_out_inplane_conv)
        P['c1'], P['c1_kpad'] = group_conv(cs.conv3D_1.roll_out_convs)

    # ------------------------------------------------------------------ ViT pieces
    def _group(self, x, q, B, N, H):
        self._plane_block(x, q['b0'], B, N, H)
        self._cross_block(x, q['b1'], B, N, H)

    def _cross_block(self, x, q, B, N, H):
        """DINOv2 block whose attention is the nested cross-plane block: x += ls1 * (n + proj(axis_attn(norm1'(n)))), n = norm1(x)."""
        ws, P = self._ws, self._packed
        M, D = x.shape
        n = ws.get('n', (M, D), torch.float32)
        r = ws.get('r', (M, D), torch.float32)
        ops.layernorm_f32(x, q['n1'][0], q['n1'][1], n, M, D, 1e-6)
        ops.layernorm_f32(x, q['n1g'][0], q['n1g'][1], r, M, D, 1e-6)           # ls1 * n: the inner block's residual, gated
        h = ws.get('h', (M, D), torch.bfloat16)
        ops.norm_modulate(n, h, M, D, kind=0, eps=1e-6, weight=q['ca_n'][0], shift=q['ca_n'][1], scale=P['zeros'], mod_rows=M, mod_ld=0)
        qkv = ws.get('ca_qkv', (M, 3 * D), torch.float32)
        ops.gemm(h, q['qkv_w'], q['qkv_b'], ops.EPI_F32, qkv)
        o = ws.get('o', (M, D), torch.bfloat16)
        ops.triplane_axis_attention(qkv, o, B, int(round(N ** 0.5)), H, scale=(D // H) ** -0.5)
        ops.gemm(o, q['o_w'], q['o_b'], ops.EPI_GATE_RES, x, gate=q['ls1'], gate_rows=1, gate_ld=0, res_bias=r, res_bias_ld=D)
        vit_mlp_hip(ws, x, q, P['zeros'], 1e-6, ops.EPI_GELU_ERF)

    def _conv_sr(self, up, res, planes_cl, B, r, R, Cm, Co):
        """Both 3x3 group convolutions as im2col gathers + the MFMA GEMM, one object plane at a time."""
        x0 = self._conv_x0(up, res, B, r, R, Cm, Co)
        self._conv_planes(x0, planes_cl, B, R, Co)
        return {}

    def _conv_x0(self, up, res, B, r, R, Cm, Co):
        """x0 = resize(res) + lrelu(conv3D_0(up)); the convolution's output stays in the scratch 't'"""
        P, ws = self._packed, self._ws
        N = B * 3
        up = up.view(N, R, R, Cm)
        t = ws.get('t', (N, R * R, Co), torch.float32)
        col = ws.get('col0', (R * R, P['c0_kpad']), torch.bfloat16)
        for n in range(N):
            w, b = P['c0'][n % 3]
            ops.im2col3x3(up[n], col, 1, R, R, Cm, 1, P['c0_kpad'])
            ops.gemm(col, w, b, ops.EPI_F32, t[n])
        x0 = ws.get('x0', (B, 3, R, R, Co), torch.float32)
        ops.resize_add_lrelu(res, t, x0, N, r, r, R, R, Co, 0.01)
        return x0

    def _conv_planes(self, x0, planes_cl, B, R, Co):
        """planes = x0 + lrelu(conv3D_1(roll-out of x0)); the convolution's output stays in the scratch 't'"""
        P, ws = self._packed, self._ws
        N = B * 3
        t = ws.get('t', (N, R * R, Co), torch.float32)
        rowm = ws.get('rowm', (B, 3, R, Co), torch.float32)
        colm = ws.get('colm', (B, 3, R, Co), torch.float32)
        ops.rollout_means(x0, rowm, colm, N, R, R, Co)
        col = ws.get('col1', (R * R, P['c1_kpad']), torch.bfloat16)
        for b in range(B):
            for i in range(3):
                w, bias = P['c1'][i]
                ops.im2col3x3_rollout(x0[b], rowm[b], colm[b], col, i, R, R, Co, P['c1_kpad'])
                ops.gemm(col, w, bias, ops.EPI_F32, t[b * 3 + i])
        ops.resize_add_lrelu(x0, t, planes_cl, N, R, R, R, R, Co, 0.01)

    # ------------------------------------------------------------------ reference-named stages
    @torch.no_grad()
    def vit_decode_backbone(self, latent, img_size=None):
        if isinstance(latent, dict):
            latent = latent['latent_normalized_2Ddiffusion']
        if not latent.is_cuda:
            raise RuntimeError("ln3diff_amd decoder runs on the HIP device only (no CPU fallback)")
        self._ensure_packed(latent.device)
        B = latent.shape[0]
        D, S = self._packed['D'], self.vae_p * self.token_size
        L = 3 * self.token_size ** 2
        raw = self._ws.get('pe_raw', (B * L, D), torch.float32)
        ops.patch_embed_triplane(latent.contiguous().float(), self._packed['pe_w'], self._packed['pe_b'],
                                 self._ws.get('pe_silu', (B * L, D), torch.bfloat16), raw, B, self.ldm_embed_dim, S, self.vae_p, D)
        return self.forward_vit_decoder(raw.view(B, L, D), img_size)

    def _down_packed(self, dev):
        """ldm_downsample's GEMM operands (a side pack, as _quant_packed)"""
        ld = self.superresolution['ldm_downsample']
        return self._side_pack('down', dev, lambda dev: {'w': bf16(ld.weight, dev), 'b': f32(ld.bias, dev)})

    @torch.no_grad()
    def vae_reparameterization(self, latent, sample_posterior, eps=None):
        """latent: ViT encoder tokens [B, 256, 384] -> ldm_downsample -> unpatchify3D (p = 2) -> quant_conv posterior (mode, or
        mean + std * eps with eps [B, 4, 3, 1024]; sampling without eps draws it like the reference, on the CPU generator)."""
        if not latent.is_cuda:
            raise RuntimeError("ln3diff_amd decoder runs on the HIP device only (no CPU fallback)")
        dev = latent.device
        ld = self.superresolution['ldm_downsample']
        q = self._down_packed(dev)
        B, T, Ce = latent.shape
        xb = torch.empty(B * T, Ce, device=dev, dtype=torch.bfloat16)
        ops.cast_bf16(latent.contiguous().float(), xb)
        y = torch.empty(B * T, ld.weight.shape[0], device=dev, dtype=torch.float32)
        ops.gemm(xb, q['w'], q['b'], ops.EPI_F32, y)
        t, p, Cz = self.token_size, self.vae_p, 2 * self.ldm_z_channels
        # unpatchify3D 'nhwpqdc->ndhpwqc' then B 3 C H W -> B 3C H W: a layout copy for the posterior kernel's NCHW input
        h = y.view(B, t, t, p, p, 3, Cz).permute(0, 5, 6, 1, 3, 2, 4).reshape(B, 3 * Cz, t * p, t * p)
        HW = (t * p) ** 2
        if sample_posterior and eps is None:
            eps = torch.randn(B, self.ldm_embed_dim, 3, HW)
        r = self._posterior(h, eps if sample_posterior else None, 1)
        return dict(normal_entropy=r['entropy'], latent_normalized=r['latent_tok'],
                    latent_normalized_2Ddiffusion=r['z'].view(B, -1, t * p, t * p), log_q_2Ddiffusion=r['log_q'].view(B, -1, t * p, t * p),
                    log_q=r['log_q'], posterior=DiagonalGaussianDistribution(r['mean'], r['logvar']))

    @torch.no_grad()
    def vit_decode(self, latent, img_size, sample_posterior=True, eps=None, **kwargs):
        ret_dict = self.vae_reparameterization(latent, sample_posterior, eps=eps)
        tok = self.vit_decode_backbone(ret_dict, img_size)
        return self.vit_decode_postprocess(tok, ret_dict)
