"""Tri-plane VAE decoder (latent [B,12,32,32] -> planes [B,96,128,128] -> renders / grids) on the HIP path.

Mirrors the released decoder class of the reference (vit/vit_triplane.py:1982, same long class name so that
`construct_class_by_name` strings keep working) for the methods the samplers call:
vit_decode_backbone :996, vit_decode_postprocess :1913, triplane_decode :1013, forward_points :2009,
triplane_decode_grid :2052; state-dict keys `superresolution.ldm_upsample.*`, `superresolution.conv_sr.*`
(ldm Decoder: ldm/modules/diffusionmodules/model.py:625-745), `vit_decoder.*`, `triplane_decoder.decoder.*`.

Everything runs channel-last on the device: the DiT2 token stream [B*3, 16*16, D] IS the NHWC input of the conv decoder, whose blocks
(3x3 conv as im2col + GEMM with the nearest-2x upsample fused into the gather, GroupNorm+swish, ResnetBlock) and their launch
sequences are those of ln3diff_amd/convstack.py, on scratch from this decoder's Workspace.  The decoder's last GEMM writes the planes
directly in the [B,3,H,W,32] layout the ray-marcher gathers from (the reference layout [B,96,H,W] is produced only when a caller
asks for `latent_after_vit`)."""
import torch
import torch.nn as nn

from .. import ops, _cache
from ..convstack import ConvStack, pack_conv3, pack_gn, pack_lin, pack_resblock
from ..dit.dit_decoder import DiT2
from ..dit.dit_models_xformers import Workspace, f32, self_attention_hip
from ..nsr.triplane import Triplane


class DiagonalGaussianDistribution:
    """The posterior object of the reference (utils/torch_utils/distributions/distributions.py:44-88, soft_clamp=True) as far as the
    encoder path produces it: mean / logvar [B, C, 3, H*W] (logvar already soft-clamped by ln3d_mv_posterior); mode() is the mean.
    Sampling, log_p and the entropy are computed inside the fused kernel (vae_reparameterization)."""

    def __init__(self, mean, logvar):
        self.mean, self.logvar = mean, logvar

    def mode(self):
        return self.mean


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, k, padding=k // 2)


class _GN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))


class ResnetBlock(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1, self.conv1 = _GN(in_channels), _conv(in_channels, out_channels, 3)
        self.norm2, self.conv2 = _GN(out_channels), _conv(out_channels, out_channels, 3)
        if in_channels != out_channels:
            self.nin_shortcut = _conv(in_channels, out_channels, 1)


class AttnBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = _GN(c)
        self.q, self.k, self.v, self.proj_out = _conv(c, c, 1), _conv(c, c, 1), _conv(c, c, 1), _conv(c, c, 1)


class _Up(nn.Module):
    pass


class Decoder(nn.Module):
    """Container with the ldm Decoder's module tree (ch=32, ch_mult=[1,2,2,4], num_res_blocks=1, out_ch=32)."""

    def __init__(self, *, ch=32, out_ch=32, ch_mult=(1, 2, 2, 4), num_res_blocks=1, z_channels=1024, **_):
        super().__init__()
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        block_in = ch * ch_mult[-1]
        self.conv_in = _conv(z_channels, block_in, 3)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(block_in, block_in)
        self.mid.attn_1 = AttnBlock(block_in)
        self.mid.block_2 = ResnetBlock(block_in, block_in)
        self.up = nn.ModuleList()
        for lvl in reversed(range(self.num_resolutions)):
            up = _Up()
            up.block = nn.ModuleList()
            block_out = ch * ch_mult[lvl]
            for _ in range(num_res_blocks + 1):
                up.block.append(ResnetBlock(block_in, block_out))
                block_in = block_out
            if lvl != 0:
                up.upsample = nn.Module()
                up.upsample.conv = _conv(block_in, block_in, 3)
            self.up.insert(0, up)
        self.norm_out = _GN(block_in)
        self.conv_out = _conv(block_in, out_ch, 3)


class PatchEmbedTriplane(nn.Module):
    def __init__(self, img_size=32, patch_size=2, in_chans=12, embed_dim=768):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim * 3, kernel_size=patch_size, stride=patch_size, groups=3)


class _RendererSeams:
    """The renderer side shared by the three decoder classes: tri-planes (a vit_decode_postprocess dict or [B, 96, H, W]) -> renders,
    point queries and grids.  The class that inherits it provides `triplane_decoder` (nsr.triplane.Triplane) and `rendering_kwargs`."""
    grid_ignores_aabb = False                  # triplane_decode_grid(aabb=...): raise, or (the Objaverse class) use the preset's box anyway

    @torch.no_grad()
    def triplane_decode(self, vit_decode_out, c, return_raw_only=False, **kwargs):
        """The reference also passes ws = sr_w_code, which only Triplane.superresolution reads (not built: --sr_training False)."""
        if isinstance(vit_decode_out, dict):
            pcl = vit_decode_out.get('planes_channel_last')
            planes = vit_decode_out.get('latent_after_vit')
        else:
            pcl, planes = None, vit_decode_out
            vit_decode_out = dict(latent_normalized=planes)
        if pcl is not None:
            V = c.shape[0]
            idx = kwargs.pop('plane_index', None)
            if idx is None:
                assert pcl.shape[0] in (V, 1)
                idx = torch.arange(V, device=c.device, dtype=torch.int32) if pcl.shape[0] == V else \
                    torch.zeros(V, device=c.device, dtype=torch.int32)
            ret = self.triplane_decoder(c=c, planes_channel_last=pcl, plane_index=idx, **kwargs)
        else:
            ret = self.triplane_decoder(planes, c, **kwargs)
        ret.update({'latent_after_vit': planes, **vit_decode_out})
        return ret

    @torch.no_grad()
    def triplane_renderer(self, latent, coordinates, directions=None):
        """decoder output at explicit points (vit/vit_triplane.py:377-388 -> renderer.run_model): latent = tri-planes
        [B,96,H,W] / dict, coordinates [B,P,3] -> {'rgb': [B,P,3], 'sigma': [B,P,1]} (directions are unused by OSGDecoder)."""
        if isinstance(latent, dict):
            pcl = latent.get('planes_channel_last')
            if pcl is None:
                pcl = self.triplane_decoder.to_channel_last(latent['latent_after_vit'])
        else:
            pcl = self.triplane_decoder.to_channel_last(latent)
        return self.forward_points(pcl, coordinates)

    @torch.no_grad()
    def forward_points(self, planes_channel_last, points, chunk_size=2 ** 16, with_grad=False):
        """with_grad: also 'sigma_grad' and 'normal' [B,P,3] (Triplane.query_points)."""
        outs = [self.triplane_decoder.query_points(planes_channel_last[n], points[n], with_grad=with_grad) for n in range(points.shape[0])]
        return {k: torch.stack([o[k] for o in outs], 0) for k in outs[0]}

    @torch.no_grad()
    def snap_points(self, planes_channel_last, points, level, iters, **kw):
        """points [B,P,3] put onto sigma = level of planes_channel_last[n] (Triplane.snap_points; **kw: its tol, max_step, max_dist) ->
        {'points': [B,P,3], 'residual', 'state', 'evals': [B,P]}"""
        outs = [self.triplane_decoder.snap_points(planes_channel_last[n], points[n], level, iters, **kw) for n in range(points.shape[0])]
        return {k: torch.stack([o[k] for o in outs], 0) for k in outs[0]}

    @torch.no_grad()
    def triplane_decode_grid(self, vit_decode_out, grid_size, aabb=None, **kwargs):
        """vit_triplane.py:290-337, :2052: the grid spans sampler_bbox_min / max when the preset has them, else +- box_warp / 2 (ShapeNet)."""
        pcl = vit_decode_out.get('planes_channel_last')
        if pcl is None:
            pcl = self.triplane_decoder.to_channel_last(vit_decode_out['latent_after_vit'])
        N = pcl.shape[0]
        rk = self.rendering_kwargs
        if aabb is not None and not self.grid_ignores_aabb:
            raise NotImplementedError("triplane_decode_grid: a per-object aabb is not supported; the preset's box is used")
        lo, hi = (rk['sampler_bbox_min'], rk['sampler_bbox_max']) if 'sampler_bbox_min' in rk else (-rk['box_warp'] / 2, rk['box_warp'] / 2)
        ax = torch.linspace(lo, hi, grid_size, device=pcl.device)
        pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).reshape(1, -1, 3).expand(N, -1, -1)
        f = self.forward_points(pcl, pts)
        return {k: v.reshape(N, grid_size, grid_size, grid_size, -1) for k, v in f.items()}


class _PosteriorSeams:
    """The quant_conv posterior of the encoder side (vit_triplane.py:912-933, :1152-1199).  The class that inherits it provides
    `superresolution['quant_conv']` (grouped 1 x 1 conv), `ldm_embed_dim` and, as a _cache.PackedWeights, `_side_pack`."""

    def _quant_packed(self, dev):
        qc = self.superresolution['quant_conv']
        return self._side_pack('quant', dev, lambda dev: {'w': f32(qc.weight.reshape(qc.weight.shape[0], -1), dev), 'b': f32(qc.bias, dev)})

    def _posterior(self, h, eps, num_frames):
        if not h.is_cuda:
            raise RuntimeError("ln3diff_amd posterior runs on the HIP device only (no CPU fallback)")
        if h.shape[0] % num_frames:
            raise ValueError(f"posterior input batch {h.shape[0]} is not a multiple of num_frames={num_frames}")
        q = self._quant_packed(h.device)
        B = h.shape[0] // num_frames
        if eps is not None:
            eps = eps.to(h.device, torch.float32).reshape(B, self.ldm_embed_dim, 3, -1).contiguous()
        return ops.mv_posterior(h, q['w'], q['b'], eps, B, num_frames, self.ldm_embed_dim)

    @torch.no_grad()
    def vae_encode(self, h, num_frames=1):
        """h: encoder output [B, 2*3*ldm_z_channels, H, W] -> DiagonalGaussianDistribution(soft_clamp=True) over [B, C, 3, H*W].
        num_frames > 1: h is the per-frame output [B*F, ...] (Encoder.forward_frames) and the frame mean is taken first."""
        r = self._posterior(h, None, num_frames)
        return DiagonalGaussianDistribution(r['mean'], r['logvar'])


class RodinSR_256_fusionv6_ConvQuant_liteSR_dinoInit3DAttn_SD_B_3L_C_withrollout_withSD_D_ditDecoder(_RendererSeams, _PosteriorSeams, _cache.PackedWeights, nn.Module):
    grid_ignores_aabb = True

    def __init__(self, vit_decoder: DiT2, triplane_decoder: Triplane, cls_token=False, normalize_feat=True,
                 sr_ratio=2, vae_p=2, ldm_z_channels=4, ldm_embed_dim=4, token_size=16, **kwargs):
        super().__init__()
        assert not cls_token and vae_p == 2
        self.vit_decoder, self.triplane_decoder = vit_decoder, triplane_decoder
        self.vae_p, self.token_size, self.ldm_embed_dim = vae_p, token_size, ldm_embed_dim
        D = vit_decoder.embed_dim
        self.register_buffer('w_avg', torch.zeros([512]))
        self.superresolution = nn.ModuleDict(dict(
            ldm_upsample=PatchEmbedTriplane(vae_p * token_size, vae_p, 3 * ldm_embed_dim, D),
            quant_conv=nn.Conv2d(2 * 3 * ldm_z_channels, 2 * ldm_embed_dim * 3, kernel_size=1, groups=3),  # encoder side
            conv_sr=Decoder(ch=32, out_ch=32, ch_mult=[1, 2, 2, 4], num_res_blocks=1, z_channels=D)))
        self.rendering_kwargs = triplane_decoder.rendering_kwargs
        self._ws = self._cs = None

    # ------------------------------------------------------------------ packing
    def _pack(self, P, dev):
        sr = self.superresolution
        P['pe_w'], P['pe_b'] = f32(sr['ldm_upsample'].proj.weight, dev), f32(sr['ldm_upsample'].proj.bias, dev)
        d = sr['conv_sr']
        gn = lambda g: pack_gn(g, dev, eps=1e-6)            # the _GN containers carry no eps
        res = lambda b: pack_resblock(b.norm1, b.conv1, b.norm2, b.conv2, dev, shortcut=getattr(b, 'nin_shortcut', None), eps=1e-6)
        P['conv_in'] = pack_conv3(d.conv_in, dev)
        P['mid1'], P['mid2'] = res(d.mid.block_1), res(d.mid.block_2)
        a = d.mid.attn_1
        P['attn'] = {'n': gn(a.norm), 'qkv': pack_lin(torch.cat([a.q.weight, a.k.weight, a.v.weight], 0),
                                                       torch.cat([a.q.bias, a.k.bias, a.v.bias], 0), dev),
                     'proj': pack_lin(a.proj_out.weight, a.proj_out.bias, dev)}
        P['up'] = []
        for lvl in range(d.num_resolutions):
            u = d.up[lvl]
            q = {'blocks': [res(b) for b in u.block]}
            if hasattr(u, 'upsample'):
                q['upsample'] = pack_conv3(u.upsample.conv, dev)
            P['up'].append(q)
        P['norm_out'] = gn(d.norm_out)
        P['conv_out'] = pack_conv3(d.conv_out, dev)
        self._ws = Workspace(dev)
        self._cs = ConvStack(dev, self._ws.get, ws=self._ws)             # scratch by name from the workspace: nothing is allocated after the first decode

    def _attn(self, x, q, N, H, W):
        """mid.attn_1: one head as wide as the block (128 in the released decoder), on the MFMA attention kernels at any token count."""
        C, HW = q['proj']['cout'], H * W
        h = self._cs.gn(x, q['n'], N, HW, C, False)
        o = self_attention_hip(self._ws, 'ca_', h, N, HW, C, 1, q['qkv']['w'], q['qkv']['b'])
        ops.gemm(o, q['proj']['w'], q['proj']['b'], ops.EPI_GATE_RES, x)
        return x

    # ------------------------------------------------------------------ reference-named stages
    @torch.no_grad()
    def vit_decode_backbone(self, latent, img_size=None):
        if isinstance(latent, dict):
            latent = latent['latent_normalized_2Ddiffusion']
        if not latent.is_cuda:
            raise RuntimeError("ln3diff_amd decoder runs on the HIP device only (no CPU fallback)")
        dev = latent.device
        self._ensure_packed(dev)
        B = latent.shape[0]
        D = self.vit_decoder.embed_dim
        S = self.vae_p * self.token_size
        sc = self._ws.get('silu_c', (B * 768, D), torch.bfloat16)
        ops.patch_embed_triplane(latent.contiguous().float(), self._packed['pe_w'], self._packed['pe_b'], sc, None, B,
                                 self.ldm_embed_dim, S, self.vae_p, D)
        tok = self.vit_decoder.forward_tokens(sc, B, self._ws)
        return tok.view(B, 768, D)

    @torch.no_grad()
    def vit_decode_postprocess(self, latent_from_vit, ret_dict: dict, want_nchw=True):
        P, ws, cs = self._packed, self._ws, self._cs
        B, L, D = latent_from_vit.shape
        N, H, W = B * 3, 16, 16
        xb = cs.bf(latent_from_vit.reshape(-1, D), 'tok_bf')
        x = ws.get('dec_x128_256', (N * H * W, 128), torch.float32)
        cs.conv3(xb, N, H, W, P['conv_in'], x)
        x = cs.res(x, P['mid1'], N, H, W)
        x = self._attn(x, P['attn'], N, H, W)
        x = cs.res(x, P['mid2'], N, H, W)
        for lvl in reversed(range(len(P['up']))):
            u = P['up'][lvl]
            for q in u['blocks']:
                x = cs.res(x, q, N, H, W)
            if 'upsample' in u:
                C = u['upsample']['cin']
                xb2 = cs.bf(x, 'up_xb')
                x = ws.get(f'up_x{C}_{H * 2}', (N * H * W * 4, C), torch.float32)
                H, W = cs.conv3(xb2, N, H, W, u['upsample'], x, up=2)
        h = cs.gn(x, P['norm_out'], N, H * W, 32, True)
        planes_cl = torch.empty(B, 3, H, W, 32, device=x.device, dtype=torch.float32)
        cs.conv3(h, N, H, W, P['conv_out'], planes_cl)
        ret_dict.update(dict(cls_token=None, planes_channel_last=planes_cl))
        if want_nchw:
            nchw = torch.empty(B, 96, H, W, device=x.device, dtype=torch.float32)
            ops.planes_to_nchw(planes_cl, nchw, B, 32, H, W)
            ret_dict['latent_after_vit'] = nchw
        return ret_dict

    # ------------------------------------------------------------------ encoder side (the posterior itself: _PosteriorSeams)
    @torch.no_grad()
    def vae_reparameterization(self, latent, sample_posterior, eps=None, num_frames=1):
        """latent: encoder output [B, 24, 32, 32] (any strides with a uniform pixel stride; num_frames > 1: the per-frame output of
        Encoder.forward_frames, pooled inside the same kernel).  sample_posterior: mean + std * eps with eps drawn like the reference,
        torch.randn(mean.shape) on the CPU generator, then moved to the device (or the caller's `eps` [B, C, 3, H*W]); False: the mode."""
        B = latent.shape[0] // num_frames
        HW = latent.shape[2] * latent.shape[3]
        if sample_posterior and eps is None:
            eps = torch.randn(B, self.ldm_embed_dim, 3, HW)
        r = self._posterior(latent, eps if sample_posterior else None, num_frames)
        H, W = latent.shape[2], latent.shape[3]           # token_size * vae_p for the released 256 x 256 input
        return dict(normal_entropy=r['entropy'], latent_normalized=r['latent_tok'],
                    latent_normalized_2Ddiffusion=r['z'].view(B, -1, H, W), log_q_2Ddiffusion=r['log_q'].view(B, -1, H, W),
                    log_q=r['log_q'], posterior=DiagonalGaussianDistribution(r['mean'], r['logvar']))

    @torch.no_grad()
    def vit_decode(self, latent, img_size, sample_posterior=True, eps=None, num_frames=1, **kwargs):
        """vit_triplane.py:879-885: reparameterise (sampling by default), backbone, postprocess."""
        ret_dict = self.vae_reparameterization(latent, sample_posterior, eps=eps, num_frames=num_frames)
        tok = self.vit_decode_backbone(ret_dict, img_size)
        return self.vit_decode_postprocess(tok, ret_dict)


def __getattr__(name):
    """The ShapeNet launchers' decoder class (--ae_classname vit.vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn)
    lives in vit_triplane_shapenet, which imports this module; it is re-exported here lazily.  So is the FFHQ launcher's
    (vit_triplane_ffhq)."""
    if name == 'RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn':
        from . import vit_triplane_shapenet
        return vit_triplane_shapenet.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn
    if name == 'VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_PEinit_2d_sincos_uvit_RodinRollOutConv_4x4_lite_mlp_unshuffle_4XC_final':
        from . import vit_triplane_ffhq
        return getattr(vit_triplane_ffhq, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
