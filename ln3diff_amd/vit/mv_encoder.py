"""Multi-view VAE encoder of the released tri-plane VAE (`mv-sd-dit-dynaInp-trilatent`) on the HIP path: posed views -> the
pre-posterior encoder output that `vae_reparameterization` of the decoder class turns into the tri-plane latent.

Same constructor arguments and state-dict keys as the reference's ldm/modules/diffusionmodules/model.py `Encoder` (:459-561) and
`MVEncoderGSDynamicInp` (:603-623), with ldm/modules/attention.py `SpatialTransformer3D` / `BasicTransformerBlock3D` (:390-463) as
the middle attention (`attn_type="mv-vanilla"`).  Input [B*F, in_channels, S, S]: F = num_frames consecutive views of one object
(the released input has 10 channels: normalised RGB, Pluecker rays o x d | d, normalised depth; datasets/g_buffer_objaverse.py).

Everything runs channel-last on the device; the blocks (3x3 conv as im2col + GEMM, ResnetBlock, the transformer) and their launch
sequences are those of ln3diff_amd/convstack.py.  What is the encoder's own:

  conv_in         the input is cast and zero-padded 10 -> 16 channels by ln3d_nchw_to_cl_bf16
  Downsample      the pad-(0,1,0,1) stride-2 gather (ln3d_im2col3x3_pad01)
  mid.attn_1      attn1 over ALL F*H*W tokens of an object (`(b f) l c -> b (f l) c` is the row order already), attn2 over the same
                  tokens per frame
  pooling         ln3d_frame_mean (forward) or inside ln3d_mv_posterior (AE 'encoder_vae' / 'enc_dec': the decoder's
                  vae_reparameterization reads the per-frame output directly)

There is no CPU fallback.  Not built: attn_resolutions (the released encoder attends in the middle only), resamp_with_conv=False,
temb, the 4-view `MVEncoder` with its fusion_layer and the other dino_versions (they raise).
"""
import torch
import torch.nn as nn

from .. import ops, _cache
from ..convstack import ConvStack, empty_alloc, pack_conv3, pack_gn, pack_resblock, pack_transformer
from ..guided_diffusion.unet import CrossAttention, FeedForward

RELEASED_DINO_VERSION = 'mv-sd-dit-dynaInp-trilatent'


def Normalize(in_channels):     # model.py:29-30
    return nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)


class ResnetBlock(nn.Module):   # model.py:94-153 with temb_channels=0 (the Encoder's)
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=0):
        super().__init__()
        if conv_shortcut or temb_channels:
            raise NotImplementedError("ResnetBlock: conv_shortcut / temb are not used by the encoder")
        out_channels = in_channels if out_channels is None else out_channels
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = Normalize(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.norm2 = Normalize(out_channels)
        self.dropout = nn.Dropout(dropout)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, 1, 1)
        if in_channels != out_channels:
            self.nin_shortcut = nn.Conv2d(in_channels, out_channels, 1, 1, 0)


class Downsample(nn.Module):    # model.py:72-91, with_conv=True
    def __init__(self, in_channels, with_conv=True):
        super().__init__()
        if not with_conv:
            raise NotImplementedError("Downsample(with_conv=False): resamp_with_conv is True in the released encoder")
        self.with_conv = True
        self.conv = nn.Conv2d(in_channels, in_channels, 3, 2, 0)


class BasicTransformerBlock3D(nn.Module):       # attention.py:315-329 (init), :390-402 (forward)
    def __init__(self, dim, n_heads, d_head, dropout=0., context_dim=None, gated_ff=True, checkpoint=True, disable_self_attn=False):
        super().__init__()
        if context_dim is not None or disable_self_attn:
            raise NotImplementedError("BasicTransformerBlock3D: the encoder's blocks are self-attention only (context_dim=None)")
        self.disable_self_attn = False
        self.attn1 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout, glu=gated_ff)
        self.attn2 = CrossAttention(query_dim=dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)


class SpatialTransformer3D(nn.Module):          # attention.py:405-463 (use_linear=False)
    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0., context_dim=None, disable_self_attn=False, use_linear=False,
                 use_checkpoint=True):
        super().__init__()
        if use_linear:
            raise NotImplementedError("SpatialTransformer3D(use_linear=True) is not used by the encoder")
        self.in_channels, self.n_heads, self.d_head = in_channels, n_heads, d_head
        inner = n_heads * d_head
        self.norm = Normalize(in_channels)
        self.proj_in = nn.Conv2d(in_channels, inner, 1, 1, 0)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock3D(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim,
                                                                         disable_self_attn=disable_self_attn) for _ in range(depth)])
        self.proj_out = nn.Conv2d(inner, in_channels, 1, 1, 0)      # zero_module in the reference; loaded weights replace it
        self.use_linear = False


class Encoder(_cache.PackedWeights, nn.Module):
    """ldm Encoder (model.py:459-561) with the multi-view middle attention: forward(x) -> conv_out output [N, 2*z_channels, H/8, W/8]
    (per frame, not pooled).  `forward_frames` returns the same values as a channel-last tensor seen through an NCHW view."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0, resamp_with_conv=True,
                 in_channels, resolution, z_channels, double_z=True, use_linear_attn=False, attn_type="vanilla", attn_kwargs=None,
                 add_fusion_layer=False, num_frames=None, **ignore_kwargs):
        super().__init__()
        if attn_type != "mv-vanilla" or use_linear_attn:
            raise NotImplementedError(f"Encoder(attn_type={attn_type!r}): only the multi-view 'mv-vanilla' middle attention of the released "
                                      f"encoder is built")
        if len(attn_resolutions):
            raise NotImplementedError("Encoder(attn_resolutions != []): the released encoder attends in the middle only")
        if add_fusion_layer:
            raise NotImplementedError("Encoder(add_fusion_layer=True): the 4-view MVEncoder with its fusion layer is not built")
        attn_kwargs = dict(attn_kwargs or {})
        widths = sorted({ch * m for m in (1,) + tuple(ch_mult)})
        for w in widths:
            if w % 32 or 256 % w:          # ln3d_groupnorm_swish: GroupNorm(32) with the channel count dividing 256
                raise ValueError(f"Encoder: channel width {w} (ch x ch_mult) must be one of 32, 64, 128, 256 (GroupNorm(32) kernel)")
        inner = attn_kwargs.get('n_heads', 8) * attn_kwargs.get('d_head', 64)
        if inner % 128 or inner > 1536:
            raise ValueError(f"Encoder: transformer width {inner} - the LayerNorm kernel takes multiples of 128 up to 1536")
        self.ch, self.temb_ch = ch, 0
        self.num_resolutions, self.num_res_blocks = len(ch_mult), num_res_blocks
        self.resolution, self.in_channels = resolution, in_channels
        self.z_channels, self.double_z = z_channels, double_z
        self.num_frames = 1 if num_frames is None else num_frames
        self.conv_in = nn.Conv2d(in_channels, ch, 3, 1, 1)
        in_ch_mult = (1,) + tuple(ch_mult)
        self.in_ch_mult = in_ch_mult
        self.down = nn.ModuleList()
        block_in = ch
        for i_level in range(self.num_resolutions):
            block = nn.ModuleList()
            block_in = ch * in_ch_mult[i_level]
            block_out = ch * ch_mult[i_level]
            for _ in range(num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, dropout=dropout))
                block_in = block_out
            down = nn.Module()
            down.block = block
            down.attn = nn.ModuleList()
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(block_in, resamp_with_conv)
            self.down.append(down)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
        self.mid.attn_1 = SpatialTransformer3D(block_in, **attn_kwargs)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, dropout=dropout)
        self.norm_out = Normalize(block_in)
        self.conv_out = nn.Conv2d(block_in, 2 * z_channels if double_z else z_channels, 3, 1, 1)
        self._cs = None

    # ------------------------------------------------------------------ packing
    def _pack(self, P, dev):
        res = lambda b: pack_resblock(b.norm1, b.conv1, b.norm2, b.conv2, dev, shortcut=getattr(b, 'nin_shortcut', None))
        P['conv_in'] = pack_conv3(self.conv_in, dev, cin_pad=(self.in_channels + 7) // 8 * 8)
        P['down'] = [{'blocks': [res(b) for b in d.block], 'down': pack_conv3(d.downsample.conv, dev) if hasattr(d, 'downsample') else None}
                     for d in self.down]
        P['mid1'], P['mid2'] = res(self.mid.block_1), res(self.mid.block_2)
        P['attn'] = pack_transformer(self.mid.attn_1, False, dev)
        P['norm_out'] = pack_gn(self.norm_out, dev)
        P['conv_out'] = pack_conv3(self.conv_out, dev)
        self._cs = ConvStack(dev, empty_alloc(dev), who='SpatialTransformer3D')

    # ------------------------------------------------------------------ forward
    def _check_input(self, x, F):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"encoder input {tuple(x.shape)}: expected [B*F, {self.in_channels}, H, W]")
        if x.shape[0] % F:
            raise ValueError(f"encoder input batch {x.shape[0]} is not a multiple of num_frames={F} (consecutive frames form one object)")
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"encoder input {x.shape[2]}x{x.shape[3]}: the three Downsamples need sides divisible by 8")
        if not x.is_cuda:
            raise RuntimeError("ln3diff_amd encoder runs on the HIP device only (no CPU fallback)")

    def steps(self):
        """The forward as ordered step names: conv_in, down{l} (the level's ResnetBlocks), down{l}_ds, mid_block_1, mid_attn_1,
        mid_block_2, conv_out (norm_out + swish + conv_out)."""
        names = ['conv_in']
        for lvl, d in enumerate(self.down):
            names.append(f'down{lvl}')
            if hasattr(d, 'downsample'):
                names.append(f'down{lvl}_ds')
        return names + ['mid_block_1', 'mid_attn_1', 'mid_block_2', 'conv_out']

    @torch.no_grad()
    def _run_step(self, name, h, N, H, W):
        """One step of steps() on h [N*H*W, C] f32 channel-last rows (conv_in: the NCHW input itself) -> (h, H, W).  A step without a
        shortcut GEMM adds its residual onto h in place."""
        dev = h.device
        P = self._ensure_packed(dev)
        cs = self._cs
        new = lambda rows, cols, dtype=torch.float32: torch.empty(rows, cols, device=dev, dtype=dtype)
        if name == 'conv_in':
            pc = P['conv_in']
            x_cl = new(N * H * W, pc['cin'], torch.bfloat16)
            ops.nchw_to_cl_bf16(h.contiguous().float(), x_cl, N, h.shape[1], H * W, pc['cin'])
            out = new(N * H * W, pc['cout'])
            cs.conv3(x_cl, N, H, W, pc, out)
            return out, H, W
        if name.startswith('down'):
            d = P['down'][int(name[4:].split('_')[0])]
            if name.endswith('_ds'):                    # Downsample: pad (0,1,0,1), stride 2, padding 0
                a = cs.bf(h)
                out = new(N * ((H - 2) // 2 + 1) * ((W - 2) // 2 + 1), d['down']['cout'])
                H, W = cs.conv3(a, N, H, W, d['down'], out, pad01=True)
                return out, H, W
            for q in d['blocks']:
                h = cs.res(h, q, N, H, W)
            return h, H, W
        if name in ('mid_block_1', 'mid_block_2'):
            return cs.res(h, P['mid1' if name == 'mid_block_1' else 'mid2'], N, H, W), H, W
        if name == 'mid_attn_1':
            att = P['attn']

            def attn2(a, b):                            # within each frame
                o, padded = cs.self_attend(a, b['qkv2'], N, H * W, att['heads'], att['dh'], 'f_')
                return o, b['o2p' if padded else 'o2']
            return cs.transformer(h, att, N, H, W, attn2, frames=self.num_frames), H, W
        if name == 'conv_out':
            a = cs.gn(h, P['norm_out'], N, H * W, h.shape[1], True)
            out = new(N * H * W, P['conv_out']['cout'])
            cs.conv3(a, N, H, W, P['conv_out'], out)
            return out, H, W
        raise KeyError(name)

    @torch.no_grad()
    def forward_frames(self, x, stages=None):
        """x [B*F, in_channels, S, S] -> conv_out per frame as [B*F, 2*z_channels, S/8, S/8] (an NCHW view of channel-last memory).
        stages: optional dict that receives NCHW copies of every stage (level outputs, middle before / after the attention)."""
        self._check_input(x, self.num_frames)
        N, _, H, W = x.shape
        h = x
        for name in self.steps():
            h, H, W = self._run_step(name, h, N, H, W)
            if stages is not None and name != 'conv_out':
                stages[name] = h.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()
        return h.view(N, H, W, -1).permute(0, 3, 1, 2)

    @torch.no_grad()
    def forward(self, x, **kwargs):
        return self.forward_frames(x).contiguous()


class MVEncoderGSDynamicInp(Encoder):
    """model.py:603-623: the Encoder over F = num_frames views per object, then the mean over each object's frames ->
    [B, 2*z_channels, S/8, S/8].  The middle attention always groups self.num_frames frames; the `num_frames` argument of forward
    only changes the pooling (as in the reference)."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0, resamp_with_conv=True, in_channels,
                 resolution, z_channels, double_z=True, use_linear_attn=False, attn_type="mv-vanilla", num_frames, **ignore_kwargs):
        if num_frames <= 4:
            raise ValueError(f"MVEncoderGSDynamicInp: num_frames={num_frames}; the reference asserts num_frames > 4 (model.py:618)")
        super().__init__(ch=ch, out_ch=out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks, attn_resolutions=attn_resolutions,
                         dropout=dropout, resamp_with_conv=resamp_with_conv, in_channels=in_channels, resolution=resolution,
                         z_channels=z_channels, double_z=double_z, use_linear_attn=use_linear_attn, attn_type=attn_type,
                         add_fusion_layer=False, num_frames=num_frames, **ignore_kwargs)

    @torch.no_grad()
    def forward(self, x, num_frames=None):
        F = self.num_frames if num_frames is None else num_frames
        if F <= 4:
            raise ValueError(f"MVEncoderGSDynamicInp: num_frames={F}; the reference asserts num_frames > 4")
        if x.shape[0] % F:
            raise ValueError(f"encoder input batch {x.shape[0]} is not a multiple of num_frames={F}")
        h = self.forward_frames(x)
        N, C, H, W = h.shape
        out = torch.empty(N // F, C, H, W, device=h.device, dtype=torch.float32)
        ops.frame_mean(h, out, N // F, F, H * W, C)
        return out


def create_encoder(dino_version=RELEASED_DINO_VERSION, encoder_in_channels=10, sd_E_ch=64, sd_E_num_res_blocks=1, z_channels=12,
                   num_frames=6, resolution=256, **_):
    """The encoder branch of nsr/script_util.py create_model (:1294-1340) for the released VAE (vae_xl_reconstruction.sh)."""
    if dino_version != RELEASED_DINO_VERSION:
        raise NotImplementedError(f"dino_version {dino_version!r}: only the released multi-view encoder ({RELEASED_DINO_VERSION!r}) is built; "
                                  f"the 4-view MVEncoder with its fusion layer (DiT2-B/2 VAE) and the other encoders are not")
    return MVEncoderGSDynamicInp(double_z=True, resolution=resolution, in_channels=encoder_in_channels, ch=sd_E_ch, ch_mult=[1, 2, 4, 4],
                                 num_res_blocks=sd_E_num_res_blocks, num_frames=num_frames, dropout=0.0, attn_resolutions=[], out_ch=3,
                                 z_channels=z_channels, attn_kwargs={'n_heads': 8, 'd_head': 64})
