"""CPU oracle (TEST INFRASTRUCTURE ONLY) - torch restatement of the U-Net denoiser behind the ShapeNet / FFHQ entry point
(scripts/vit_triplane_diffusion_sample.py).  Never imported by the product path.

Reference citations:
  UNetModel               guided_diffusion/unet.py:427-791 (constructor wiring :553-726, forward :752-791)
  ResBlock                guided_diffusion/unet.py:164-278 (use_scale_shift_norm branch :267-271)
  Downsample / Upsample   guided_diffusion/unet.py:102-161
  AttentionBlock          guided_diffusion/unet.py:281-336, QKVAttentionLegacy :359-389 (the non-transformer variant)
  SpatialTransformer      ldm/modules/attention_compat.py:228-277 (GroupNorm eps 1e-6, 1x1 proj_in / proj_out)
  BasicTransformerBlock   ldm/modules/attention_compat.py:205-225, CrossAttention :161-202, FeedForward / GEGLU :45-82
  timestep_embedding      guided_diffusion/nn.py:103-121, normalization = GroupNorm32(32, C) (eps 1e-5) :93-100
  mixed prediction        guided_diffusion/gaussian_diffusion.py:327-348, :548-558; continuous_diffusion_utils.py:748-754

`layout(cfg)` replays the constructor's wiring and returns, per block of input_blocks / middle_block / output_blocks, the list of
layer kinds - the same walk the product's ln3diff_amd.guided_diffusion.unet does.  `blocks(cfg)` names them in forward order (with the
head), `run_block` runs one, and `unet_forward` is their composition.

Working precision: every function keeps the dtype of `sd` and the inputs (the conventions of oracle/dit.py): fp32 in, the arithmetic is
what it always was; a float64 state dict and float64 inputs run in float64 end to end.  Under dit.operand_rounding(bf16) every conv
and linear takes bf16 operands (the GroupNorm / LayerNorm output, the cast of x in front of a shortcut GEMM, of the tokens in front of
proj_out, of the context), residual and bias stay in the accumulator's precision (the GEMM epilogue).  With kernel_arith=True the two
attention launches of ln3diff_amd/convstack.py ConvStack.self_attend are restated where they round (see `attend`)."""
import math

import torch
import torch.nn.functional as F

from . import dit as odit
from .dit import _fp, _r, linear

# ConvStack.self_attend (restated; tests/test_unet_pixels_cpu.py holds these to ln3diff_amd.convstack and csrc/kernel_plan.h)
MFMA_MIN_TOKENS = 256


def default_channel_mult(image_size):
    """guided_diffusion/script_util.py:292-317"""
    return {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4), 32: (1, 2, 4, 4),
            16: (1, 2, 3, 4)}[image_size]


def layout(cfg):
    """cfg: image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions (ds values), channel_mult,
    num_heads, num_head_channels (-1), num_heads_upsample (-1: num_heads), use_spatial_transformer, transformer_depth, context_dim,
    legacy (True), resblock_updown (False).
    Returns (input_blocks, middle_block, output_blocks): lists of blocks, a block = list of (kind, params).
    The head arithmetic is the reference constructor's, statement by statement (unet.py:570-590, :619-645, :671-692): num_heads is
    REASSIGNED to ch // num_head_channels when that is given; an AttentionBlock gets (num_heads - in the output blocks
    num_heads_upsample -, num_head_channels=dim_head) and takes channels // dim_head heads unless dim_head is -1 (:299-305); a
    SpatialTransformer gets (num_heads, dim_head) everywhere."""
    mc, nrb, cm = cfg['model_channels'], cfg['num_res_blocks'], cfg['channel_mult']
    nh, nhc = cfg.get('num_heads', -1), cfg.get('num_head_channels', -1)
    nhu = cfg.get('num_heads_upsample', -1)
    if nhu == -1:
        nhu = nh
    st, legacy = cfg['use_spatial_transformer'], cfg.get('legacy', True)
    assert not cfg.get('resblock_updown', False)

    def attn(ch, upsample=False):
        nonlocal nh
        if nhc == -1:
            dim_head = ch // nh
        else:
            nh = ch // nhc
            dim_head = nhc
        if legacy:
            dim_head = ch // nh if st else nhc
        if st:
            return ('transformer', dict(ch=ch, heads=nh, dim_head=dim_head, depth=cfg.get('transformer_depth', 1),
                                        context_dim=cfg['context_dim']))
        heads = nhu if upsample else nh
        return ('attention', dict(ch=ch, heads=heads if dim_head == -1 else ch // dim_head))

    inp = [[('conv', dict(cin=cfg['in_channels'], cout=mc))]]
    chans = [mc]
    ch, ds = mc, 1
    for level, mult in enumerate(cm):
        for _ in range(nrb):
            layers = [('res', dict(cin=ch, cout=int(mult * mc)))]
            ch = int(mult * mc)
            if ds in cfg['attention_resolutions']:
                layers.append(attn(ch))
            inp.append(layers)
            chans.append(ch)
        if level != len(cm) - 1:
            inp.append([('down', dict(ch=ch))])
            chans.append(ch)
            ds *= 2
    mid = [('res', dict(cin=ch, cout=ch)), attn(ch), ('res', dict(cin=ch, cout=ch))]
    out = []
    for level, mult in list(enumerate(cm))[::-1]:
        for i in range(nrb + 1):
            ich = chans.pop()
            layers = [('res', dict(cin=ch + ich, cout=int(mc * mult)))]
            ch = int(mc * mult)
            if ds in cfg['attention_resolutions']:
                layers.append(attn(ch, upsample=True))
            if level and i == nrb:
                layers.append(('up', dict(ch=ch)))
                ds //= 2
            out.append(layers)
    return inp, mid, out


def blocks(cfg):
    """The network in forward order: [(name, layers)] - 'input_blocks.0' (the stem conv), every 'input_blocks.i', 'middle_block',
    every 'output_blocks.i' and 'out' (out.0 GroupNorm + SiLU + out.2 conv).  The wiring between them is unet_forward's: the output of
    every input block is pushed, every output block's input is cat([h, pop()], channels)."""
    inp, mid, out = layout(cfg)
    return ([(f'input_blocks.{i}', l) for i, l in enumerate(inp)] + [('middle_block', mid)] +
            [(f'output_blocks.{i}', l) for i, l in enumerate(out)] + [('out', [('head', dict(ch=cfg['model_channels']))])])


def timestep_embedding(t, dim, max_period=10000, dtype=torch.float32):
    """The frequency table and the argument t * freq are fp32 by definition (reference and HIP kernel alike, see dit.timestep_embedding):
    in float64 mode too the fp32 argument is what enters cos / sin."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half)
    args = (t[:, None].float() * freqs[None]).to(dtype)
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def time_embed(sd, cfg, timesteps):
    """time_embed(timestep_embedding(t)) [B, 4 model_channels].  Under operand rounding: bf16 sin / cos of the fp32 argument
    (timestep_embedding_kernel) -> GEMM + SiLU stored bf16 (LN3D_EPI_SILU) -> GEMM, emb in the accumulator's precision; SiLU(emb) is
    rounded where the ResBlocks' emb Linear takes it (LN3D_EPI_F32_SILU stores it in bf16)."""
    emb = timestep_embedding(timesteps, cfg['model_channels'], dtype=sd['time_embed.0.weight'].dtype)
    return linear(F.silu(linear(emb, sd['time_embed.0.weight'], sd['time_embed.0.bias'])), sd['time_embed.2.weight'], sd['time_embed.2.bias'])


def _gn(sd, pre, x, eps):
    return F.group_norm(x, 32, sd[pre + '.weight'], sd[pre + '.bias'], eps)


def _conv(sd, pre, x, stride=1, padding=1):
    # under dit.operand_rounding(): bf16 activations / weights into an fp32-accumulating product, like the im2col + MFMA GEMM
    return F.conv2d(_r(x), _r(sd[pre + '.weight']), sd[pre + '.bias'], stride=stride, padding=padding)


def res_block(sd, pre, x, emb, scale_shift):
    h = _conv(sd, pre + '.in_layers.2', F.silu(_gn(sd, pre + '.in_layers.0', x, 1e-5)))
    e = linear(F.silu(emb), sd[pre + '.emb_layers.1.weight'], sd[pre + '.emb_layers.1.bias'])[:, :, None, None]
    if scale_shift:
        scale, shift = torch.chunk(e, 2, dim=1)
        h = _gn(sd, pre + '.out_layers.0', h, 1e-5) * (1 + scale) + shift
        h = _conv(sd, pre + '.out_layers.3', F.silu(h))
    else:
        h = _conv(sd, pre + '.out_layers.3', F.silu(_gn(sd, pre + '.out_layers.0', h + e, 1e-5)))
    skip = x if (pre + '.skip_connection.weight') not in sd else _conv(sd, pre + '.skip_connection', x, padding=0)
    return skip + h


# ------------------------------------------------------------------------------------------------ attention
def head_pad(dh):
    """the width a head is stored at for the MFMA kernels (dit_models_xformers.attn_head_pad): zero-padded to 64 / 80 / 128"""
    return 64 if dh <= 64 else (80 if dh <= 80 else 128)


def attn_route(dh, L, self_attention=True):
    """The launch ConvStack.self_attend makes for L tokens at head size dh, as this restatement ASSUMES it: 'small'
    (ln3d_attention_small: cross-attention always; head sizes that are no multiple of 8 or above 128; fewer than MFMA_MIN_TOKENS tokens
    or a token count that is no multiple of 32), else the MFMA kernel ln3d_plan_attention chooses for heads zero-padded to head_pad(dh)
    and keys padded to a multiple of 64: 'stream' (64 wide, a multiple of 256 keys - the K-resident kernel, a head for every CU, is
    not restated and must not be what runs), 'ring64', 'ring80', 'ring128'."""
    if not (self_attention and dh % 8 == 0 and dh <= 128 and L >= MFMA_MIN_TOKENS and L % 32 == 0):
        return 'small'
    dp = head_pad(dh)
    if dp == 64:
        return 'stream' if L % 256 == 0 else 'ring64'
    return 'ring%d' % dp


def attend(q, k, v, self_attention=True):
    """softmax(q k^T / sqrt(dh)) v for q, k, v [B, H, N, dh].  Under operand_rounding(kernel_arith=True), by attn_route:
      small  attn_small_kernel (csrc/unet_ops.hip): q / k / v stored in bf16 by their projections, the scale applied to the fp32
             scores, the probabilities NOT rounded, the output rounded to bf16 (by the projection that takes it);
      MFMA   dit._sdpa_kernel on heads zero-padded to head_pad(dh) - the padded width chooses the kernel (64 wide over a multiple of
             256 keys: the streaming kernel), the true one is the scale's (self_attention_hip: scale=Dh ** -0.5, head_dim_pad=Dp)."""
    dh, L = q.shape[-1], k.shape[-2]
    if odit.OPERAND_ROUND[0] is None or not odit.KERNEL_ARITH[0]:
        return odit.sdpa(q, k, v)
    if attn_route(dh, L, self_attention) == 'small':
        s = (_r(q) @ _r(k).transpose(-1, -2)) * dh ** -0.5
        return torch.softmax(s, dim=-1) @ _r(v)
    pad = head_pad(dh) - dh
    return odit._sdpa_kernel(F.pad(q, (0, pad)), F.pad(k, (0, pad)), F.pad(v, (0, pad)), False, dh_true=dh)[..., :dh]


def cross_attention(sd, pre, x, context, heads):
    """CrossAttention.forward: x [B,N,D], context [B,L,Dc] or None (self-attention)."""
    ctx = x if context is None else context
    q = linear(x, sd[pre + '.to_q.weight'])
    k = linear(ctx, sd[pre + '.to_k.weight'])
    v = linear(ctx, sd[pre + '.to_v.weight'])
    B, N, inner = q.shape
    dh = inner // heads
    sp = lambda t: t.reshape(B, -1, heads, dh).permute(0, 2, 1, 3)
    if odit.OPERAND_ROUND[0] is None:
        sim = torch.einsum('bhid,bhjd->bhij', sp(q), sp(k)) * dh ** -0.5
        o = torch.einsum('bhij,bhjd->bhid', sim.softmax(-1), sp(v))
    else:
        o = attend(sp(q), sp(k), sp(v), context is None)
    return linear(o.permute(0, 2, 1, 3).reshape(B, N, inner), sd[pre + '.to_out.0.weight'], sd[pre + '.to_out.0.bias'])


def spatial_transformer(sd, pre, x, context, p, frames=1):
    """frames: attn1 attends jointly over `frames` consecutive images ('(b f) l c -> b (f l) c': SpatialTransformer3D of the multi-view
    VAE encoder, ldm/modules/attention.py:390-463); attn2 and the feed-forward stay per image."""
    B, C, H, W = x.shape
    h = _conv(sd, pre + '.proj_in', _gn(sd, pre + '.norm', x, 1e-6), padding=0)
    h = h.permute(0, 2, 3, 1).reshape(B, H * W, -1)
    D = h.shape[-1]
    for d in range(p['depth']):
        b = f'{pre}.transformer_blocks.{d}'
        ln = lambda n, t: F.layer_norm(t, (D,), sd[f'{b}.{n}.weight'], sd[f'{b}.{n}.bias'], 1e-5)
        joint = h.reshape(B // frames, frames * H * W, D)
        h = (cross_attention(sd, b + '.attn1', ln('norm1', joint), None, p['heads']) + joint).reshape(B, H * W, D)
        h = cross_attention(sd, b + '.attn2', ln('norm2', h), context, p['heads']) + h
        g = linear(ln('norm3', h), sd[b + '.ff.net.0.proj.weight'], sd[b + '.ff.net.0.proj.bias'])
        a, gate = g.chunk(2, dim=-1)
        # geglu_kernel (csrc/unet_ops.hip) evaluates 0.5 g (1 + erff(g / sqrt 2)) in fp32 with the library erf: to fp32 accuracy
        h = linear(a * F.gelu(gate), sd[b + '.ff.net.2.weight'], sd[b + '.ff.net.2.bias']) + h
    h = h.reshape(B, H, W, D).permute(0, 3, 1, 2)
    return _conv(sd, pre + '.proj_out', h, padding=0) + x


def attention_block(sd, pre, x, p):
    """AttentionBlock + QKVAttentionLegacy (heads split before q / k / v)."""
    B, C, H, W = x.shape
    xf = x.reshape(B, C, -1)
    qkv = F.conv1d(_r(F.group_norm(xf, 32, sd[pre + '.norm.weight'], sd[pre + '.norm.bias'], 1e-5)), _r(sd[pre + '.qkv.weight']),
                   sd[pre + '.qkv.bias'])
    nh = p['heads']
    ch = C // nh
    q, k, v = qkv.reshape(B * nh, ch * 3, -1).split(ch, dim=1)
    if odit.OPERAND_ROUND[0] is None:
        s = 1 / math.sqrt(math.sqrt(ch))
        w = torch.einsum('bct,bcs->bts', q * s, k * s).softmax(-1)
        a = torch.einsum('bts,bcs->bct', w, v).reshape(B, -1, H * W)
    else:                       # the product scales the scores by ch ** -0.5 once (the same number, rounded elsewhere)
        hd = lambda t: t.reshape(B, nh, ch, -1).transpose(-1, -2)
        a = attend(hd(q), hd(k), hd(v)).transpose(-1, -2).reshape(B, -1, H * W)
    return (xf + F.conv1d(_r(a), _r(sd[pre + '.proj_out.weight']), sd[pre + '.proj_out.bias'])).reshape(B, C, H, W)


# ------------------------------------------------------------------------------------------------ blocks and the forward
def upsample2x(h):
    return F.interpolate(h, scale_factor=2, mode='nearest')


def run_layers(sd, prefix, layers, h, emb, context, scale_shift, first=0):
    """layers [(kind, params)] with the parameters of layer li under f'{prefix}.{first + li}'"""
    for li, (kind, p) in enumerate(layers):
        pre = f'{prefix}.{first + li}'
        if kind == 'conv':
            h = _conv(sd, pre, h)
        elif kind == 'res':
            h = res_block(sd, pre, h, emb, scale_shift)
        elif kind == 'transformer':
            h = spatial_transformer(sd, pre, h, context, p)
        elif kind == 'attention':
            h = attention_block(sd, pre, h, p)
        elif kind == 'down':
            h = _conv(sd, pre + '.op', h, stride=2)
        elif kind == 'up':
            h = _conv(sd, pre + '.conv', upsample2x(h))
        elif kind == 'head':
            return _conv(sd, 'out.2', F.silu(_gn(sd, 'out.0', h, 1e-5)))
        else:
            raise KeyError(kind)
    return h


def run_block(sd, cfg, name, h, emb, context):
    """One block of blocks(cfg) on its input h [B, C, H, W] (an output block's: the concatenation; roll_out: the rolled-out layout),
    with the time embedding emb [B, 4 model_channels] and the context."""
    layers = dict(blocks(cfg))[name]
    return run_layers(sd, name, layers, h, emb, context, cfg.get('use_scale_shift_norm', True))


def roll(x):
    """'b (n c) h w -> b c h (n w)', n = 3 (unet.py:775-776)"""
    B, C3, H, W = x.shape
    return x.reshape(B, 3, C3 // 3, H, W).permute(0, 2, 3, 1, 4).reshape(B, C3 // 3, H, 3 * W)


def unroll(h):
    """'b c h (n w) -> b (n c) h w'"""
    B, C, H, W3 = h.shape
    return h.reshape(B, C, H, 3, W3 // 3).permute(0, 3, 1, 2, 4).reshape(B, 3 * C, H, W3 // 3)


def unet_forward(sd, cfg, x, timesteps, context=None, taps=None):
    """UNetModel.forward.  x [B, C, S, S] (roll_out: [B, 3C, S, S] re-laid as [B, C, S, 3S] like :775-776).  taps: a dict that
    receives name -> (input, output) of every block of blocks(cfg) (an output block's input is the concatenation) and
    'time_embed' -> (timesteps, emb)."""
    if isinstance(context, dict):
        context = context['crossattn']
    emb = time_embed(sd, cfg, timesteps)
    if taps is not None:
        taps['time_embed'] = (timesteps, emb)
    h = _fp(x)
    if cfg.get('roll_out', False):
        h = roll(h)
    hs = []
    for name, _ in blocks(cfg):
        if name.startswith('output_blocks'):
            h = torch.cat([h, hs.pop()], dim=1)
        y = run_block(sd, cfg, name, h, emb, context)
        if taps is not None:
            taps[name] = (h, y)
        if name.startswith('input_blocks'):
            hs.append(y)
        h = y
    return unroll(h) if cfg.get('roll_out', False) else h


def mixed_prediction(eps, x, mixing_logit, sqrt_one_minus_ab):
    """get_mixed_prediction on an eps model (gaussian_diffusion.py:336-348): (1 - s) * sqrt(1 - ab_t) * x_t + s * eps, s = sigmoid(logit)."""
    c = torch.sigmoid(mixing_logit)
    return (1 - c) * (sqrt_one_minus_ab * x) + c * eps
