"""CPU oracle (TEST INFRASTRUCTURE ONLY) - plain torch restatement of the two DINOv2-based tri-plane VAE decoder classes, stage by
stage.  Never imported by the product.

  'shapenet'  RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn                   latent [B, 12, 32, 32]
  'ffhq'      VAE_LDM_V4_vit3D_v3_conv3D_depth2_xformer_mha_..._4XC_final             latent [B, 12, 16, 16]

Reference citations (relative to the reference checkout):
  the two classes                                vit/vit_triplane.py:802-1121 (ShapeNet), :516-800 (FFHQ)
  forward_vit_decoder (pos_embed, UViT skips)    vit/vit_triplane.py:1076-1118
  unpatchify_triplane / unpatchify3D             vit/vit_triplane.py:393-414 / :888-909
  vae_encode / vae_reparameterization            vit/vit_triplane.py:912-994; utils/torch_utils/distributions/distributions.py:44-88
  cross-plane attention (xygrid)                 vit/vision_transformer.py:442-529
  Conv3DCrossAttentionBlock (+ Nested)           vit/vision_transformer.py:1647-1741
  TriplaneFusionBlockv3 / v4_nested_init_from_dino    vit/vision_transformer.py:1871-1953 / :2062-2142
  roll-out group convolutions                    vit/vision_transformer.py:639-733
  RodinConv3D4X_lite_mlp_as_residual (+ _lite)   vit/vision_transformer.py:1047-1151, :1202-1213
  DINOv2 block (eval mode)                       x + ls1 * attn(norm1(x)); x + ls2 * mlp(norm2(x)), erf-GELU (published layout)

Every function takes `sd`, a state dict with the reference's parameter names, and keeps its dtype: a float64 state dict and float64
inputs run in float64 end to end.  Tokens are [B, 3 * N, D] (plane-major), planes NCHW [B, 3 * C, R, R] with channel = plane * C + c
(`to_cl` gives the product's channel-last [B, 3, R, R, C]).  A batch decodes object by object (the product's documented behaviour: the
reference's batched cross-plane attention re-orders query rows across objects for B > 1): nothing below mixes objects.

Under oracle.dit.operand_rounding(bf16, kernel_arith=True) the functions round where the HIP launches round and nowhere else:
  * every GEMM operand (oracle.dit.linear), q / k / v and the probabilities of the per-plane attention (oracle.dit.sdpa: the streaming /
    ring kernels' softmax), the polynomial erf-GELU of the fc1 epilogue;
  * the cross-plane attention (ln3d_triplane_axis_attention) reads the fp32 q / k / v its projection wrote and accumulates in fp32:
    `axis_attention` rounds NOTHING; its bf16 output is the operand of `proj` and is rounded there;
  * the FFHQ class carries the weights that write the residual stream (attention proj, fc2, the fusion proj, skip_linear) as a bf16
    pair, w = bf16(w) + bf16(w - bf16(w)), in two accumulating launches: `res_linear(..., pair=True)`;
  * the ShapeNet patch embedding is an fp32 kernel and the FFHQ token embedding is exact up to its xl . wl term ([xh | xh | xl] .
    [wh | wl | wh] in the GEMM's K padding): both unrounded;
  * a skip is kept in bf16 (rounded when pushed; skip_linear rounds its operand again, which changes nothing);
  * the up-sampled planes `up` are bf16, and so is short_cut's input; the roll-out convolutions round x, the row means, the column
    means and the weights; the FFHQ class's first convolution pools the bf16 `up` (ln3d_rollout_means_bf16);
  * LayerNorm, pos_embed, unpatchify, the bilinear resize + leaky-ReLU residual and the posterior are fp32: unrounded.
"""
import math

import torch
import torch.nn.functional as F

from .decoder import patch_embed_triplane
from .dit import OPERAND_ROUND, _r, layer_norm, linear, sdpa
from .vit_image import _gelu_erf

VD = 'vit_decoder.'
SR = 'superresolution.'
CS = SR + 'conv_sr.'
CLASSES = ('shapenet', 'ffhq')
SLOPE = 0.01                                     # nn.LeakyReLU()'s default


# ------------------------------------------------------------------------------------------------ layouts
def to_cl(x, planes=3):
    """NCHW [B, 3C, H, W] -> channel-last [B, 3, H, W, C]"""
    B, C3, H, W = x.shape
    return x.reshape(B, planes, C3 // planes, H, W).permute(0, 1, 3, 4, 2)


def to_nchw(x):
    """channel-last [B, 3, H, W, C] -> NCHW [B, 3C, H, W]"""
    B, P, H, W, C = x.shape
    return x.permute(0, 1, 4, 2, 3).reshape(B, P * C, H, W)


def _depth(sd):
    return 1 + max(int(k[len(VD):].split('.')[1]) for k in sd if k.startswith(VD + 'blocks.'))


# ------------------------------------------------------------------------------------------------ GEMMs onto the residual stream
def res_linear(x, w, b=None, pair=False):
    """a projection that writes the residual stream.  pair (the FFHQ class, under operand rounding): the weight is the bf16 pair
    bf16(w) + bf16(w - bf16(w)), the activation a single bf16; otherwise oracle.dit.linear."""
    if pair and OPERAND_ROUND[0] is not None:
        hi = _r(w)
        return F.linear(_r(x), hi + _r(w - hi), b)
    return linear(x, w, b)


# ------------------------------------------------------------------------------------------------ token embedding, pos_embed
def embed_shapenet(sd, latent):
    """PatchEmbedTriplane: latent [B, 12, 32, 32] -> raw tokens [B, 768, D] (an fp32 kernel: no rounding)"""
    return patch_embed_triplane(sd, latent)


def ffhq_tokens(latent):
    """the FFHQ latent re-layout B z 3 L -> B 3 L z: [B, 3z, h, h] -> [B, 3 * h * h, z]"""
    B, C3, h, _ = latent.shape
    return latent.reshape(B, C3 // 3, 3, h * h).permute(0, 2, 3, 1).reshape(B, 3 * h * h, C3 // 3)


def embed_ffhq(sd, latent):
    """the Linear on the re-laid-out latent; exact up to the xl . wl term of the split product: unrounded"""
    tok = ffhq_tokens(latent) if latent.dim() == 4 else latent
    return F.linear(tok, sd[SR + 'ldm_upsample.weight'], sd[SR + 'ldm_upsample.bias'])


def embed(sd, cls, latent):
    return embed_shapenet(sd, latent) if cls == 'shapenet' else embed_ffhq(sd, latent)


def add_pos(sd, x):
    return x + sd[VD + 'pos_embed']


# ------------------------------------------------------------------------------------------------ blocks
def _ln(sd, p, x):
    return layer_norm(x, 1e-6, sd[p + 'weight'], sd[p + 'bias'])


def mlp_half(sd, p, x, pair=False):
    """x + ls2 * fc2(gelu(fc1(norm2(x))))"""
    h = _gelu_erf(linear(_ln(sd, p + 'norm2.', x), sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias']))
    return x + sd[p + 'ls2.gamma'] * res_linear(h, sd[p + 'mlp.fc2.weight'], sd[p + 'mlp.fc2.bias'], pair)


def plane_block(sd, p, x, H, pair=False):
    """the DINOv2 block over each plane's tokens: x [B, 3N, D], attention within a plane"""
    B, L, D = x.shape
    N = L // 3
    xs = x.reshape(B * 3, N, D)
    qkv = linear(_ln(sd, p + 'norm1.', xs), sd[p + 'attn.qkv.weight'], sd[p + 'attn.qkv.bias'])
    q, k, v = (t.reshape(B * 3, N, H, D // H).transpose(1, 2) for t in qkv.chunk(3, -1))
    o = sdpa(q, k, v).transpose(1, 2).reshape(B * 3, N, D)
    xs = xs + sd[p + 'ls1.gamma'] * res_linear(o, sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias'], pair)
    return mlp_half(sd, p, xs, pair).reshape(B, L, D)


def axis_attention(q, k, v):
    """q, k, v [B, 3, p, p, H, Dh] (plane, y, x): the token (i, y, x) attends to row y of plane i + 1 (keys j = 0 .. p-1 along x) and
    to column x of plane i + 2 (keys along y), one softmax over the 2p keys, scale Dh^-0.5.  Nothing is rounded (see the module
    docstring); -> [B, 3, p, p, H, Dh]"""
    p, scale = q.shape[2], q.shape[-1] ** -0.5
    out = []
    for i in range(3):
        kr, vr = k[:, (i + 1) % 3], v[:, (i + 1) % 3]                 # [B, y, j, H, Dh]
        kc, vc = k[:, (i + 2) % 3], v[:, (i + 2) % 3]                 # [B, j, x, H, Dh]
        s = torch.cat([torch.einsum('byxhd,byjhd->byxhj', q[:, i], kr), torch.einsum('byxhd,bjxhd->byxhj', q[:, i], kc)], -1) * scale
        a = torch.softmax(s, -1)
        out.append(torch.einsum('byxhj,byjhd->byxhd', a[..., :p], vr) + torch.einsum('byxhj,bjxhd->byxhd', a[..., p:], vc))
    return torch.stack(out, 1)


def cross_attention(sd, p, x, H, pair=False):
    """Conv3DCrossAttentionBlock without its residual: proj(axis_attention([wq ; w_kv] norm1(x))); p: the block's prefix"""
    B, L, D = x.shape
    g = int(round(math.sqrt(L // 3)))
    assert 3 * g * g == L
    h = _ln(sd, p + 'norm1.', x)
    q = linear(h, sd[p + 'attn.wq.weight'], sd[p + 'attn.wq.bias'])
    k, v = linear(h, sd[p + 'attn.w_kv.weight'], sd[p + 'attn.w_kv.bias']).chunk(2, -1)
    sp = lambda t: t.reshape(B, 3, g, g, H, D // H)
    o = axis_attention(sp(q), sp(k), sp(v)).reshape(B, L, D)
    return res_linear(o, sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias'], pair)


def cross_block(sd, p, x, H):
    """the ShapeNet class's second block of a pair: its `attn` is a whole cross-plane block that returns its input plus the attention,
    x <- x + ls1 * (n + CA(n)), n = norm1(x); then the DINOv2 MLP half"""
    n = _ln(sd, p + 'norm1.', x)
    x = x + sd[p + 'ls1.gamma'] * (n + cross_attention(sd, p + 'attn.', n, H))
    return mlp_half(sd, p, x)


def fusion(sd, p, x, H):
    """the FFHQ class's `fusion` (has_mlp False): x <- x + CA(x)"""
    return x + cross_attention(sd, p, x, H, pair=True)


def group(sd, cls, j, x, H):
    """fusion group j: ShapeNet plane block + nested cross block; FFHQ two plane blocks + fusion"""
    p = f'{VD}blocks.{j}.'
    if cls == 'shapenet':
        return cross_block(sd, p + 'vit_blks.1.', plane_block(sd, p + 'vit_blks.0.', x, H), H)
    x = plane_block(sd, p + 'vit_blks.0.', x, H, pair=True)
    x = plane_block(sd, p + 'vit_blks.1.', x, H, pair=True)
    return fusion(sd, p + 'fusion.', x, H)


def push_skip(x):
    """the long skip as it is kept: bf16 under operand rounding"""
    return _r(x)


def skip_step(sd, cls, j, x, skip):
    """x <- x + skip_linear([x, skip])"""
    w, b = sd[f'{VD}blocks.{j}.skip_linear.weight'], sd[f'{VD}blocks.{j}.skip_linear.bias']
    D = x.shape[-1]
    pair = cls == 'ffhq'
    return x + res_linear(x, w[:, :D], b, pair) + res_linear(skip, w[:, D:], None, pair)


def final_norm(sd, x):
    return _ln(sd, VD + 'norm.', x)


def vit_forward(sd, cls, raw, H, taps=None, pop=lambda skips: skips.pop()):
    """forward_vit_decoder: raw tokens [B, 3N, D] -> + pos_embed -> groups with UViT long skips (popped last in, first out) -> norm.
    taps: name -> (inputs, output) of every stage: 'pos', 'skip{j}', 'group{j}', 'norm'.  pop: how a skip leaves the stack (the tests
    seed a first-in-first-out defect through it)."""
    def tap(name, ins, out):
        if taps is not None:
            taps[name] = (ins, out)
        return out
    depth = _depth(sd)
    x = tap('pos', (raw,), add_pos(sd, raw))
    skips = [push_skip(x)]
    for j in range(depth):
        if j >= depth // 2:
            s = pop(skips)
            x = tap(f'skip{j}', (x, s), skip_step(sd, cls, j, x, s))
        x = tap(f'group{j}', (x,), group(sd, cls, j, x, H))
        if j < depth // 2 - 1:
            skips.append(push_skip(x))
    return tap('norm', (x,), final_norm(sd, x))


# ------------------------------------------------------------------------------------------------ decoder_pred, unpatchify, conv_sr
def decoder_pred(sd, tok):
    return linear(tok, sd['decoder_pred.weight'], sd['decoder_pred.bias'])


def unpatchify_triplane(pred, p=4):
    """[B, 3 * h * h, p * p * C] -> NCHW [B, 3C, h * p, h * p]"""
    B, L, PC = pred.shape
    h = int(round(math.sqrt(L // 3)))
    C = PC // (p * p)
    x = pred.reshape(B, 3, h, h, p, p, C)
    return torch.einsum('ndhwpqc->ndchpwq', x).reshape(B, 3 * C, h * p, h * p)


def short_cut_view(lat):
    """short_cut's input: channels regrouped as (k, e) -> [B, 3 (e), L, C (k)], the value of channel 3k + e"""
    B, C3, h, w = lat.shape
    return lat.reshape(B, C3 // 3, 3, h * w).permute(0, 2, 3, 1)


def short_cut(sd, lat):
    """the residual branch at the low resolution: NCHW [B, 3Cm, r, r] -> NCHW [B, 3Co, r, r]"""
    B, _, h, w = lat.shape
    y = linear(short_cut_view(lat), sd[CS + 'short_cut.weight'], sd[CS + 'short_cut.bias'])         # [B, 3, L, Co]
    return y.permute(0, 1, 3, 2).reshape(B, -1, h, w)


def resize(x, R):
    """bilinear, align_corners False (the reference passes antialias=True, which changes nothing when a side grows)"""
    if x.shape[-1] == R and x.shape[-2] == R:
        return x
    return F.interpolate(x, size=(R, R), mode='bilinear', align_corners=False)


def upsample_t(lat, R):
    """the transposed planes resized to R x R, kept in bf16 (the first convolution's operand)"""
    return _r(resize(lat.permute(0, 1, 3, 2), R))


def rollout(x):
    """RodinRollOutConv3D_GroupConv's input: plane i -> [x_i | row means of plane i + 1 | column means of plane i + 2]: [B, 9C, H, W]"""
    B, C3, H, W = x.shape
    v = x.reshape(B, 3, C3 // 3, H, W)
    parts = []
    for i in range(3):
        rowm = v[:, (i + 1) % 3].mean(-1, keepdim=True).expand(-1, -1, -1, W)
        colm = v[:, (i + 2) % 3].mean(-2, keepdim=True).expand(-1, -1, H, -1)
        parts += [v[:, i], rowm, colm]
    return torch.cat(parts, 1)


def group_conv(sd, p, x):
    """3x3 convolution, groups = 3, zero padding 1; both operands rounded under operand rounding"""
    return F.conv2d(_r(x), _r(sd[p + 'weight']), sd[p + 'bias'], padding=1, groups=3)


def conv0(sd, cls, up):
    """conv3D_0 on the up-sampled planes: in-plane (ShapeNet) or rolled out (FFHQ; the means are those of the bf16 `up`)"""
    if cls == 'shapenet':
        return group_conv(sd, CS + 'conv3D_0.roll_out_inplane_conv.', up)
    return group_conv(sd, CS + 'conv3D_0.roll_out_convs.', rollout(up))


def conv1(sd, x0):
    return group_conv(sd, CS + 'conv3D_1.roll_out_convs.', rollout(x0))


def resize_add_lrelu(base, t, R=None):
    """resize(base) + leaky_relu(t)"""
    return resize(base, t.shape[-1] if R is None else R) + F.leaky_relu(t, SLOPE)


def conv_x0(sd, cls, up, res):
    return resize_add_lrelu(res, conv0(sd, cls, up))


def conv_planes(sd, x0):
    return resize_add_lrelu(x0, conv1(sd, x0))


def postprocess(sd, cls, tok, R, taps=None):
    """vit_decode_postprocess: tokens [B, 3N, D] -> planes NCHW [B, 3Co, R, R].  taps: 'decoder_pred', 'unpatchify', 'short_cut',
    'upsample', 'conv0', 'x0', 'conv1', 'planes' -> (inputs, output)."""
    def tap(name, ins, out):
        if taps is not None:
            taps[name] = (ins, out)
        return out
    pred = tap('decoder_pred', (tok,), decoder_pred(sd, tok))
    lat = tap('unpatchify', (pred,), unpatchify_triplane(pred))
    res = tap('short_cut', (lat,), short_cut(sd, lat))
    up = tap('upsample', (lat,), upsample_t(lat, R))
    t0 = tap('conv0', (up,), conv0(sd, cls, up))
    x0 = tap('x0', (res, t0), resize_add_lrelu(res, t0))
    t1 = tap('conv1', (x0,), conv1(sd, x0))
    return tap('planes', (x0, t1), resize_add_lrelu(x0, t1))


def decode(sd, cls, latent, H, R, taps=None):
    """vit_decode_backbone + vit_decode_postprocess -> (ViT tokens, planes NCHW); taps: every stage, 'embed' first"""
    raw = embed(sd, cls, latent)
    if taps is not None:
        taps['embed'] = ((latent,), raw)
    tok = vit_forward(sd, cls, raw, H, taps)
    return tok, postprocess(sd, cls, tok, R, taps)


# ------------------------------------------------------------------------------------------------ the ShapeNet encoder side
def unpatchify3d(x, p, C):
    """[B, h * h, p * p * 3 * C] -> [B, 3, h * p, h * p, C]"""
    B, L, _ = x.shape
    h = int(round(math.sqrt(L)))
    x = x.reshape(B, h, h, p, p, 3, C)
    return torch.einsum('nhwpqdc->ndhpwqc', x).reshape(B, 3, h * p, h * p, C)


def downsample_moments_input(sd, tokens, p=2):
    """ldm_downsample (a bf16 GEMM) + unpatchify3D + 'B 3 H W C -> B 3C H W': encoder tokens [B, 256, 384] -> [B, 24, 32, 32]"""
    y = linear(tokens, sd[SR + 'ldm_downsample.weight'], sd[SR + 'ldm_downsample.bias'])
    v = unpatchify3d(y, p, y.shape[-1] // (3 * p * p))
    B, _, Hh, Ww, C = v.shape
    return v.permute(0, 1, 4, 2, 3).reshape(B, 3 * C, Hh, Ww)


def posterior(sd, h, eps=None):
    """quant_conv (grouped 1 x 1, fp32) and DiagonalGaussianDistribution(soft_clamp=True) over [B, C, 3, H * W]; eps None: the mode"""
    B, _, Hh, Ww = h.shape
    m = F.conv2d(h, sd[SR + 'quant_conv.weight'], sd[SR + 'quant_conv.bias'], groups=3)
    m = m.reshape(B, m.shape[1] // 3, 3, Hh * Ww)
    mean, logvar = m.chunk(2, dim=1)
    logvar = torch.tanh(logvar / 20.0) * 20.0
    std, var = torch.exp(0.5 * logvar), torch.exp(logvar)
    z = mean if eps is None else mean + std * eps.to(mean.dtype).reshape(mean.shape)
    ns = (z - mean) / var
    c = 0.5 * math.log(2 * math.pi)
    return dict(mean=mean, logvar=logvar, z=z, log_q=-0.5 * ns * ns - c - logvar, entropy=logvar + (c + 0.5),
                latent_tok=z.permute(0, 2, 3, 1).reshape(B, -1, z.shape[1]))


def vae_reparameterization(sd, tokens, eps=None):
    """the ShapeNet class's vae_reparameterization: -> posterior() of the moments input, which is returned as 'h' as well"""
    h = downsample_moments_input(sd, tokens)
    r = posterior(sd, h, eps)
    r['h'] = h
    r['latent_normalized_2Ddiffusion'] = r['z'].reshape(h.shape[0], -1, h.shape[2], h.shape[3])
    return r
