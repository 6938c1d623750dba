"""CPU oracle (TEST INFRASTRUCTURE ONLY) - torch restatement of the multi-view VAE encoder of the released tri-plane VAE
(`mv-sd-dit-dynaInp-trilatent`).  Never imported by the product path.

Reference citations:
  Encoder                 ldm/modules/diffusionmodules/model.py:459-561 (forward :536-561)
  MVEncoderGSDynamicInp   ldm/modules/diffusionmodules/model.py:603-623 (the mean over each object's frames)
  ResnetBlock             ldm/modules/diffusionmodules/model.py:94-153 (GroupNorm eps 1e-6, nin_shortcut): oracle.decoder.resnet_block
  Downsample              ldm/modules/diffusionmodules/model.py:72-91: pad (0, 1, 0, 1), then a stride-2 conv without padding
  SpatialTransformer3D    ldm/modules/attention.py:405-463, BasicTransformerBlock3D :390-402: attn1 over the tokens regrouped
                          `(b f) l c -> b (f l) c`, attn2 and the feed-forward per frame, no context (oracle.unet.spatial_transformer
                          with frames = num_frames; GroupNorm eps 1e-6, LayerNorm eps 1e-5)

cfg: ch, ch_mult, num_res_blocks, in_channels, z_channels, double_z (True), n_heads (8), d_head (64), depth (1), num_frames.
`stages(cfg)` names the forward in order, `run_stage` runs one, `forward` is their composition.

Working precision: every function keeps the dtype of `sd` and the input (the conventions of oracle/dit.py and oracle/unet.py).  It is
built on the convs, norms, linears and attention of the other oracles, so under dit.operand_rounding(bf16, kernel_arith=True) it gives
the kernels' arithmetic - bf16 operands into every conv and linear (the zero-padded input channels of conv_in are exact), the two
attention launches of ConvStack.self_attend by oracle.unet.attn_route, which is asked once with the joint token count (attn1) and once
with the per-frame count (attn2) - with no rounding point of its own."""
import torch.nn.functional as F

from . import decoder as odec
from . import unet as ounet
from .dit import _fp


def stages(cfg):
    n = len(cfg['ch_mult'])
    names = ['conv_in']
    for lvl in range(n):
        names.append(f'down{lvl}')
        if lvl != n - 1:
            names.append(f'down{lvl}_ds')
    return names + ['mid_block_1', 'mid_attn_1', 'mid_block_2', 'conv_out']


def downsample(sd, pre, x):
    return ounet._conv(sd, pre + '.conv', F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)


def transformer(sd, cfg, x, frames=None):
    p = dict(heads=cfg.get('n_heads', 8), depth=cfg.get('depth', 1))
    return ounet.spatial_transformer(sd, 'mid.attn_1', x, None, p, frames=cfg['num_frames'] if frames is None else frames)


def run_stage(sd, cfg, name, x):
    """One stage of stages(cfg) on its input x [B*F, C, H, W] (consecutive frames form an object)."""
    if name == 'conv_in':
        return ounet._conv(sd, 'conv_in', x)
    if name.startswith('down'):
        lvl = int(name[4:].split('_')[0])
        if name.endswith('_ds'):
            return downsample(sd, f'down.{lvl}.downsample', x)
        for ib in range(cfg['num_res_blocks']):
            x = odec.resnet_block(sd, f'down.{lvl}.block.{ib}.', x)
        return x
    if name in ('mid_block_1', 'mid_block_2'):
        return odec.resnet_block(sd, 'mid.block_%s.' % name[-1], x)
    if name == 'mid_attn_1':
        return transformer(sd, cfg, x)
    if name == 'conv_out':
        return ounet._conv(sd, 'conv_out', odec._swish(ounet._gn(sd, 'norm_out', x, 1e-6)))
    raise KeyError(name)


def forward(sd, cfg, x, taps=None):
    """Encoder.forward(x, num_frames=cfg['num_frames']): conv_out per frame [B*F, 2 z_channels, H/8, W/8].  taps: a dict that receives
    name -> (input, output) of every stage."""
    h = _fp(x)
    for name in stages(cfg):
        y = run_stage(sd, cfg, name, h)
        if taps is not None:
            taps[name] = (h, y)
        h = y
    return h


def pooled(sd, cfg, x, num_frames=None):
    """MVEncoderGSDynamicInp.forward: the mean over every `num_frames` consecutive frames (the argument changes the pooling only; the
    attention always groups cfg['num_frames'])."""
    h = forward(sd, cfg, x)
    f = cfg['num_frames'] if num_frames is None else num_frames
    return h.reshape(h.shape[0] // f, f, *h.shape[1:]).mean(1)
