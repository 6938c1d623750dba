"""Shared table for tests/test_state_cpu.py and tests/test_state_gpu.py: every class that keeps packed device copies of its weights
(ln3diff_amd/_cache.py), at the suite's tiny sizes, with how to build it, how to make it pack, and the channels that change weights.

A holder is described by
  root()        the module that is built (on the CPU, weights seeded by `reseed(root, 0)`),
  pick(root)    the cache holder inside it (the root itself unless the holder only exists inside a parent: DiT2, Triplane),
  pack(h, dev)  builds every pack the holder keeps for `dev` (_cache.PackedWeights: `_ensure_packed`, plus the side packs chosen per
                holder) and returns them as one tree (dicts / lists / tuples / runner objects),
  child         dotted path, below the holder, of a submodule with parameters (a block, a res-block),
  ckpt          the keyword of checkpoint.load_checkpoint that takes the ROOT.
"""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')      # unet_configs lives beside the goldens
if _GOLDEN not in sys.path:
    sys.path.insert(0, _GOLDEN)

# ----------------------------------------------------------------------------- builders (the suite's tiny configurations, on the CPU)
def _t23d():
    from test_dit_gpu import _build
    return _build(128, 2, 2)


def _i23d():
    from test_i23d_gpu import _build
    return _build(128, 2, 2)


def _pcd():
    from ln3diff_amd.dit.dit_i23d import DiT_pcd_I23D_PixelArt_MVCond
    return DiT_pcd_I23D_PixelArt_MVCond(input_size=32, patch_size=1, in_channels=19, hidden_size=128, depth=2, num_heads=2, num_classes=0,
                                        learn_sigma=False, context_dim=768, roll_out=True, pooling_ctx_dim=768)


def _ae():
    from test_decode_gpu import build_decoder
    return build_decoder(128, 2, 2)


def _shapenet():
    from test_shapenet_decoder_cpu import _build
    return _build(128, 2)


def _ffhq():
    from test_ffhq_decoder_cpu import _build
    return _build(128, 2)


def _encoder():
    from test_encoder_cpu import _encoder
    return _encoder()


def _unet():
    from test_unet_cpu import _product
    from unet_configs import CONFIGS
    return _product(CONFIGS['tiny_st'])


def _triplane():
    from ln3diff_amd.nsr.triplane import Triplane
    return Triplane(img_resolution=16)


def _clip_text():
    from conftest import golden
    from test_clip_gpu import _build
    return _build(golden('clip_text_tiny'))


def _openclip():
    from ln3diff_amd.sgm.image_encoders import FrozenOpenCLIPImageEmbedder
    return FrozenOpenCLIPImageEmbedder(arch='tiny', width=128, mlp_width=512, layers=1, heads=2, image_size=56, patch_size=14, embed_dim=64,
                                       output_tokens=True)


def _dino():
    from ln3diff_amd.sgm.image_encoders import FrozenDinov2ImageEmbedder
    return FrozenDinov2ImageEmbedder(width=128, layers=1, heads=2, image_size=56)


# ----------------------------------------------------------------------------- packing
def _pack_ensure(h, dev):
    return {'packed': h._ensure_packed(dev)}


def _pack_ae(h, dev, quant, down):
    """quant / down: whether this class keeps the posterior's quant_conv operands / the ldm_downsample operands (chosen per holder in
    HOLDERS, not probed: a renamed method must fail here, not drop out of the comparison)"""
    out = {'packed': h._ensure_packed(dev), 'dec': h.triplane_decoder._ensure_packed(dev)}
    if quant:
        out['quant'] = h._quant_packed(dev)
    if down:
        out['down'] = h._down_packed(dev)
    return out


def _pack_ae_dit2(h, dev):
    return dict(_pack_ae(h, dev, True, False), vit=h.vit_decoder._ensure_packed(dev))


class Holder:
    def __init__(self, name, root, pack, child, ckpt, pick=lambda r: r):
        self.name, self.root, self.pack, self.child, self.ckpt, self.pick = name, root, pack, child, ckpt, pick

    def build(self, seed=0):
        root = self.root()
        reseed(root, seed)
        return root, self.pick(root)


HOLDERS = [
    Holder('DiT_TriLatent', _t23d, _pack_ensure, 'blocks.1', 'dit'),
    Holder('DiT_I23D_PixelArt', _i23d, _pack_ensure, 'blocks.1', 'dit'),
    Holder('DiT_pcd_I23D_PixelArt_MVCond', _pcd, _pack_ensure, 'blocks.0', 'dit'),
    Holder('DiT2', _ae, _pack_ensure, 'blocks.1', 'decoder', pick=lambda r: r.vit_decoder),
    Holder('AE_decoder', _ae, _pack_ae_dit2, 'superresolution.conv_sr.mid.block_1', 'decoder'),
    Holder('ShapeNet_decoder', _shapenet, lambda h, dev: _pack_ae(h, dev, True, True), 'vit_decoder.blocks.0', 'decoder'),
    Holder('FFHQ_decoder', _ffhq, lambda h, dev: _pack_ae(h, dev, False, False),      # its encoder side is not built
            'vit_decoder.blocks.0', 'decoder'),
    Holder('mv_Encoder', _encoder, _pack_ensure, 'mid.block_1', 'encoder'),
    Holder('UNetModel', _unet, _pack_ensure, 'input_blocks.1', 'dit'),
    Holder('Triplane', _ae, _pack_ensure, 'decoder.net', 'decoder', pick=lambda r: r.triplane_decoder),
    Holder('FrozenCLIPEmbedder', _clip_text, _pack_ensure, 'transformer.text_model.encoder.layers.0', 'conditioner'),
    Holder('FrozenOpenCLIPImageEmbedder', _openclip, _pack_ensure, 'model.visual.transformer.resblocks.0', 'conditioner'),
    Holder('FrozenDinov2ImageEmbedder', _dino, _pack_ensure, 'model.blocks.0', 'conditioner'),
]
BY_NAME = {h.name: h for h in HOLDERS}


# ----------------------------------------------------------------------------- weights
def new_values(sd, seed):
    """{key: tensor} like `sd` with every floating-point entry redrawn (CPU generator, the entry's own spread); computed positional
    embeddings and integer buffers are kept."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    for k, v in sd.items():
        if 'pos_embed' in k or not v.dtype.is_floating_point or v.numel() == 0:
            out[k] = v.detach().clone()
            continue
        r = torch.randn(v.shape, generator=g)
        if v.dim() == 1:
            out[k] = (r * 0.05 + (1.0 if k.endswith('weight') else 0.0)).to(v.dtype)
        else:
            fan = max(1, v[0].numel())
            out[k] = (r * (0.7 / fan ** 0.5)).to(v.dtype)
    return out


def reseed(module, seed):
    module.load_state_dict(new_values(module.state_dict(), seed), strict=True)
    return module


def edit_in_place(module):
    """the bare in-place write that no hook sees: every parameter scaled and shifted under no_grad"""
    with torch.no_grad():
        for p in module.parameters():
            if p.dtype.is_floating_point:
                p.mul_(1.25).add_(0.015625)


# ----------------------------------------------------------------------------- walking what a holder keeps
def leaves(tree, path='', seen=None):
    """(path, leaf) of every tensor and plain value reachable from a pack: dicts, lists, tuples and the attribute dicts of plain objects
    (ops.MX operands, the image embedders' runner); scratch (Workspace), modules and the epoch stamp are not weights and are skipped."""
    from ln3diff_amd.dit.dit_models_xformers import Workspace
    seen = set() if seen is None else seen
    if torch.is_tensor(tree):
        yield path, tree
    elif isinstance(tree, dict):
        for k in sorted(tree, key=str):
            if k != 'epoch':
                yield from leaves(tree[k], f'{path}/{k}', seen)
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from leaves(v, f'{path}/{i}', seen)
    elif isinstance(tree, (Workspace, nn.Module)):
        return
    elif hasattr(tree, '__dict__') and id(tree) not in seen:
        seen.add(id(tree))
        yield from leaves(vars(tree), path, seen)
    else:
        yield path, tree


def snapshot(tree):
    """deep copy of the leaves: {path: tensor clone or value}"""
    return {p: (v.detach().clone() if torch.is_tensor(v) else copy.copy(v)) for p, v in leaves(tree)}


def same(a, b):
    """a, b: snapshots.  Returns the list of paths that differ (missing on one side counts)."""
    bad = [p for p in set(a) ^ set(b)]
    for p in set(a) & set(b):
        x, y = a[p], b[p]
        if torch.is_tensor(x) != torch.is_tensor(y):
            bad.append(p)
        elif torch.is_tensor(x):
            if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x, y):
                bad.append(p)
        elif callable(x) or callable(y):
            continue
        elif x != y:
            bad.append(p)
    return sorted(bad)


# ----------------------------------------------------------------------------- channels: everything that may change weights
def _world1_group(tmp):
    """a one-rank gloo process group in this process (what a launcher-started single rank has), for parallel.broadcast_flat"""
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='file://' + os.path.join(str(tmp), 'pg'), rank=0, world_size=1)
        return True
    return False


def ch_load_holder(root, h, spec, tmp):
    h.load_state_dict(new_values(h.state_dict(), 11), strict=True)


def ch_load_strict_error(root, h, spec, tmp):
    """a strict load that ends in RuntimeError (one key missing): the tensors that matched were copied before it raised"""
    sd = new_values(h.state_dict(), 17)
    sd.popitem()
    with pytest.raises(RuntimeError, match='Missing key'):
        h.load_state_dict(sd, strict=True)


def ch_load_parent(root, h, spec, tmp):
    parent = nn.ModuleDict({'inner': root})
    parent.load_state_dict({'inner.' + k: v for k, v in new_values(root.state_dict(), 12).items()}, strict=True)


def ch_load_child(root, h, spec, tmp):
    c = h.get_submodule(spec.child)
    c.load_state_dict(new_values(c.state_dict(), 13), strict=True)


def ch_apply(root, h, spec, tmp):
    edit_in_place(h)                      # alone this needs invalidate_weight_caches(); the _apply that follows must re-pack
    h.float()


def ch_fill_random(root, h, spec, tmp):
    from ln3diff_amd.synth import fill_module_random_
    fill_module_random_(h, 14)


def ch_checkpoint(root, h, spec, tmp):
    from ln3diff_amd.checkpoint import load_checkpoint
    f = os.path.join(str(tmp), 'ck.pt')
    prefix = 'encoder.' if spec.ckpt == 'encoder' else ''         # the encoder is looked up under its checkpoint prefixes only
    torch.save({prefix + k: v.cpu() for k, v in new_values(root.state_dict(), 15).items()}, f)
    load_checkpoint(f, **{spec.ckpt: root})


def ch_broadcast(root, h, spec, tmp):
    import torch.distributed as dist
    from ln3diff_amd import parallel
    mine = _world1_group(tmp)
    try:
        edit_in_place(h)
        parallel.broadcast_flat([p.data for p in h.parameters()] + list(h.buffers()), src=0)
    finally:
        if mine:
            dist.destroy_process_group()


def ch_invalidate(root, h, spec, tmp):
    import ln3diff_amd
    edit_in_place(h)
    ln3diff_amd.invalidate_weight_caches()


def ch_replace_child(root, h, spec, tmp):
    """a submodule replaced after the caches were built: no hook sees the new module, the caller invalidates"""
    import ln3diff_amd
    parent_path, _, leaf = spec.child.rpartition('.')
    parent = h.get_submodule(parent_path) if parent_path else h
    new = copy.deepcopy(getattr(parent, leaf))
    for sub in new.modules():             # a module built elsewhere carries none of the holder's hooks
        sub.__dict__.pop('_ln3d_watched', None)
        sub._load_state_dict_post_hooks.clear()
    new.load_state_dict(new_values(new.state_dict(), 16), strict=True)
    setattr(parent, leaf, new)
    ln3diff_amd.invalidate_weight_caches()


CHANNELS = {'load_state_dict': ch_load_holder, 'load_strict_error': ch_load_strict_error, 'load_parent': ch_load_parent,
            'load_child': ch_load_child, 'apply': ch_apply, 'fill_module_random_': ch_fill_random, 'load_checkpoint': ch_checkpoint,
            'broadcast_flat': ch_broadcast, 'invalidate_weight_caches': ch_invalidate, 'replace_submodule': ch_replace_child}


def fresh_like(spec, root, dev=None):
    """the reference of every state test: a new instance, built from scratch, holding root's current weights"""
    r2 = spec.root()
    r2.load_state_dict({k: v.detach().cpu().clone() for k, v in root.state_dict().items()}, strict=True)
    if dev is not None:
        r2 = r2.to(dev)
    return r2, spec.pick(r2)
