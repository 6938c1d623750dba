#!/usr/bin/env python
"""Bitwise A/B listing for changes to the host side of the conv stack (ln3diff_amd/convstack.py and the three models on it): builds the
Objaverse VAE decoder, the multi-view encoder and the U-Net with the tests' seeded synthetic weights and prints one sha256 line per
output and per distinct packed operand tensor.  Run it on two trees that load the same libln3d_hip.so and diff the listings:

    python tools/conv_stack_ab.py [--tree OTHER_CHECKOUT] > listing.txt

Only the models' public surface and their `_packed` dict are used, so the same file runs against an older checkout (--tree)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout to import ln3diff_amd and tests/ from')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
for p in (os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import ln3diff_amd  # noqa: E402
assert os.path.abspath(ln3diff_amd.__file__).startswith(ROOT + os.sep), (ln3diff_amd.__file__, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def out(case, name, t):
    print(f'{case} {name} {str(t.dtype)[6:]}{list(t.shape)} {sha(t)}')


def tensors(node):
    if isinstance(node, torch.Tensor):
        yield node
    elif isinstance(node, (dict, list, tuple)):
        for v in (node.values() if isinstance(node, dict) else node):
            yield from tensors(v)


def packed(case, P):
    """The packed operands by content: one line per distinct (dtype, shape, sha256) in the dict, sorted.  Key names are left out and
    equal tensors count once, so a renamed key or one copy serving two keys does not show; a changed, missing or new value does."""
    for line in sorted({f'{str(t.dtype)[6:]}{list(t.shape)} {sha(t)}' for t in tensors(P)}):
        print(f'{case} packed {line}')


def decoder():
    from conftest import load_synth
    from ln3diff_amd.synth import synth_input
    from test_decode_gpu import build_decoder
    dec = build_decoder(128, 2, 2)
    load_synth(dec, 0)
    dec = dec.cuda()
    latent = synth_input('latent', (2, 12, 32, 32), 5).cuda()
    for ws in ('cold', 'warm'):            # the second pass runs on the workspace the first one left: overlapping scratch names show here
        tok = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': latent}, 128)
        out(f'decoder/{ws}', 'tokens', tok)
        ret = dec.vit_decode_postprocess(tok, {})
        out(f'decoder/{ws}', 'planes_channel_last', ret['planes_channel_last'])
        out(f'decoder/{ws}', 'latent_after_vit', ret['latent_after_vit'])
    packed('decoder', dec._packed)


def encoder():
    from conftest import load_synth
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.vit.mv_encoder import create_encoder
    enc = create_encoder()
    load_synth(enc, 0)
    enc = enc.cuda()
    x = synth_input('mv_small', (6, 10, 64, 64), 7).cuda()
    st = {}
    out('encoder', 'forward_frames', enc.forward_frames(x, stages=st))
    for k in st:
        out('encoder', 'stage.' + k, st[k])
    out('encoder', 'forward', enc(x))
    packed('encoder', enc._packed)


def unet(tag):
    from conftest import golden, manifest
    from ln3diff_amd.synth import synth_input
    from test_unet_cpu import _product
    from unet_configs import CONFIGS, synth_unet_sd
    cfg = CONFIGS[tag]
    m = _product(cfg)
    m.load_state_dict(synth_unet_sd(manifest(golden('unet_' + tag)), 0), strict=True)
    m = m.cuda()
    C = cfg['in_channels'] * (3 if cfg['roll_out'] else 1)
    t = torch.tensor([10.0, 500.0]).cuda()
    # 2x the golden side: both attention levels on the MFMA kernels; the golden side: one level on each route; / 2 and / 4:
    # ln3d_attention_small at both (the sides stay divisible by the U-Net's total downsample, 2)
    for side in (2 * cfg['image_size'], cfg['image_size'], cfg['image_size'] // 2, cfg['image_size'] // 4):
        x = synth_input('x', (2, C, side, side), 3).cuda()
        ctx = synth_input('c', (2, 77, cfg['context_dim']), 3).cuda() if cfg['use_spatial_transformer'] else None
        out(f'unet/{tag}', f'side{side}', m(x, t, context=ctx))
    packed(f'unet/{tag}', m._packed)


if __name__ == '__main__':
    decoder()
    encoder()
    unet('tiny_st')         # scale-shift ResBlocks, SpatialTransformer against a text context
    unet('tiny_attn')       # `h + emb` ResBlocks, AttentionBlock (head size 32 / 64: the padded projection), roll_out
