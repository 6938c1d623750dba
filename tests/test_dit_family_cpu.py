"""The class tree of the DiT denoiser family, without a GPU: state-dict manifests, registries, surface and ancestry.

tests/golden/dit_family_manifest.json is a recorded result of this project's own code (written by `python
tests/test_dit_family_cpu.py --dump` on the commit in front of the one-base refactor): for each of the eight classes, at the
constructor arguments of dit_token_refs.T23D_SIZES / I23D_NETS, the ordered (key, shape) list of state_dict() and the sha256 of
pos_embed; for every key of both registries, the name of the class it builds.  Order is part of the contract: synth.fill_module_random_
draws from one generator in key order, so a module registered earlier or later changes every benchmark weight.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

import dit_token_refs as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dit_family_manifest.json')
NETS = [('t23d', s) for s in R.T23D_SIZES] + [('i23d', n) for n in R.I23D_NETS]
# what the launchers and bench.py hand to a registry factory
REGISTRY_KW = {'t23d': dict(input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=768, roll_out=True),
               'i23d': dict(input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=1024, roll_out=True, pooling_ctx_dim=768)}


def _build(kind, net):
    return R.build_t23d(net) if kind == 't23d' else R.build_i23d(net)


def _manifest(m):
    sd = m.state_dict()
    out = {'class': type(m).__name__, 'keys': [[k, list(v.shape)] for k, v in sd.items()]}
    if 'pos_embed' in sd:
        out['pos_embed_sha256'] = hashlib.sha256(sd['pos_embed'].contiguous().numpy().tobytes()).hexdigest()
    return out


def _registries():
    from ln3diff_amd.dit import dit_i23d, dit_trilatent
    return {'t23d': dit_trilatent.DiT_models, 'i23d': dit_i23d.DiT_models}


def _registry_instance(kind, key):
    kw = dict(REGISTRY_KW[kind])
    if kind == 't23d' and 'PixelArt' not in key:
        from ln3diff_amd.dit.dit_models_xformers import TextCondDiTBlock
        kw['vit_blk'] = TextCondDiTBlock
    with torch.device('meta'):                           # no full-size weights are allocated
        return _registries()[kind][key](**kw)


def _record():
    rec = {'nets': {f'{kind}-{net}': _manifest(_build(kind, net)) for kind, net in NETS}, 'registry': {}}
    for kind, reg in _registries().items():
        for key in reg:
            m = _registry_instance(kind, key)
            rec['registry'][f'{kind}:{key}'] = {'class': type(m).__name__, 'depth': m.depth, 'hidden_size': m.embed_dim,
                                                'num_heads': m.num_heads, 'patch_size': m.patch_size,
                                                'keys': len(m.state_dict())}
    return rec


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('kind,net', NETS)
def test_state_dict_manifest(recorded, kind, net):
    """the same keys, in the same order, with the same shapes; pos_embed bit-identical"""
    want, got = recorded['nets'][f'{kind}-{net}'], _manifest(_build(kind, net))
    assert got['class'] == want['class']
    assert got['keys'] == want['keys']
    assert got.get('pos_embed_sha256') == want.get('pos_embed_sha256')


def test_manifest_covers_the_eight_classes(recorded):
    assert {v['class'] for v in recorded['nets'].values()} == set(MRO)


def test_registries_build_the_recorded_classes(recorded):
    regs = _registries()
    assert {f'{kind}:{key}' for kind, reg in regs.items() for key in reg} == set(recorded['registry'])
    for name, want in recorded['registry'].items():
        kind, key = name.split(':', 1)
        m = _registry_instance(kind, key)
        got = {'class': type(m).__name__, 'depth': m.depth, 'hidden_size': m.embed_dim, 'num_heads': m.num_heads,
               'patch_size': m.patch_size, 'keys': len(m.state_dict())}
        assert got == want, name


# the ancestry of every class of the family up to the base (whose own ancestors are the packed-weights holder and nn.Module)
MRO = {
    'DiT_TriLatent': ['DiT_TriLatent', 'DiT'],
    'DiT_I23D_PixelArt': ['DiT_I23D_PixelArt', 'DiT'],
    'DiT_I23D': ['DiT_I23D', 'DiT_I23D_PixelArt', 'DiT'],
    'DiT_I23D_PixelArt_MVCond': ['DiT_I23D_PixelArt_MVCond', 'DiT_I23D_PixelArt', 'DiT'],
    'DiT_I23D_PixelArt_MVCond_noClip': ['DiT_I23D_PixelArt_MVCond_noClip', 'DiT_I23D_PixelArt', 'DiT'],
    'DiT_TriLatent_PixelArt': ['DiT_TriLatent_PixelArt', 'DiT_I23D_PixelArt', 'DiT'],
    'DiT_pcd_I23D_PixelArt_MVCond': ['DiT_pcd_I23D_PixelArt_MVCond', 'DiT_I23D_PixelArt_MVCond', 'DiT_I23D_PixelArt', 'DiT'],
}


def _family():
    from ln3diff_amd.dit import dit_i23d, dit_trilatent
    return {n: getattr(dit_trilatent if n == 'DiT_TriLatent' else dit_i23d, n) for n in MRO}


def test_classes_are_related_through_the_base_and_their_stated_parent_only():
    from ln3diff_amd.dit import dit_trilatent
    for name, cls in _family().items():
        names = [c.__name__ for c in cls.__mro__]
        assert names[:names.index('DiT') + 1] == MRO[name], name
        assert cls.__mro__[names.index('DiT')] is dit_trilatent.DiT


def test_prepare_timesteps_is_t23d_surface_only():
    """the whole-schedule adaLN cache is sized for depth*6D + 2D columns, which only DiT_TriLatent's pack has"""
    assert [n for n, cls in _family().items() if hasattr(cls, 'prepare_timesteps')] == ['DiT_TriLatent']


def test_mxfp8_is_refused_by_class_not_by_function_identity():
    """an I23D class refuses 'mxfp8' with the ValueError it always raised and drops nothing; 'bf16' is a no-op"""
    m = R.build_i23d('pixart')
    m._packed = sentinel = object()
    with pytest.raises(ValueError, match='the mxfp8 path is built for the T23D DiT_TriLatent forward only'):
        m.set_matmul_precision('mxfp8')
    assert m.set_matmul_precision('bf16') is m and m._packed is sentinel and m.matmul_precision == 'bf16'
    with pytest.raises(ValueError, match="expected one of"):
        m.set_matmul_precision('fp8')


if __name__ == '__main__':
    assert sys.argv[1:] == ['--dump']
    with open(FIXTURE, 'w') as f:
        json.dump(_record(), f, indent=1)
        f.write('\n')
