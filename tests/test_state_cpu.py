"""Packed weight copies never go stale: every class that keeps device copies of its weights (ln3diff_amd/_cache.py), every channel
that may change weights, checked at the pack level on the CPU - no kernel runs.

For each (holder, channel): pack once, apply the channel, pack again.  Every tensor reachable from the new pack (side caches included:
the posterior's quant_conv, the ShapeNet ldm_downsample, Triplane's decoder fragments, the image embedders' runner and projection)
equals, element for element, the pack of a FRESH instance that was built from scratch and given the final weights; and at least one
tensor differs from the old pack, so that a pass is not vacuous.  The reference is the fresh instance, the comparison is torch.equal:
what is pinned is independence from history, nothing numerical.  The MX-FP8 operands are quantised on the device and are covered by
tests/test_state_gpu.py."""
import pytest
import torch

from state_holders import CHANNELS, HOLDERS, fresh_like, same, snapshot

CPU = torch.device('cpu')


@pytest.mark.parametrize('channel', list(CHANNELS))
@pytest.mark.parametrize('spec', HOLDERS, ids=lambda s: s.name)
def test_repack_follows(spec, channel, tmp_path):
    root, h = spec.build(0)
    old = snapshot(spec.pack(h, CPU))
    assert any(torch.is_tensor(v) for v in old.values())
    assert same(old, snapshot(spec.pack(h, CPU))) == []              # packing again without a change gives the same pack
    CHANNELS[channel](root, h, spec, tmp_path)
    new = snapshot(spec.pack(h, CPU))
    _, hf = fresh_like(spec, root)
    want = snapshot(spec.pack(hf, CPU))
    assert same(new, want) == [], (spec.name, channel)
    assert same(new, old) != [], (spec.name, channel, 'the channel changed nothing that is packed')


@pytest.mark.parametrize('spec', [s for s in HOLDERS if s.name.startswith('DiT_') or s.name == 'Triplane'], ids=lambda s: s.name)
def test_precision_there_and_back(spec):
    """set_matmul_precision / set_plane_precision to the opt-in format and back: the bf16 / fp32 pack is what a fresh instance packs.
    (The 'mxfp8' pack itself needs the device's quantiser: tests/test_state_gpu.py.)"""
    root, h = spec.build(0)
    first = spec.pack(h, CPU)
    old = snapshot(first)
    if spec.name == 'Triplane':
        h.set_plane_precision('fp16')
        h.set_plane_precision('fp32')
    else:
        if spec.name == 'DiT_TriLatent':
            h.set_matmul_precision('mxfp8')
            assert h._packed is None                                 # the other precision's operands are not kept
        else:
            with pytest.raises(ValueError):
                h.set_matmul_precision('mxfp8')                      # built for the T23D forward only: refused, nothing dropped
        h.set_matmul_precision('bf16')
    new = snapshot(spec.pack(h, CPU))
    _, hf = fresh_like(spec, root)
    assert same(new, snapshot(spec.pack(hf, CPU))) == [] and same(new, old) == []


def test_walker_sees_a_difference():
    """the comparison itself: one changed element, a missing entry and a changed plain value are each reported"""
    a = {'w': torch.zeros(3), 'l': [{'b': torch.ones(2)}], 'n': 4, 'epoch': 1}
    b = {'w': torch.zeros(3), 'l': [{'b': torch.ones(2)}], 'n': 4, 'epoch': 9}
    assert same(snapshot(a), snapshot(b)) == []
    b['l'][0]['b'][1] = 2.0
    assert same(snapshot(a), snapshot(b)) == ['/l/0/b']
    b['n'] = 5
    del b['w']
    assert same(snapshot(a), snapshot(b)) == ['/l/0/b', '/n', '/w']


# ----------------------------------------------------------------------------- the protocol has one owner: _cache.PackedWeights
def _package_files():
    import os
    import ln3diff_amd
    root = os.path.dirname(ln3diff_amd.__file__)
    return root, sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.endswith('.py'))


def _package_modules():
    import importlib
    import os
    root, files = _package_files()
    names = [os.path.relpath(f, os.path.dirname(root))[:-3].replace(os.sep, '.') for f in files]
    return [importlib.import_module(n[:-9] if n.endswith('.__init__') else n) for n in names]


def test_every_direct_holder_is_in_the_table():
    """every class of the package that lists PackedWeights in its bases is state-tested: it is in the MRO of some HOLDERS entry"""
    from ln3diff_amd._cache import PackedWeights
    _package_modules()
    direct = {c for c in PackedWeights.__subclasses__() if c.__module__.startswith('ln3diff_amd.')}
    assert len(direct) >= 9, sorted(c.__name__ for c in direct)
    tested = set()
    for spec in HOLDERS:
        tested.update(type(spec.pick(spec.root())).__mro__)
    assert direct - tested == set(), sorted(c.__name__ for c in direct - tested)
    from ln3diff_amd.vit.vit_triplane import _PosteriorSeams          # the seam calls _side_pack: its concrete classes must be holders
    users = _PosteriorSeams.__subclasses__()
    assert len(users) >= 2 and all(issubclass(c, PackedWeights) for c in users), users


def test_cache_protocol_is_spelled_in_one_place():
    """no file of the package but _cache.py uses the primitives of the protocol, and no class but PackedWeights overrides _apply"""
    import ast
    import os
    from ln3diff_amd._cache import PackedWeights
    _, files = _package_files()
    assert len(files) > 20
    bad, private = [], {'stamp', 'fresh', 'watch', 'watch_tree', 'EPOCH'}
    for path in files:
        src = open(path).read()
        outside = os.path.basename(path) != '_cache.py'
        if outside:
            bad += [(path, w) for w in ('_cache.stamp', '_cache.fresh', '_cache.watch', '_cache.EPOCH') if w in src]
        for node in ast.walk(ast.parse(src)):
            if outside and isinstance(node, ast.Attribute) and node.attr in private:         # under any name of the module
                bad.append((path, node.lineno, '.' + node.attr))
            if outside and isinstance(node, ast.ImportFrom) and (node.module or '').split('.')[-1] == '_cache':
                bad += [(path, node.lineno, 'import ' + n.name) for n in node.names if n.name in private or n.name == '*']
            if isinstance(node, ast.ClassDef) and node.name != 'PackedWeights':
                bad += [(path, node.name + '._apply') for f in node.body if isinstance(f, ast.FunctionDef) and f.name == '_apply']
    assert bad == []
    for mod in _package_modules():                 # and at run time: every _apply in the package is PackedWeights' or torch's
        for c in vars(mod).values():
            if isinstance(c, type) and c.__module__ == mod.__name__ and c is not PackedWeights:
                assert '_apply' not in vars(c), c
