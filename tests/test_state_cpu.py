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
