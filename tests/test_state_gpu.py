"""State carried from one call to the next, on the device: packed weight copies, prepared context / timestep caches, Workspace scratch
and the precision switches must never let an earlier call show in a later one.

The reference of every comparison is a FRESH instance: built from scratch, given the same final weights, and called once with only the
call under test.  The comparison is torch.equal (fresh against fresh is bitwise repeatable on every path below; no tolerance anywhere in
this file).  Every test also asserts that what it changes does change the output, so that a pass is not vacuous.

(a) weights: call, channel, call over every channel that may change weights (tests/state_holders.py), one chain per holder.
    parallel.broadcast_flat is not in the device chain: towards the caches it is the in-place write + epoch bump that
    `invalidate_weight_caches` is here, and its bump is checked for every holder in tests/test_state_cpu.py.
(b) prepared caches: a cache from before a weight change is refused by name; prepared caches do not alias each other.
    The stale mod_cache refusal is tested on DiT_TriLatent only: the I23D family's forward takes no mod_cache (it runs its own
    timestep path; the keyword falls into **kwargs), so there is nothing prepared to go stale there.
(c) scratch reuse: shape A, shape B, shape A through one instance, B chosen to stress the Workspace keys.
(d) poison: a call with NaN / +-Inf in one input element, then the finite call; also with the poisoned call at the larger member of
    a pair of extents that share one padded scratch shape (100 / 121 point tokens + 256 appended: both pad to 384 keys; 736 / 768 with the append cache: 1024).
    The text tower takes integer ids: it has no input that can hold a non-finite value.  One case per DiT family runs the poisoned and
    the finite call through ONE prepared context (the server loop after a diverged sample).
(e) one pack per device: 'cuda' and 'cuda:<current>' get the same pack object and the same scratch.
"""
import pytest
import torch

from state_holders import BY_NAME, CHANNELS, fresh_like, new_values

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _in(name, shape, seed=0):
    from ln3diff_amd.synth import synth_input
    return synth_input(name, shape, seed).to(DEV)


# ----------------------------------------------------------------------------- one call per network: inputs(**variant), call(root, inputs)
def _t23d_in(B=2, L=77, twins=False, **_):
    c = _in('c', (B, L, 768), 1)
    if twins:                                             # [uc ; c]: zero embeddings lead, the same latents / timestep twice
        c = torch.cat([torch.zeros_like(c[:B // 2]), c[:B // 2]])
        return {'x': _in('x', (B // 2, 12, 32, 32), 1), 't': torch.full((B,), 500.0, device=DEV), 'ctx': c}
    return {'x': _in('x', (B, 12, 32, 32), 1), 't': torch.linspace(50, 900, B).to(DEV), 'ctx': c}


def _t23d_call(m, i, twins=False, precision=None, **_):
    if precision is not None:
        m.set_matmul_precision(precision)
    if twins:
        cc = m.prepare_context(i['ctx'])
        mc = m.prepare_timesteps(i['t'][None].cpu())
        return m(i['x'], i['t'], context_cache=cc, mod_cache=(mc, 0), in_scale=torch.full_like(i['t'], 0.5), cfg_twins=True)
    return m(i['x'], i['t'], i['ctx'])


def _i23d_in(B=2, fold=False, **_):
    ca, v = _in('ca', (B, 256, 2048), 2), _in('v', (B, 768), 2)
    if fold:                                              # flow matching order [c ; uc]: the zero half trails
        ca, v = torch.cat([ca[:B // 2], torch.zeros_like(ca[:B // 2])]), torch.cat([v[:B // 2], torch.zeros_like(v[:B // 2])])
    return {'x': _in('x', (B, 12, 32, 32), 2), 't': torch.linspace(0.1, 0.9, B).to(DEV), 'ctx': ca, 'vec': v}


def _i23d_call(m, i, **_):
    return m(i['x'], i['t'], {'crossattn': i['ctx'], 'vector': i['vec']})


def _pcd_in(B=2, N=96, **_):
    return {'x': _in('pcd', (B, 768, 19), 3)[:, :N].contiguous(), 't': torch.linspace(0.1, 0.9, B).to(DEV), 'ctx': _in('ca', (B, 256, 1024), 3),
            'vec': _in('v', (B, 768), 3), 'mv': _in('mv', (B, 2, 64, 768), 3)}


def _pcd_call(m, i, **_):
    return m(i['x'], i['t'], {'crossattn': i['ctx'], 'vector': i['vec'], 'concat': i['mv']})


def _ae_in(B=1, **_):
    return {'x': _in('lat', (B, 12, 32, 32), 4)}


def _ae_call(dec, i, **_):
    return dec.vit_decode_postprocess(dec.vit_decode_backbone(i['x']), {})['latent_after_vit']


def _ffhq_in(B=1, **_):
    return {'x': _in('lat', (B, 12, 16, 16), 5)}


def _dino_dec_call(dec, i, **_):
    vit = dec.vit_decode_backbone({'latent_normalized_2Ddiffusion': i['x']}, 128)
    return dec.vit_decode_postprocess(vit, {})['planes_channel_last']


def _enc_in(N=6, S=32, **_):
    return {'x': _in('mv', (12, 10, 40, 40), 6)[:N, :, :S, :S].contiguous()}


def _unet_in(B=2, L=77, **_):
    return {'x': _in('x', (B, 4, 16, 16), 7), 't': torch.linspace(20, 900, B).to(DEV), 'ctx': _in('c', (B, L, 768), 7)}


def _tp_in(V=3, res=8, rays=False, **_):
    from ln3diff_amd.synth import orbit_cameras
    g = torch.Generator().manual_seed(8)
    cams = orbit_cameras(8)[[1, 4, 6][:V]]
    i = {'x': _in('planes', (V, 96, 32, 32), 8) * 4.0, 'cams': cams.to(DEV), 'j': torch.rand(V, res * res, 64, generator=g).to(DEV),
         'u': torch.rand(V * res * res, 64, generator=g).to(DEV), 'res': res}
    if rays:
        from oracle import render as orender
        ro, rd = orender.make_rays(cams, res)
        i['ro'], i['rd'] = ro.to(DEV), rd.to(DEV)
    return i


def _tp_call(tp, i, rays=False, plane_precision=None, **_):
    if plane_precision is not None:
        tp.set_plane_precision(plane_precision)
    if rays:
        V = i['x'].shape[0]
        o = tp.renderer(i['x'].view(V, 3, 32, 32, 32), tp.decoder, i['ro'], i['rd'], tp.rendering_kwargs, jitter=i['j'], u_fine=i['u'])
        return torch.cat([o['feature_samples'], o['depth_samples'], o['weights_samples']], -1)
    o = tp(i['x'], i['cams'], neural_rendering_resolution=i['res'], jitter=i['j'], u_fine=i['u'])
    return torch.cat([o['image_raw'], o['image_depth'], o['weights_samples']], 1)


def _clip_in(B=2, **_):
    from conftest import golden
    ids = torch.from_numpy(golden('clip_text_tiny')['ids']).long()
    return {'ids': ids.repeat(4, 1)[:B].to(DEV)}


def _img_in(B=2, **_):
    return {'x': torch.tanh(_in('img', (B, 3, 56, 56), 9))}


NETS = {   # holder name -> (inputs, call on the ROOT'S picked module; `on_root`: the call goes through the root that contains the holder)
    'DiT_TriLatent': (_t23d_in, _t23d_call, False),
    'DiT_I23D_PixelArt': (_i23d_in, _i23d_call, False),
    'DiT_pcd_I23D_PixelArt_MVCond': (_pcd_in, _pcd_call, False),
    'DiT2': (_ae_in, _ae_call, True),
    'AE_decoder': (_ae_in, _ae_call, True),
    'ShapeNet_decoder': (_ae_in, _dino_dec_call, True),
    'FFHQ_decoder': (_ffhq_in, _dino_dec_call, True),
    'mv_Encoder': (_enc_in, lambda m, i, **_: m(i['x']), False),
    'UNetModel': (_unet_in, lambda m, i, **_: m(i['x'], i['t'], context=i['ctx']), False),
    'Triplane': (_tp_in, _tp_call, False),
    'FrozenCLIPEmbedder': (_clip_in, lambda m, i, **_: m(i['ids'])[0], False),
    'FrozenOpenCLIPImageEmbedder': (_img_in, lambda m, i, **_: torch.cat([t.flatten(1) for t in m(i['x'])], 1), False),
    'FrozenDinov2ImageEmbedder': (_img_in, lambda m, i, **_: m(i['x']), False),
}


def run(name, root, h, variant=None, poison=None):
    """one call of network `name`; poison = (input key, value): an inner and the last element of that input are overwritten"""
    variant = variant or {}
    inputs, call, on_root = NETS[name]
    i = inputs(**variant)
    if poison is not None:
        key, value = poison
        i[key] = i[key].clone()
        if name == 'Triplane':                              # one texel row through the volume's centre: rays do cross it
            i[key][0, :, 16, :] = value
        else:
            i[key].view(-1)[i[key].numel() // 3] = value
            i[key].view(-1)[-1] = value                     # and the last row: with appended tokens it lands in the last key rows
    y = call(root if on_root else h, i, **variant)
    torch.cuda.synchronize()
    return y.clone()


_FRESH = {}


def fresh_out(name, variant=None, seed=0):
    """the reference: a fresh instance with the seed's weights, called once with only this call (computed once, shared, never changed)"""
    key = (name, tuple(sorted((variant or {}).items())), seed)
    if key not in _FRESH:
        root, h = BY_NAME[name].build(seed)
        root.to(DEV)
        _FRESH[key] = run(name, root, h, variant)
    return _FRESH[key]


def built(name, seed=0):
    root, h = BY_NAME[name].build(seed)
    root.to(DEV)
    return root, h


def same(a, b, what=''):
    if a.shape == b.shape and torch.equal(a, b):
        return True
    d = float((a.double() - b.double()).abs().max()) if a.shape == b.shape else 'shapes %s / %s' % (tuple(a.shape), tuple(b.shape))
    print('state: NOT equal', what, 'max abs diff', d)
    return False


# ----------------------------------------------------------------------------- (a) weights
GPU_CHANNELS = [c for c in CHANNELS if c != 'broadcast_flat']


@pytest.mark.parametrize('name', list(NETS))
def test_weights_chain(hip_lib, name, tmp_path):
    spec = BY_NAME[name]
    root, h = built(name)
    want = fresh_out(name)
    prev = run(name, root, h)
    assert same(prev, want, 'first call')
    for ch in GPU_CHANNELS:
        CHANNELS[ch](root, h, spec, tmp_path)
        y = run(name, root, h)
        r2, h2 = fresh_like(spec, root, DEV)
        assert same(y, run(name, r2, h2), f'{name} after {ch}'), (name, ch)
        assert not torch.equal(y, prev), (name, ch, 'the channel did not change the output')
        # building the fresh instance loaded weights and so moved the global epoch: call again, so that the holder's caches are current
        # and the NEXT channel alone has to invalidate them
        assert same(run(name, root, h), y, f'{name} again after {ch}'), (name, ch)
        prev = y


def test_mxfp8_pack_follows_weights(hip_lib, tmp_path):
    """the MX-FP8 operands are quantised on the device when the model is packed: they follow every channel too"""
    name, v = 'DiT_TriLatent', {'precision': 'mxfp8'}
    spec = BY_NAME[name]
    root, h = built(name)
    prev = run(name, root, h, v)
    assert not torch.equal(prev, fresh_out(name))                      # the other precision is another output
    for ch in ('load_state_dict', 'load_child', 'apply', 'invalidate_weight_caches'):
        CHANNELS[ch](root, h, spec, tmp_path)
        y = run(name, root, h, v)
        r2, h2 = fresh_like(spec, root, DEV)
        assert same(y, run(name, r2, h2, v), ch) and not torch.equal(y, prev), ch
        assert same(run(name, root, h, v), y, ch)                      # caches current again (the fresh instance moved the epoch)
        prev = y


# ----------------------------------------------------------------------------- (b) prepared caches
def _ctx_of(name, i):
    return {'DiT_TriLatent': lambda: i['ctx'], 'DiT_I23D_PixelArt': lambda: {'crossattn': i['ctx'], 'vector': i['vec']},
            'DiT_pcd_I23D_PixelArt_MVCond': lambda: {'crossattn': i['ctx'], 'vector': i['vec'], 'concat': i['mv']}}[name]()


PREPARED = ['DiT_TriLatent', 'DiT_I23D_PixelArt', 'DiT_pcd_I23D_PixelArt_MVCond']


@pytest.mark.parametrize('name', PREPARED)
def test_stale_context_cache_is_refused(hip_lib, name):
    spec = BY_NAME[name]
    root, m = built(name)
    i = NETS[name][0]()
    want0 = fresh_out(name)                        # first: building an instance loads weights, which moves the global epoch
    cc = m.prepare_context(_ctx_of(name, i))
    y0 = m(i['x'], i['t'], context_cache=cc).clone()
    assert same(y0, want0, 'prepared context, first use')
    m.load_state_dict(new_values(m.state_dict(), 21), strict=True)
    with pytest.raises(RuntimeError, match='prepare_context'):
        m(i['x'], i['t'], context_cache=cc)
    y1 = m(i['x'], i['t'], context_cache=m.prepare_context(_ctx_of(name, i))).clone()
    r2, m2 = fresh_like(spec, root, DEV)
    assert same(y1, run(name, r2, m2), 'prepared again') and not torch.equal(y1, y0)
    # the epoch is global: a load into an unrelated module counts as well
    cc = m.prepare_context(_ctx_of(name, i))
    other = torch.nn.Linear(2, 2)
    from ln3diff_amd import _cache
    _cache.watch(other)
    other.load_state_dict(other.state_dict())
    with pytest.raises(RuntimeError, match='prepare_context'):
        m(i['x'], i['t'], context_cache=cc)


def test_stale_timestep_cache_is_refused(hip_lib):
    name = 'DiT_TriLatent'
    spec = BY_NAME[name]
    root, m = built(name)
    i = NETS[name][0]()
    sched = torch.stack([i['t'].cpu(), i['t'].cpu().flip(0)])
    cached = lambda net: net(i['x'], i['t'], i['ctx'], mod_cache=(net.prepare_timesteps(sched), 0)).clone()
    want0 = cached(built(name)[1])                 # first: building an instance moves the global epoch
    mc = m.prepare_timesteps(sched)
    y0 = m(i['x'], i['t'], i['ctx'], mod_cache=(mc, 0)).clone()
    assert same(y0, want0, 'prepared timesteps, first use')
    m.load_state_dict(new_values(m.state_dict(), 22), strict=True)
    with pytest.raises(RuntimeError, match='prepare_timesteps'):
        m(i['x'], i['t'], i['ctx'], mod_cache=(mc, 0))
    y1 = cached(m)
    assert same(y1, cached(fresh_like(spec, root, DEV)[1]), 'prepared again') and not torch.equal(y1, y0)


@pytest.mark.parametrize('rows', ['one row per step', 'a row per sample'])
def test_two_schedules_of_one_length_do_not_alias(hip_lib, rows):
    """prepare_timesteps returns storage of its own: preparing a second schedule with the same step count leaves the first alone"""
    name = 'DiT_TriLatent'
    root, m = built(name)
    i = NETS[name][0]()
    if rows == 'one row per step':
        s1, s2 = torch.tensor([[700.0] * 2, [300.0] * 2]), torch.tensor([[650.0] * 2, [120.0] * 2])
    else:
        s1, s2 = torch.tensor([[700.0, 20.0], [300.0, 900.0]]), torch.tensor([[650.0, 40.0], [120.0, 500.0]])
    _, mf = built(name)                                                  # fresh instance: only schedule 1 is ever prepared
    mcf = mf.prepare_timesteps(s1)
    mc1 = m.prepare_timesteps(s1)
    mc2 = m.prepare_timesteps(s2)
    assert mc1['mod'].data_ptr() != mc2['mod'].data_ptr()
    for step in (0, 1):
        got = m(i['x'], s1[step].to(DEV), i['ctx'], mod_cache=(mc1, step)).clone()
        assert same(got, mf(i['x'], s1[step].to(DEV), i['ctx'], mod_cache=(mcf, step)), f'schedule 1 step {step} after preparing schedule 2')
        assert same(got, m(i['x'], s1[step].to(DEV), i['ctx']), f'step {step} against the run without mod_cache')
        assert not torch.equal(got, m(i['x'], s2[step].to(DEV), i['ctx'], mod_cache=(mc2, step)))


@pytest.mark.parametrize('name,append,fold', [('DiT_TriLatent', True, True), ('DiT_TriLatent', True, False),      # (no append cache there)
                                              ('DiT_I23D_PixelArt', True, True), ('DiT_I23D_PixelArt', True, False),
                                              ('DiT_I23D_PixelArt', False, True), ('DiT_I23D_PixelArt', False, False)])
def test_two_prompts_a_b_a(hip_lib, monkeypatch, name, append, fold):
    """two prepared prompts used in the order A, B, A, with an unrelated forward at another batch size in between; the I23D append
    cache on and off (off: the identity check on _ha_src / _ha_buf), the zero-context fold on and off"""
    if not append:
        monkeypatch.setenv('LN3D_NO_APPEND_CACHE', '1')
    if not fold:
        monkeypatch.setenv('LN3D_NO_UC_FOLD', '1')
    va = {'B': 2, 'twins': True} if name == 'DiT_TriLatent' else {'B': 2, 'fold': True}
    root, m = built(name)
    ia = NETS[name][0](**va)
    ib = {k: (v.flip(1) if k in ('ctx', 'vec') and v.dim() > 1 else v) for k, v in ia.items()}     # another prompt, the same zeros
    if name == 'DiT_TriLatent':
        ia['x'], ib['x'] = ia['x'].repeat(2, 1, 1, 1), ib['x'].repeat(2, 1, 1, 1)
    # references: a fresh instance per prompt, one call with the plain context
    refs = []
    for i in (ia, ib):
        _, mf = built(name)
        refs.append(mf(i['x'], i['t'], _ctx_of(name, i)).clone())
    assert not torch.equal(refs[0], refs[1])
    cca, ccb = m.prepare_context(_ctx_of(name, ia)), m.prepare_context(_ctx_of(name, ib))
    assert cca['fold'] == ccb['fold'] == (1 if fold else 0)
    y = [m(ia['x'], ia['t'], context_cache=cca).clone(), m(ib['x'], ib['t'], context_cache=ccb).clone()]
    if name != 'DiT_TriLatent':
        assert (cca.get('akv') is not None) == append
    run(name, root, m, {'B': 3})                                         # unrelated forward, another batch size, same network
    y.append(m(ia['x'], ia['t'], context_cache=cca).clone())
    run(name, root, m, {'B': 3})
    y.append(m(ib['x'], ib['t'], context_cache=ccb).clone())
    for k, (got, want) in enumerate(zip(y, (refs[0], refs[1], refs[0], refs[1]))):
        assert same(got, want, f'{name} use {k}'), k


def test_one_context_at_two_token_counts(hip_lib):
    """the point-cloud variant takes any number of points per call: one prepared context serves 736, 768 and 736 points (with the 256
    appended tokens both pad to 1024 keys; the appended K / V^T cache, which engages at these row counts, is per token count)"""
    name = 'DiT_pcd_I23D_PixelArt_MVCond'
    root, m = built(name)
    va, vb = {'B': 4, 'N': 736}, {'B': 4, 'N': 768}
    ia, ib = NETS[name][0](**va), NETS[name][0](**vb)
    wa, wb = fresh_out(name, va), fresh_out(name, vb)
    cc = m.prepare_context(_ctx_of(name, ia))
    for k, (i, want) in enumerate(((ia, wa), (ib, wb), (ia, wa))):
        assert same(m(i['x'], i['t'], context_cache=cc).clone(), want, f'use {k}'), k
    assert cc.get('akv') is not None


# ----------------------------------------------------------------------------- (c) scratch reuse: A, B, A
SEQUENCES = [
    ('DiT_TriLatent', {'B': 4}, {'B': 2}),
    ('DiT_TriLatent', {'B': 4, 'twins': True}, {'B': 2, 'twins': True}),
    ('DiT_TriLatent', {'L': 77}, {'L': 40}),                              # another 64-row pad
    ('DiT_TriLatent', {'L': 77}, {'L': 100}),                             # the same 128-row pad
    ('DiT_TriLatent', {'precision': 'bf16'}, {'precision': 'mxfp8'}),
    ('DiT_I23D_PixelArt', {'B': 4}, {'B': 2}),
    ('DiT_I23D_PixelArt', {'B': 4, 'fold': True}, {'B': 2, 'fold': True}),
    ('DiT_pcd_I23D_PixelArt_MVCond', {'N': 100}, {'N': 121}),              # 356 / 377 keys: one 384-key scratch shape
    ('DiT_pcd_I23D_PixelArt_MVCond', {'B': 4, 'N': 736}, {'B': 4, 'N': 768}),   # append cache on, 992 / 1024 keys: one 1024-key shape
    ('DiT_pcd_I23D_PixelArt_MVCond', {'B': 2}, {'B': 1}),
    ('AE_decoder', {'B': 2}, {'B': 1}),
    ('ShapeNet_decoder', {'B': 2}, {'B': 1}),
    ('FFHQ_decoder', {'B': 2}, {'B': 1}),
    # the encoder groups a fixed num_frames (> 4, set at construction) per object, so one instance cannot change its frame count:
    # what varies per call is the number of 6-frame objects (6 / 12 images) and the image size.  16 / 25 tokens per frame take two
    # attention routes (96 joint tokens: MFMA scratch padded to 128; 150: the small-sequence kernel, no padding); no two sizes of this
    # encoder share a padded scratch shape (that needs 6 * H * W % 32 == 0 twice within one multiple of 64)
    ('mv_Encoder', {'N': 6}, {'N': 12}),
    ('mv_Encoder', {'S': 32}, {'S': 40}),
    ('UNetModel', {'B': 4}, {'B': 2}),
    ('UNetModel', {'L': 77}, {'L': 40}),
    ('UNetModel', {'L': 77}, {'L': 100}),
    ('Triplane', {'V': 3}, {'V': 1}),
    ('Triplane', {'res': 8}, {'res': 16}),
    ('Triplane', {'V': 3, 'rays': True}, {'V': 1, 'rays': True}),
    ('Triplane', {'plane_precision': 'fp32'}, {'plane_precision': 'fp16'}),
    ('FrozenCLIPEmbedder', {'B': 4}, {'B': 2}),
    ('FrozenOpenCLIPImageEmbedder', {'B': 4}, {'B': 2}),
    ('FrozenDinov2ImageEmbedder', {'B': 4}, {'B': 2}),
]


@pytest.mark.parametrize('name,a,b', SEQUENCES, ids=[f'{n}-{a}-{b}'.replace(' ', '').replace("'", '') for n, a, b in SEQUENCES])
def test_scratch_a_b_a(hip_lib, name, a, b):
    root, h = built(name)
    wa, wb = fresh_out(name, a), fresh_out(name, b)
    assert wa.shape != wb.shape or not torch.equal(wa, wb)
    for k, v in enumerate((a, b, a)):
        assert same(run(name, root, h, v), wa if v is a else wb, f'{name} call {k} {v}'), (k, v)


# ----------------------------------------------------------------------------- (d) poison
POISON = [   # network, input keys that can hold a non-finite value, finite variant, poisoned variant (None: the same shape)
    ('DiT_TriLatent', ('x', 'ctx'), {}, None),
    ('DiT_TriLatent', ('x', 'ctx'), {'L': 77}, {'L': 100}),
    ('DiT_TriLatent', ('x',), {'precision': 'mxfp8'}, None),
    ('DiT_I23D_PixelArt', ('x', 'ctx', 'vec'), {}, None),
    ('DiT_pcd_I23D_PixelArt_MVCond', ('x', 'ctx', 'mv'), {}, None),
    ('DiT_pcd_I23D_PixelArt_MVCond', ('x', 'ctx'), {'N': 100}, {'N': 121}),     # the same-pad pair: poisoned at the larger member
    ('DiT_pcd_I23D_PixelArt_MVCond', ('x', 'ctx'), {'B': 4, 'N': 736}, {'N': 768}),    # the same, with the append cache on
    ('AE_decoder', ('x',), {}, None),
    ('ShapeNet_decoder', ('x',), {}, None),
    ('FFHQ_decoder', ('x',), {}, None),
    ('mv_Encoder', ('x',), {}, None),
    ('UNetModel', ('x', 'ctx'), {}, None),
    ('UNetModel', ('x', 'ctx'), {'L': 77}, {'L': 100}),
    ('Triplane', ('x',), {}, None),
    ('FrozenOpenCLIPImageEmbedder', ('x',), {}, None),
    ('FrozenDinov2ImageEmbedder', ('x',), {}, None),
]


@pytest.mark.parametrize('name,keys,fin,bad', POISON, ids=[f'{n}-{f}-{b}'.replace(' ', '').replace("'", '') for n, _, f, b in POISON])
def test_finite_call_after_poisoned_calls(hip_lib, name, keys, fin, bad):
    """NaN and +-Inf in one element of one input at a time (nothing is asserted about those outputs: non-finite values in a kernel
    are arithmetic), then the finite call: it equals the fresh instance's"""
    root, h = built(name)
    want = fresh_out(name, fin)
    assert bool(torch.isfinite(want).all())
    bad = fin if bad is None else dict(fin, **bad)
    for key in keys:
        spoiled = 0
        for value in (float('nan'), float('inf'), float('-inf')):
            y = run(name, root, h, bad, poison=(key, value))
            spoiled += int(not bool(torch.isfinite(y).all()) or (y.shape == want.shape and not torch.equal(y, want)))
            assert same(run(name, root, h, fin), want, f'{name} after {value} in {key}'), (key, value)
        assert spoiled > 0, (key, 'no poisoned call changed the output: the poison in this input never reached the network')


@pytest.mark.parametrize('name,fin,bad', [('DiT_TriLatent', {}, {}), ('DiT_I23D_PixelArt', {}, {}),
                                          ('DiT_pcd_I23D_PixelArt_MVCond', {'B': 4, 'N': 736}, {'B': 4, 'N': 768})],
                         ids=['DiT_TriLatent', 'DiT_I23D_PixelArt', 'DiT_pcd-736-after-768'])
def test_prepared_context_survives_a_diverged_latent(hip_lib, name, fin, bad):
    """the server loop: ONE prepared prompt, a call whose latent holds NaN / +-Inf, then the finite call through the same prepared
    context (its K / V^T, the appended tokens' K / V^T it owns, the scratch behind it); the point-cloud case poisons at 768 points and
    follows with 736 and 768 finite ones through the same context"""
    root, m = built(name)
    want, want_bad = fresh_out(name, fin), fresh_out(name, bad)          # first: building an instance moves the global epoch
    i_fin, i_bad = NETS[name][0](**fin), NETS[name][0](**bad)
    cc = m.prepare_context(_ctx_of(name, i_fin))
    assert same(m(i_fin['x'], i_fin['t'], context_cache=cc).clone(), want, 'before any poison')
    for value in (float('nan'), float('inf'), float('-inf')):
        x = i_bad['x'].clone()
        x.view(-1)[x.numel() // 3] = value
        x.view(-1)[-1] = value
        y = m(x, i_bad['t'], context_cache=cc).clone()
        assert not bool(torch.isfinite(y).all()), 'the poison never reached the network'
        assert same(m(i_fin['x'], i_fin['t'], context_cache=cc).clone(), want, f'{name} after {value}'), value
        assert same(m(i_bad['x'], i_bad['t'], context_cache=cc).clone(), want_bad, f'{name} after {value}, the poisoned shape'), value
    if name != 'DiT_TriLatent':
        assert cc.get('akv') is not None                                 # the appended-token cache was engaged throughout


# ----------------------------------------------------------------------------- (e) one pack per device, however the device is spelled
@pytest.mark.parametrize('name', ['Triplane', 'AE_decoder'])
def test_bare_cuda_and_indexed_cuda_name_one_pack(hip_lib, name):
    """torch.device('cuda') and torch.device('cuda', current_device) compare unequal; _ensure_packed normalises, so the second spelling
    gets the first one's pack (and the decoder keeps its Workspace and ConvStack) instead of a rebuild.  Packing only, no kernel."""
    if name == 'Triplane':
        from ln3diff_amd.nsr.triplane import Triplane
        h = Triplane(img_resolution=16).to(DEV)
    else:
        h = built(name)[1]
    bare, indexed = torch.device('cuda'), torch.device('cuda', torch.cuda.current_device())
    assert bare != indexed
    P = h._ensure_packed(bare)
    scratch = (h._ws, h._cs) if name == 'AE_decoder' else ()
    assert None not in scratch
    assert h._ensure_packed(indexed) is P and h._ensure_packed(bare) is P and P['device'] == indexed
    if name == 'AE_decoder':
        assert h._ws is scratch[0] and h._cs is scratch[1]
