"""GPU parity of the I23D path (DiT-PixArt denoiser with qk-norm / RMSNorm / appended DINO tokens + flow-matching ODE)
against the reference goldens.  Tolerances as in test_dit_gpu.py (bf16 operands, fp32 state).
The coefficients of the flow ODE / SDE loops are pinned per step, to 1e-5 against float64 with an exact field, in tests/test_sampler_loops_gpu.py."""
import pytest
import torch

from conftest import golden, load_synth, manifest, rel_l2

pytestmark = pytest.mark.gpu


def _build(hidden, depth, heads):
    from ln3diff_amd.dit.dit_i23d import DiT_I23D_PixelArt
    return DiT_I23D_PixelArt(input_size=32, patch_size=2, in_channels=4, hidden_size=hidden, depth=depth, num_heads=heads,
                             num_classes=0, learn_sigma=False, context_dim=1024, roll_out=True, pooling_ctx_dim=768)


def test_i23d_tiny_forward_with_cfg(hip_lib):
    from ln3diff_amd.synth import synth_input
    g = golden('i23d_tiny')
    m = _build(128, 2, 2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (4, 12, 32, 32), 0).cuda()
    ctx = {'crossattn': synth_input('ca', (4, 256, 2048), 0).cuda(), 'vector': synth_input('v', (4, 768), 0).cuda()}
    y = m.forward_with_cfg(x, torch.from_numpy(g['t']).cuda(), ctx, 4.0).cpu()
    e = rel_l2(y, g['y'])
    print('i23d tiny', e)
    assert e < 2e-2, e


def test_i23d_pixart_l2_forward_with_cfg(hip_lib):
    from ln3diff_amd.dit.dit_i23d import DiT_models
    from ln3diff_amd.synth import synth_input
    g = golden('i23d_pixart_l2')
    m = DiT_models['DiT-PixArt-L/2'](input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=1024,
                                     roll_out=True, pooling_ctx_dim=768)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (2, 12, 32, 32), 0).cuda()
    ctx = {'crossattn': synth_input('ca', (2, 256, 2048), 0).cuda(), 'vector': synth_input('v', (2, 768), 0).cuda()}
    y = m.forward_with_cfg(x, torch.from_numpy(g['t']).cuda(), ctx, 4.0).cpu()
    e = rel_l2(y, g['y'])
    print('i23d PixArt-L/2', e)
    assert e < 2e-2, e


@pytest.mark.parametrize("method,steps", [('euler', 50), ('heun', 10), ('midpoint', 10), ('rk4', 6)])
def test_flow_matching_ode_vs_reference_golden(hip_lib, method, steps):
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.transport import Sampler, create_transport
    g = golden(f'flow_tiny_{method}{steps}')
    m = _build(128, 2, 2)
    load_synth(m, 0)
    m = m.cuda()
    z = synth_input('z', (2, 12, 32, 32), 42).cuda()
    cond = {'crossattn': synth_input('ca', (2, 256, 2048), 42).cuda(), 'vector': synth_input('v', (2, 768), 42).cuda()}
    ctx = {k: torch.cat([v, torch.zeros_like(v)], 0) for k, v in cond.items()}       # flow matching: [c, uc]
    cache = m.prepare_context(ctx)
    fn = Sampler(create_transport(snr_type='lognorm')).sample_ode(sampling_method=method, num_steps=steps)
    y = fn(torch.cat([z, z]), m.forward_with_cfg, context_cache=cache, cfg_scale=4.0)[-1].chunk(2)[0].cpu()
    e = rel_l2(y, g['final'])
    print('flow', method, steps, e)
    assert e < 1e-2, e          # measured 1.7e-3 .. 1.9e-3


@pytest.mark.parametrize("method,steps,form,last", [('Euler', 25, 'sigma', 'Mean'), ('Heun', 8, 'linear', 'Euler'),
                                                    ('Euler', 12, 'decreasing', 'Tweedie')])
def test_flow_matching_sde_vs_reference_golden(hip_lib, method, steps, form, last):
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.transport import Sampler, create_transport
    g = golden(f'sde_tiny_{method.lower()}{steps}_{form}_{last.lower()}')
    m = _build(128, 2, 2)
    load_synth(m, 0)
    m = m.cuda()
    z = synth_input('z', (2, 12, 32, 32), 42).cuda()
    cond = {'crossattn': synth_input('ca', (2, 256, 2048), 42).cuda(), 'vector': synth_input('v', (2, 768), 42).cuda()}
    ctx = {k: torch.cat([v, torch.zeros_like(v)], 0) for k, v in cond.items()}
    cache = m.prepare_context(ctx)
    fn = Sampler(create_transport(snr_type='lognorm')).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=0.7,
                                                                  last_step=last, last_step_size=0.04, num_steps=steps)
    torch.manual_seed(1234)                     # same Wiener increments as the reference run (global CPU generator)
    xs = fn(torch.cat([z, z]), m.forward_with_cfg, context_cache=cache, cfg_scale=4.0)
    assert len(xs) == steps
    e = rel_l2(xs[-1].chunk(2)[0].cpu(), g['final'])
    print('sde', method, steps, form, last, e)
    assert e < 1e-2, e          # measured 1.7e-3 .. 1.9e-3
    with pytest.raises(TypeError):
        Sampler(create_transport()).sample_sde(diffusion_form='constant', num_steps=3)(z, m.forward_with_cfg, context_cache=cache, cfg_scale=4.0)


def test_dopri5_converges_to_fixed_step_solution(hip_lib):
    """Adaptive Dormand-Prince (parity unpinned: torchdiffeq is absent) must agree with a fine fixed-step Heun solution of
    the same ODE, and tighter tolerances must get closer."""
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.transport import Sampler, create_transport
    m = _build(128, 2, 2)
    load_synth(m, 0)
    m = m.cuda()
    z = synth_input('z', (2, 12, 32, 32), 42).cuda()
    cond = {'crossattn': synth_input('ca', (2, 256, 2048), 42).cuda(), 'vector': synth_input('v', (2, 768), 42).cuda()}
    ctx = {k: torch.cat([v, torch.zeros_like(v)], 0) for k, v in cond.items()}
    cache = m.prepare_context(ctx)
    S = Sampler(create_transport(snr_type='lognorm'))
    zz = torch.cat([z, z])
    ref = S.sample_ode(sampling_method='heun', num_steps=201)(zz, m.forward_with_cfg, return_trajectory=False,
                                                              context_cache=cache, cfg_scale=4.0)[-1]
    errs = []
    for rtol in (1e-2, 1e-3, 1e-4):
        fn = S.sample_ode(sampling_method='dopri5', num_steps=5, atol=1e-6, rtol=rtol)
        y = fn(zz, m.forward_with_cfg, context_cache=cache, cfg_scale=4.0)
        assert y.shape[0] == 5
        errs.append(rel_l2(y[-1].cpu(), ref.cpu()))
        print('dopri5 rtol', rtol, 'rel-l2 vs heun-200', errs[-1], fn.last_stats)
    assert errs[-1] < 5e-3 and errs[-1] <= errs[0] * 1.5


def test_dopri5_matches_the_oracle_restatement_step_for_step(hip_lib):
    """The released I23D sampler: sample_ode() defaults to torchdiffeq's dopri5 with atol 1e-6 / rtol 1e-3 (transport.py:377-380).
    torchdiffeq is absent, so the semantics (steps not clipped to the output grid, 4th-order dense output, rms error norm, step
    controller constants, Hairer's first step) are restated twice from its published algorithm - oracle/samplers.py on the CPU,
    ln3diff_amd/transport on the device - and compared here: same number of network evaluations and of accepted / rejected
    steps on an fp32 vector field, overshoot beyond t = 1, and - through the tiny I23D network - the final latent within the
    bf16-network tolerance.  An analytic ODE checks the solver itself to 1e-6 without any network."""
    from oracle import dit as odit, samplers as osamp
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.transport import Sampler, create_transport
    m = _build(128, 2, 2)
    sd, _ = load_synth(m, 0)
    m = m.cuda()
    z = synth_input('z', (2, 12, 32, 32), 42)
    cond = {'crossattn': synth_input('ca', (2, 256, 2048), 42), 'vector': synth_input('v', (2, 768), 42)}
    ctx = {k: torch.cat([v, torch.zeros_like(v)], 0) for k, v in cond.items()}
    zz = torch.cat([z, z])
    st = {}
    with torch.no_grad():
        y_or = osamp.flow_ode_dopri5(lambda x, t, **kw: odit.i23d_forward_with_cfg(sd, x, t, kw['context'], kw['cfg_scale'], 2), zz, 50,
                                     1e-6, 1e-3, st, context=ctx, cfg_scale=4.0)
    cache = m.prepare_context({k: v.cuda() for k, v in ctx.items()})
    fn = Sampler(create_transport(snr_type='lognorm')).sample_ode(num_steps=50)             # the reference's defaults: dopri5, 1e-6 / 1e-3
    traj = fn(zz.cuda(), m.forward_with_cfg, context_cache=cache, cfg_scale=4.0)
    assert traj.shape[0] == 50
    print('dopri5 oracle', st, 'hip', fn.last_stats, 'final rel-l2', rel_l2(traj[-1].cpu(), y_or))
    assert rel_l2(traj[-1].cpu(), y_or) < 1e-2                        # measured 1.7e-3
    # The step SEQUENCE depends on the error estimate, and at rtol 1e-3 that estimate sees the bf16 rounding of the network
    # (~1e-3 of |v|): the HIP path accepts smaller steps than the fp32 oracle (measured 5 steps / 32 evaluations vs 3 / 20).  Both
    # overshoot t = 1 and interpolate back, as torchdiffeq does.
    assert st['t_end'] >= 1.0 and fn.last_stats['t_end'] >= 1.0 and fn.last_stats['nfe'] <= 3 * st['nfe']
    # Step-for-step equality of the two restatements on a vector field that is the SAME fp32 arithmetic on both sides (elementwise
    # torch ops): number of evaluations, of attempted and accepted steps, the end of the last step, and all 50 outputs.
    field = lambda y, t, **kw: torch.sin(3.0 * t)[:, None, None, None] * y - 0.3 * y * y * y + torch.cos(y * 2.0)
    y0 = synth_input('y0', (2, 12, 32, 32), 7)
    for rtol in (1e-3, 1e-5):
        so = {}
        outs_o = []
        yo = osamp.flow_ode_dopri5(field, y0, 50, 1e-6, rtol, so)
        fh = Sampler(create_transport()).sample_ode(num_steps=50, atol=1e-6, rtol=rtol)
        th = fh(y0.cuda(), field)
        print('dopri5 fp32 field rtol', rtol, 'oracle', so, 'hip', fh.last_stats, 'final', rel_l2(th[-1].cpu(), yo))
        assert (fh.last_stats['nfe'], fh.last_stats['steps'], fh.last_stats['accepted']) == (so['nfe'], so['steps'], so['accepted'])
        assert abs(fh.last_stats['t_end'] - so['t_end']) < 1e-4 * so['t_end']
        assert rel_l2(th[-1].cpu(), yo) < 1e-5
    # analytic: dy/dt = -2 y + sin(3 t) through the device solver
    y0 = torch.tensor([[1.0, -0.5, 2.0, 0.25]] * 2).cuda()
    lin = lambda y, t, **kw: -2.0 * y + torch.sin(3.0 * t)[:, None]
    fa = Sampler(create_transport()).sample_ode(num_steps=11, atol=1e-9, rtol=1e-7)
    ya = fa(y0, lin)[-1].cpu().double()
    c = torch.tensor([[1.0, -0.5, 2.0, 0.25]]).double()
    import math
    exact = (c + 3.0 / 13.0) * math.exp(-2.0) + (2.0 * math.sin(3.0) - 3.0 * math.cos(3.0)) / 13.0
    assert float((ya[:1] - exact).abs().max()) < 2e-6, (ya, exact)


@pytest.mark.parametrize("size,B", [("tiny", 2), ("tiny", 3), ("L/2", 2)])
def test_i23d_unconditional_branch_fold_is_exact_algebra(hip_lib, size, B, monkeypatch):
    """[c, uc] batches of the flow-matching engine: the ZERO conditioning of the unconditional half (pipeline._zero_uc) makes every
    cross-attention key / value row of those samples identical, so their cross-attention sub-block is the constant to_out(v) + b.
    prepare_context() folds a TRAILING run of such samples into the self-attention projection's epilogue.  Checked against the same
    network with the fold off, against the CPU oracle, and that a leading zero half / a non-uniform half is not folded."""
    from ln3diff_amd.dit.dit_i23d import DiT_models
    from ln3diff_amd.synth import synth_input
    from oracle import dit as odit
    if size == "tiny":
        m = _build(128, 2, 2)
    else:
        m = DiT_models['DiT-PixArt-L/2'](input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=1024, roll_out=True,
                                         pooling_ctx_dim=768)
    sd, _ = load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (B, 12, 32, 32), 7).cuda()
    x2 = torch.cat([x, x])
    t = torch.full((2 * B,), 0.37).cuda()
    ca, v = synth_input('ca', (B, 256, 2048), 7).cuda(), synth_input('v', (B, 768), 7).cuda()
    ctx = {'crossattn': torch.cat([ca, torch.zeros_like(ca)]), 'vector': torch.cat([v, torch.zeros_like(v)])}      # [c, uc]
    cc = m.prepare_context(ctx)
    assert cc['fold'] == B and cc['const'].shape == (m.depth, 2 * B, m.embed_dim) and float(cc['const'][:, :B].abs().max()) == 0.0
    y_fold = m(x2, t, context_cache=cc)
    monkeypatch.setenv('LN3D_NO_UC_FOLD', '1')
    cc0 = m.prepare_context(ctx)
    assert cc0['fold'] == 0
    y_full = m(x2, t, context_cache=cc0)
    monkeypatch.delenv('LN3D_NO_UC_FOLD')
    e = rel_l2(y_fold, y_full)
    print(size, B, 'i23d fold vs no fold', e, 'cond half', rel_l2(y_fold[:B], y_full[:B]), 'uncond half', rel_l2(y_fold[B:], y_full[B:]))
    assert e < 1e-3, e
    if size == "tiny":
        pick = [0, B]
        y_or = odit.i23d_forward(sd, x2[pick].cpu(), t[:2].cpu(), {k: w[pick].cpu() for k, w in ctx.items()}, m.num_heads)
        assert rel_l2(y_fold[pick].cpu(), y_or) < 2e-2
    # zeros FIRST ([uc, c]) are not a trailing run; a second half with differing rows is not uniform
    assert m.prepare_context({'crossattn': torch.cat([torch.zeros_like(ca), ca]), 'vector': torch.cat([torch.zeros_like(v), v])})['fold'] == 0
    assert m.prepare_context({'crossattn': torch.cat([ca, ca.flip(0)]), 'vector': torch.cat([v, v])})['fold'] == 0
    # CLIP tokens identical per sample but NON-zero (a constant image embedding): still uniform attention, still exact
    flat = ca[:, :1].expand(-1, 256, -1).clone()
    flat[..., 1024:] = ca[..., 1024:]                                  # the DINO half feeds the self-attention tokens, not the keys
    ctx3 = {'crossattn': torch.cat([ca, flat]), 'vector': torch.cat([v, v])}
    cc3 = m.prepare_context(ctx3)
    assert cc3['fold'] == B
    y3 = m(x2, t, context_cache=cc3)
    monkeypatch.setenv('LN3D_NO_UC_FOLD', '1')
    y3_full = m(x2, t, context_cache=m.prepare_context(ctx3))
    monkeypatch.delenv('LN3D_NO_UC_FOLD')
    assert rel_l2(y3, y3_full) < 1e-3


@pytest.mark.parametrize("which", ["pixart", "mvcond", "plain"])
def test_appended_token_kv_cache_equals_full_projection(hip_lib, which, monkeypatch):
    """The tokens appended to the self-attention sequence are constant per prompt: their per-layer K / V^T rows are computed once
    (DiT_I23D_PixelArt._appended_kv) and the blocks project the x tokens only.  Same network output as projecting the whole
    [x ; appended] sequence in every block (LN3D_NO_APPEND_CACHE=1), at a width where the fused qk-norm epilogue applies."""
    from ln3diff_amd.dit import dit_i23d
    from ln3diff_amd.synth import synth_input
    kw = dict(input_size=32, patch_size=2, in_channels=4, hidden_size=512, depth=2, num_heads=8, num_classes=0, learn_sigma=False,
              roll_out=True)
    B = 6               # 6 x 256 appended rows = 1536: the size from which the appended rows' own projection also takes the fused-norm tiles
    if which == "pixart":
        m = dit_i23d.DiT_I23D_PixelArt(context_dim=1024, pooling_ctx_dim=768, **kw)
        ctx = {'crossattn': synth_input('ca', (B, 256, 2048), 3).cuda(), 'vector': synth_input('v', (B, 768), 3).cuda()}
    elif which == "mvcond":
        m = dit_i23d.DiT_I23D_PixelArt_MVCond(context_dim=768, pooling_ctx_dim=768, **kw)
        ctx = {'crossattn': synth_input('ca', (B, 256, 1024), 3).cuda(), 'vector': synth_input('v', (B, 768), 3).cuda(),
               'concat': synth_input('mv', (B, 2, 256, 768), 3).cuda()}
    else:
        m = dit_i23d.DiT_I23D(context_dim=1024, **kw)
        ctx = {'crossattn': synth_input('ca', (B, 256, 2048), 3).cuda(), 'vector': synth_input('v', (B, 1024), 3).cuda()}
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (B, 12, 32, 32), 3).cuda()
    t = torch.linspace(0.1, 0.9, B).cuda()
    cc = m.prepare_context(ctx)
    y = m(x, t, context_cache=cc).clone()
    assert cc.get('akv') is not None, "the cache did not engage at this width"
    y2 = m(x, t, context_cache=cc).clone()                 # second evaluation on the same cache (what a sampler step does)
    assert torch.equal(y, y2)
    monkeypatch.setenv('LN3D_NO_APPEND_CACHE', '1')
    cc0 = m.prepare_context(ctx)
    y0 = m(x, t, context_cache=cc0)
    assert cc0.get('akv') is None
    e = rel_l2(y, y0)
    print(which, 'appended K/V cache vs full projection', e)
    assert e < 1e-5, e


@pytest.mark.parametrize("tag,hidden,depth,heads,patch", [("tiny", 128, 2, 2, 2), ("h72", 1152, 1, 16, 2), ("p1", 128, 1, 2, 1)])
def test_i23d_plain_variant_vs_reference_golden(hip_lib, tag, hidden, depth, heads, patch):
    """The plain DiT_I23D (ImageCondDiTBlock blocks: per-block adaLN, affine-free LayerNorm pre-norms, per-block attention_y_norm,
    clip_text_proj pooled token; dit/dit_i23d.py:24-170) on the I23D block machinery; h72 = 72-wide heads in padded 128-wide
    heads (the registry's 'DiT-XL/2'), p1 = patch size 1 ('DiT-B/1': 3072 + 256 tokens)."""
    from ln3diff_amd.dit.dit_i23d import DiT_I23D
    from ln3diff_amd.synth import synth_input
    g = golden('i23d_plain_' + tag)
    m = DiT_I23D(input_size=32, patch_size=patch, in_channels=4, hidden_size=hidden, depth=depth, num_heads=heads, num_classes=0,
                 learn_sigma=False, context_dim=1024, roll_out=True)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (2, 12, 32, 32), 9).cuda()
    ctx = {'crossattn': synth_input('ca', (2, 256, 2048), 9).cuda(), 'vector': synth_input('v', (2, 1024), 9).cuda()}
    y = m(x, torch.from_numpy(g['t']).cuda(), ctx).cpu()
    e = rel_l2(y, g['y'])
    print('plain DiT_I23D', tag, e)
    assert e < 2e-2, e
    # its forward_with_cfg (dit_i23d.py:156-170) with the zero unconditional half folded
    x2 = torch.cat([x, x])
    t2 = torch.from_numpy(g['t']).cuda().repeat(2)
    ctx2 = {k: torch.cat([v, torch.zeros_like(v)]) for k, v in ctx.items()}
    cc = m.prepare_context(ctx2)
    assert cc['fold'] == 2
    v = m(x2, t2, context_cache=cc)
    assert rel_l2(v[:2].cpu(), g['y']) < 2e-2


def test_i23d_multiview_variant_vs_reference_golden(hip_lib):
    """DiT_I23D_PixelArt_MVCond (CLIP spatial tokens appended, flattened multi-view DINO features cross-attended, Nk = 1024)."""
    from ln3diff_amd.dit.dit_i23d import DiT_I23D_PixelArt_MVCond
    from ln3diff_amd.synth import synth_input
    g = golden('i23d_mv_tiny')
    m = DiT_I23D_PixelArt_MVCond(input_size=32, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=0,
                                 learn_sigma=False, context_dim=768, roll_out=True, pooling_ctx_dim=768)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (2, 12, 32, 32), 5).cuda()
    ctx = {'crossattn': synth_input('ca', (2, 256, 1024), 5).cuda(), 'vector': synth_input('v', (2, 768), 5).cuda(),
           'concat': synth_input('mv', (2, 4, 256, 768), 5).cuda()}
    y = m(x, torch.from_numpy(g['t']).cuda(), ctx).cpu()
    e = rel_l2(y, g['y'])
    print('i23d MVCond tiny', e)
    assert e < 2e-2, e


def test_i23d_multiview_noclip_variant_vs_reference_golden(hip_lib):
    """DiT_I23D_PixelArt_MVCond_noClip (the registry's 'DiT-PixArt-MV-L/2'): no CLIP branch, nothing appended, Nk = 1024."""
    from ln3diff_amd.dit.dit_i23d import DiT_I23D_PixelArt_MVCond_noClip, DiT_models
    from ln3diff_amd.synth import synth_input
    assert DiT_models['DiT-PixArt-MV-L/2'].__name__ == 'DiT_L_Pixelart_MV_2_noclip'
    g = golden('i23d_mv_noclip_tiny')
    m = DiT_I23D_PixelArt_MVCond_noClip(input_size=32, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2,
                                        num_classes=0, learn_sigma=False, context_dim=768, roll_out=True, pooling_ctx_dim=768)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (2, 12, 32, 32), 5).cuda()
    y = m(x, torch.from_numpy(g['t']).cuda(), {'concat': synth_input('mv', (2, 4, 256, 768), 5).cuda()}).cpu()
    e = rel_l2(y, g['y'])
    print('i23d MVCond_noClip tiny', e)
    assert e < 2e-2, e


def test_i23d_mv_xl2_registry_vs_reference_golden(hip_lib):
    """'DiT-PixArt-MV-XL/2' (dit_i23d.py:659-664): MVCond at hidden 1152 / 16 heads - head size 72 in zero-padded 128-wide heads,
    qk-norm over the true 72 dims."""
    from ln3diff_amd.dit.dit_i23d import DiT_models
    from ln3diff_amd.synth import synth_input
    g = golden('i23d_mv_xl2')
    m = DiT_models['DiT-PixArt-MV-XL/2'](input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=768, roll_out=True,
                                         pooling_ctx_dim=768)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('x', (2, 12, 32, 32), 5).cuda()
    ctx = {'crossattn': synth_input('ca', (2, 256, 1024), 5).cuda(), 'vector': synth_input('v', (2, 768), 5).cuda(),
           'concat': synth_input('mv', (2, 4, 256, 768), 5).cuda()}
    y = m(x, torch.from_numpy(g['t']).cuda(), ctx).cpu()
    e = rel_l2(y, g['y'])
    print('i23d MV-XL/2', e)
    assert e < 2e-2, e


@pytest.mark.parametrize("tag", ['tiny', 'l'])
def test_i23d_pcd_variant_vs_reference_golden(hip_lib, tag):
    """DiT_pcd_I23D_PixelArt_MVCond / 'DiT-PixArt-MV-PCD-L' (dit_i23d.py:500-588): point tokens, Mlp embedder, no positional
    embedding, output [B, N, C]."""
    from ln3diff_amd.dit.dit_i23d import DiT_models, DiT_pcd_I23D_PixelArt_MVCond
    from ln3diff_amd.synth import synth_input
    g = golden(f'i23d_pcd_{tag}')
    kw = dict(input_size=32, num_classes=0, learn_sigma=False, in_channels=19, context_dim=768, roll_out=True, pooling_ctx_dim=768)
    m = DiT_models['DiT-PixArt-MV-PCD-L'](**kw) if tag == 'l' else \
        DiT_pcd_I23D_PixelArt_MVCond(hidden_size=128, depth=2, num_heads=2, patch_size=1, **kw)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == manifest(g)
    load_synth(m, 0)
    m = m.cuda()
    x = synth_input('pcd', (2, 768, 19), 7).cuda()
    ctx = {'crossattn': synth_input('ca', (2, 256, 1024), 5).cuda(), 'vector': synth_input('v', (2, 768), 5).cuda(),
           'concat': synth_input('mv', (2, 4, 256, 768), 5).cuda()}
    y = m(x, torch.from_numpy(g['t']).cuda(), ctx).cpu()
    assert y.shape == (2, 768, 19)
    e = rel_l2(y, g['y'])
    print('i23d pcd', tag, e)
    assert e < 2e-2, e


def test_dopri5_on_the_l2_network_vs_fp32_oracle_fixture(hip_lib):
    """the released I23D sampler (dopri5, atol 1e-6, rtol 1e-3) on DiT-PixArt-L/2 against the fp32 CPU restatement
    (tests/golden/dopri5_pixartl2_oracle.npz: 4 minutes of CPU, stored with its step sequence by make_golden_dopri5.py).
    Same initial step (Hairer's rule on the same field), same final latent to the bf16-network tolerance, both end beyond t = 1 and
    interpolate back.  The NUMBER of steps differs and cannot be made equal: the fp32 oracle's error ratio at the first step is 1e-5
    and its steps grow 9x, 3.4x, ... (5 steps, 32 evaluations); with the network evaluated in bf16 the ratio has a FLOOR of 0.02 - 0.1
    whatever the step size - state elements near zero have a tolerance of ~1e-6 (atol) while the field's bf16 rounding noise is
    ~1e-3 |v| - so the controller's growth 0.9 / ratio^0.2 stays below 2 (9 steps, 56 evaluations: +75 %, every step accepted).
    The reference evaluates its network under autocast as well; an fp32-evaluated field is the only way to the oracle's count."""
    from ln3diff_amd.synth import synth_input
    from ln3diff_amd.transport import Sampler, create_transport
    from ln3diff_amd.dit.dit_i23d import DiT_models
    g = golden('dopri5_pixartl2_oracle')
    m = DiT_models['DiT-PixArt-L/2'](input_size=32, num_classes=0, learn_sigma=False, in_channels=4, context_dim=1024, roll_out=True,
                                     pooling_ctx_dim=768)
    load_synth(m, 0)
    m = m.cuda()
    z = synth_input('z', (1, 12, 32, 32), 42)
    cond = {'crossattn': synth_input('ca', (1, 256, 2048), 42), 'vector': synth_input('v', (1, 768), 42)}
    ctx = {k: torch.cat([v, torch.zeros_like(v)], 0) for k, v in cond.items()}
    zz = torch.cat([z, z])
    cache = m.prepare_context({k: v.cuda() for k, v in ctx.items()})
    fn = Sampler(create_transport(snr_type='lognorm')).sample_ode(num_steps=50)
    out = fn(zz.cuda(), m.forward_with_cfg, return_trajectory=False, context_cache=cache, cfg_scale=4.0)[-1]
    hs = fn.last_stats
    e = rel_l2(out.cpu(), g['final'])
    print('dopri5 on DiT-PixArt-L/2: oracle nfe', int(g['nfe']), 'steps', int(g['steps']), 't_end', float(g['t_end']), '| hip nfe', hs['nfe'], 'steps',
          hs['steps'], 'accepted', hs['accepted'], 't_end', hs['t_end'], '| final rel-l2', e)
    print('  oracle (t, dt, ratio):', [tuple(round(float(v), 5) for v in r) for r in g['trace']])
    print('  hip    (t, dt, ratio):', [tuple(round(float(v), 5) for v in r) for r in hs['trace']])
    assert abs(hs['h0'] - float(g['h0'])) < 1e-3 * float(g['h0'])                      # the same first step
    assert hs['t_end'] >= 1.0 and float(g['t_end']) >= 1.0
    assert e < 1e-2
    assert hs['accepted'] == hs['steps']                                             # noise floor, not rejections
    assert int(g['nfe']) <= hs['nfe'] <= 2 * int(g['nfe'])
    assert min(r[2] for r in hs['trace']) > 50 * min(float(r[2]) for r in g['trace'])   # the floor itself
