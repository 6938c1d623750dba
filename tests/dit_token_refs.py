"""Per-token criterion for the DiT denoisers' forward() in every dispatch form (CPU only: torch and the oracle, no HIP).

The network output is [Bn, 3*C, S, S] with channel c*3 + plane; the final layer and the unpatchify are token-local, so the output
splits into one group of p*p*C numbers per (sample, plane, patch) - the TOKENS (the point-cloud variant: one group of C numbers per
point).  For every token t, with the float64 oracle (oracle/dit.py on a float64 state dict: no rounding anywhere)

    y64  the float64 oracle
    y16  the float64 oracle under operand_rounding(bf16, kernel_arith=True, unfused_norms=...): the kernels' arithmetic - bf16
         GEMM / attention operands, the attention kernels' softmax rounding, the epilogue's polynomial erf - without fp32 noise
    d_t = ||y16 - y64||_t      what bf16 operand rounding does to this token - from the oracle alone
    e_t = ||y_hip - y16||_t
    rho_t = e_t / max(d_t, 0.1 * median_t d)

and a forward passes when max_t rho_t <= CAP over EVERY token: the kernels may differ from the bf16-operand restatement by less than
operand rounding itself moves that token (what is left: summation order and rounding-boundary flips).  The oracle never folds,
caches or dedups, so every dispatch form of a network is held to the same answer; the one thing a form tells it is which qk-norms
its launches run as a pass of their own over bf16 heads (a second rounding in front of the norm: the case's `unfused_norms`, which the
GPU test checks against ops.heads_norm_fusable) - y64 never depends on the form.

The cases (network, batch, form) live here so that tests/test_dit_tokens_cpu.py can check the yardstick of every case without a GPU
and tests/test_dit_tokens_gpu.py runs exactly those cases; the oracle pair of a case is computed once per process and shared by the
forms that have the same network inputs (fold on / off, cache on / off).
"""
import functools

import torch

from conftest import load_synth
from ln3diff_amd.synth import synth_input
from oracle import dit as odit


# ------------------------------------------------------------------------------------------------ tokens
def token_groups(y, patch):
    """[Bn, 3*C, S, S] (channel c*3 + plane) -> [Bn, 3, (S/p)^2, p*p*C]: group [b, n, l] holds the numbers token n*L + l of sample b
    produces.  A point-cloud output [Bn, N, C] is [Bn, 1, N, C]."""
    if y.dim() == 3:
        return y[:, None]
    B, C3, S, _ = y.shape
    C, g = C3 // 3, S // patch
    return y.reshape(B, C, 3, g, patch, g, patch).permute(0, 2, 3, 5, 4, 6, 1).reshape(B, 3, g * g, patch * patch * C)


def token_rho(y_hip, y16, y64, patch):
    """-> (rho [Bn, planes, L], d [Bn, planes, L]) in float64; every token is in it."""
    g = lambda y: token_groups(torch.as_tensor(y).detach().double().cpu(), patch)
    g_hip, g16, g64 = g(y_hip), g(y16), g(y64)
    assert g_hip.shape == g16.shape == g64.shape, (g_hip.shape, g16.shape, g64.shape)
    d = (g16 - g64).norm(dim=-1)
    e = (g_hip - g16).norm(dim=-1)
    return e / d.clamp_min(0.1 * float(d.median())), d


def worst_token(rho):
    """(sample, plane, patch) of the largest rho and its value"""
    i = int(rho.argmax())
    P, L = rho.shape[1], rho.shape[2]
    return (i // (P * L), (i // L) % P, i % L), float(rho.flatten()[i])


def yardstick(y16, y64, patch):
    """per-token d_t / ||y64||_t: (median, max).  The allowance of the criterion is healthy while its median lies inside
    [1e-4, 2e-2] and no token is above 5e-2 - synthetic weights that blow the rounding up would otherwise inflate it."""
    g16, g64 = token_groups(y16.double(), patch), token_groups(y64.double(), patch)
    r = (g16 - g64).norm(dim=-1) / g64.norm(dim=-1)
    return float(r.median()), float(r.max())


YARD_MEDIAN, YARD_MAX = (1e-4, 2e-2), 5e-2


def to64(v):
    if isinstance(v, dict):
        return {k: to64(w) for k, w in v.items()}
    return v.double() if torch.is_tensor(v) and v.is_floating_point() else v


# ------------------------------------------------------------------------------------------------ networks
T23D_SIZES = {'small': dict(input_size=8, hidden_size=128, num_heads=2),        # N = 48: tokens % 192 != 0, unfused cross-attention
              'fused': dict(input_size=16, hidden_size=256, num_heads=4)}       # N = 192, heads * 64 = 256: LN3D_EPI_CROSS_ATTN


def build_t23d(size, depth=2):
    from ln3diff_amd.dit.dit_trilatent import DiT_TriLatent
    from ln3diff_amd.dit.dit_models_xformers import TextCondDiTBlock
    return DiT_TriLatent(patch_size=2, in_channels=4, depth=depth, num_classes=0, learn_sigma=False, context_dim=768, roll_out=True,
                         vit_blk=TextCondDiTBlock, **T23D_SIZES[size])


_I23D_KW = dict(input_size=32, in_channels=4, num_classes=0, learn_sigma=False, roll_out=True)
# class key -> (class name in ln3diff_amd.dit.dit_i23d, constructor arguments, oracle forward, context parts {name: trailing shape})
I23D_NETS = {
    'pixart': ('DiT_I23D_PixelArt', dict(patch_size=2, hidden_size=128, depth=2, num_heads=2, context_dim=1024, pooling_ctx_dim=768, **_I23D_KW),
               'i23d_forward', {'crossattn': (256, 2048), 'vector': (768,)}),
    'plain': ('DiT_I23D', dict(patch_size=2, hidden_size=128, depth=2, num_heads=2, context_dim=1024, **_I23D_KW),
              'i23d_plain_forward', {'crossattn': (256, 2048), 'vector': (1024,)}),
    'h72': ('DiT_I23D', dict(patch_size=2, hidden_size=1152, depth=1, num_heads=16, context_dim=1024, **_I23D_KW),
            'i23d_plain_forward', {'crossattn': (256, 2048), 'vector': (1024,)}),
    'mvcond': ('DiT_I23D_PixelArt_MVCond', dict(patch_size=2, hidden_size=128, depth=2, num_heads=2, context_dim=768, pooling_ctx_dim=768, **_I23D_KW),
               'i23d_mv_forward', {'crossattn': (256, 1024), 'vector': (768,), 'concat': (4, 256, 768)}),
    'noclip': ('DiT_I23D_PixelArt_MVCond_noClip', dict(patch_size=2, hidden_size=128, depth=2, num_heads=2, context_dim=768, pooling_ctx_dim=768,
                                                       **_I23D_KW),
               'i23d_mv_noclip_forward', {'concat': (4, 256, 768)}),
    't23d_pixart': ('DiT_TriLatent_PixelArt', dict(patch_size=2, hidden_size=128, depth=2, num_heads=2, context_dim=768, **_I23D_KW),
                    't23d_pixart_forward', {'crossattn': (77, 768), 'vector': (768,)}),
    'pcd': ('DiT_pcd_I23D_PixelArt_MVCond', dict(patch_size=1, hidden_size=128, depth=2, num_heads=2, context_dim=768, pooling_ctx_dim=768,
                                                 **dict(_I23D_KW, in_channels=19)),
            'i23d_pcd_forward', {'crossattn': (256, 1024), 'vector': (768,), 'concat': (4, 256, 768)}),
}


def build_i23d(net):
    from ln3diff_amd.dit import dit_i23d
    name, kw, _, _ = I23D_NETS[net]
    return getattr(dit_i23d, name)(**kw)


@functools.lru_cache(maxsize=None)
def synth_sd(kind, key):
    """the synthetic fp32 state dict of a network (seed 0, the goldens' recipe); shared, never modified"""
    m = build_t23d(key) if kind == 't23d' else build_i23d(key)
    return load_synth(m, 0)[0]


# ------------------------------------------------------------------------------------------------ T23D cases
def _t23d_case(size, form):
    """One T23D case.  Network side (what forward() is called with): x [Bx, 12, S, S], t [Bn], ctx [Bn, Lc, 768], in_scale, t_table /
    step (prepare_timesteps), cfg_twins, env.  Oracle side: x_or / t / ctx of the whole network batch.  Expected dispatch: fold, rows
    (None: no mod_cache), dedup0; okey names the oracle inputs (cases with the same okey share one oracle pair)."""
    S = T23D_SIZES[size]['input_size']
    xin = lambda B, seed: synth_input('x', (B, 12, S, S), seed)
    prompt = lambda B, L, seed: synth_input('c', (B, L, 768), seed)
    c = dict(kind='t23d', net=size, form=form, patch=2, heads=T23D_SIZES[size]['num_heads'], in_scale=None, t_table=None, step=0, cfg_twins=False,
             env=(), fold=0, rows=None, dedup0=False, unfused_norms=())
    if form == 'plain':                                  # three timesteps, three prompts
        c.update(x=xin(3, 11), t=torch.tensor([999., 500., 37.]), ctx=prompt(3, 77, 11))
    elif form in ('cfg_fold', 'cfg_nofold'):             # VanillaCFG [uc ; c] with the zero unconditional embeddings, B = 2
        x, p = xin(2, 12), prompt(2, 77, 12)
        c.update(x=torch.cat([x, x]), t=torch.tensor([900., 37., 900., 37.]), ctx=torch.cat([torch.zeros_like(p), p]), okey='cfg')
        c.update(fold=2) if form == 'cfg_fold' else c.update(env=('LN3D_NO_UC_FOLD',))
    elif form == 'oddfold':                              # the fold is not half the batch
        p = prompt(1, 77, 13)
        c.update(x=xin(3, 13), t=torch.tensor([700., 20., 310.]), ctx=torch.cat([torch.zeros_like(p), torch.zeros_like(p), p]), fold=2)
    elif form == 'modcache_shared':                      # step 1 of a 2-step table: a wrong step * rows reads step 0's row
        tab = torch.tensor([[900.] * 3, [500.] * 3])
        c.update(x=xin(3, 14), t=tab[1].clone(), ctx=prompt(3, 77, 14), t_table=tab, step=1, rows=1)
    elif form == 'modcache_ragged':
        tab = torch.tensor([[900., 800., 700.], [37., 500., 999.]])
        c.update(x=xin(3, 14), t=tab[1].clone(), ctx=prompt(3, 77, 14), t_table=tab, step=1, rows=3)
    elif form in ('twins_fold', 'twins_nofold'):         # Bx = B latents, network batch 2B, c_in given, one shared modulation row
        x, p = xin(2, 15), prompt(2, 77, 15)
        tab = torch.tensor([[900.] * 4, [500.] * 4])
        sc = torch.tensor([0.37, 0.9, 0.37, 0.9])
        c.update(x=x, x_or=torch.cat([x, x]) * sc[:, None, None, None], in_scale=sc, t=tab[1].clone(), ctx=torch.cat([torch.zeros_like(p), p]),
                 t_table=tab, step=1, rows=1, cfg_twins=True, dedup0=True, okey='twins')
        c.update(fold=2) if form == 'twins_fold' else c.update(env=('LN3D_NO_UC_FOLD',))
    elif form.startswith('lc'):                          # [zeros, c1, c2] at context lengths 1 (never folds), 64 / 65 (lpad edge), 100 (> 96 keys)
        L = int(form[2:])
        p = prompt(2, L, 16)
        c.update(x=xin(3, 16), t=torch.tensor([640., 80., 333.]), ctx=torch.cat([torch.zeros_like(p[:1]), p]), fold=0 if L < 2 else 1)
    else:
        raise KeyError(form)
    c.setdefault('x_or', c['x'])
    c['okey'] = f"t23d-{size}-{c.get('okey', form)}"
    c['id'] = f't23d-{size}-{form}'
    N = 3 * (S // 2) ** 2
    c['fused_cross'] = N % 192 == 0 and (c['heads'] * 64) % 256 == 0 and c['ctx'].shape[1] <= 96
    return c


T23D_FORMS = ('plain', 'cfg_fold', 'cfg_nofold', 'oddfold', 'modcache_shared', 'modcache_ragged', 'twins_fold', 'twins_nofold',
              'lc1', 'lc64', 'lc65', 'lc100')


# ------------------------------------------------------------------------------------------------ I23D cases
def _i23d_case(net, form):
    """One case of the I23D family.  ctx: the sgm context dict of the whole network batch; expected dispatch: fold (a TRAILING run:
    the flow-matching engine's [c, uc]), akv (appended-token K / V cache engaged), fuse_cq (cross-attention q-norm inside the query
    projection's epilogue: needs >= 1536 conditional rows, i.e. two conditional samples of 768 tokens)."""
    _, kw, _, parts = I23D_NETS[net]
    seed = 21 + sorted(I23D_NETS).index(net)
    cond = lambda B: {k: synth_input(k, (B, *shp), seed) for k, shp in parts.items()}
    xin = (lambda B: synth_input('pcd', (B, 768, 19), seed)) if net == 'pcd' else (lambda B: synth_input('x', (B, 12, 32, 32), seed))
    zero_last = lambda ctx: {k: torch.cat([v[:-1], torch.zeros_like(v[-1:])]) for k, v in ctx.items()}      # pipeline._zero_uc
    appended = net in ('pixart', 'plain', 'mvcond', 'pcd')           # the classes that append tokens to the self-attention sequence
    c = dict(kind='i23d', net=net, form=form, patch=kw['patch_size'], heads=kw['num_heads'], env=(), fold=0,
             akv=appended and kw['hidden_size'] // kw['num_heads'] == 64, fuse_cq=True)
    if form in ('default', 'cache_off'):                 # two samples, two conditionings
        c.update(x=xin(2), t=torch.tensor([0.37, 0.81]), ctx=cond(2), okey='default')
        if form == 'cache_off':
            c.update(env=('LN3D_NO_APPEND_CACHE',), akv=False)
    elif form in ('fold_on', 'fold_off'):                # [c, uc]: ONE conditional sample - below the fused q-norm's row count
        c.update(x=xin(2), t=torch.tensor([0.55, 0.55]), ctx=zero_last(cond(2)), okey='cuc')
        c.update(fold=1, fuse_cq=False) if form == 'fold_on' else c.update(env=('LN3D_NO_UC_FOLD',))
    elif form == 'fold3':                                # Bn = 3 with one trailing zero-context sample
        c.update(x=xin(3), t=torch.tensor([0.12, 0.64, 0.9]), ctx=zero_last(cond(3)), fold=1)
    else:
        raise KeyError(form)
    # qk-norms that run as a pass of their own over bf16 heads in this form (oracle.dit.operand_rounding, unfused_norms): head size
    # 72 has no fused norm at all; the cached appended rows of fewer than 6 samples x 256 tokens; one conditional sample's query
    Bn = c['t'].shape[0]
    un = set()
    if kw['hidden_size'] // kw['num_heads'] != 64:
        un.add('self_qk')
    elif c['akv'] and Bn * 256 < 1536:
        un.add('appended_k')
    if not c['fuse_cq'] and net in ('pixart', 'plain', 'h72', 'mvcond', 'pcd', 'noclip'):
        un.add('cross_q')
    c['unfused_norms'] = tuple(sorted(un))
    c['x_or'] = c['x']
    c['okey'] = f"i23d-{net}-{c.get('okey', form)}"
    c['id'] = f'i23d-{net}-{form}'
    return c


I23D_CASES = [('pixart', f) for f in ('default', 'cache_off', 'fold_on', 'fold_off', 'fold3')] + \
             [(n, 'default') for n in ('h72', 'plain', 'mvcond', 'noclip', 't23d_pixart', 'pcd')]

CASE_IDS = [f't23d-{s}-{f}' for s in T23D_SIZES for f in T23D_FORMS] + [f'i23d-{n}-{f}' for n, f in I23D_CASES]


@functools.lru_cache(maxsize=None)
def case(cid):
    kind, net, form = cid.split('-', 2)
    return _t23d_case(net, form) if kind == 't23d' else _i23d_case(net, form)


def oracle_forward(c, sd, x, t, ctx):
    """the oracle forward of the case's network on (sd, x, t, ctx) in their dtype"""
    with torch.no_grad():
        if c['kind'] == 't23d':
            return odit.t23d_forward(sd, x, t, ctx, c['heads'], c['patch'])
        fn = getattr(odit, I23D_NETS[c['net']][2])
        return fn(sd, x, t, ctx, c['heads']) if c['net'] == 'pcd' else fn(sd, x, t, ctx, c['heads'], c['patch'])


@functools.lru_cache(maxsize=None)
def _oracle64(okey, cid):
    c = case(cid)
    return oracle_forward(c, to64(synth_sd(c['kind'], c['net'])), to64(c['x_or']), to64(c['t']), to64(c['ctx']))


def rounded_oracle(cid, unfused_norms=None):
    """y16 of a case, computed afresh (the seeded-defect tests call it with oracle functions replaced)"""
    c = case(cid)
    with odit.operand_rounding(torch.bfloat16, kernel_arith=True, unfused_norms=c['unfused_norms'] if unfused_norms is None else unfused_norms):
        return oracle_forward(c, to64(synth_sd(c['kind'], c['net'])), to64(c['x_or']), to64(c['t']), to64(c['ctx']))


@functools.lru_cache(maxsize=None)
def _oracle16(okey, unfused_norms, cid):
    return rounded_oracle(cid, unfused_norms)


def oracle_pair(cid):
    """(y64, y16) of a case: the float64 oracle, and the float64 oracle with bf16 operands, the kernels' softmax rounding and the
    case's unfused qk-norms.  One computation per set of oracle inputs (and, for y16, of unfused norms): fold / no fold and the
    other forms of a batch share it."""
    c = case(cid)
    first = next(i for i in CASE_IDS if case(i)['okey'] == c['okey'])
    y64, y16 = _oracle64(c['okey'], first), _oracle16(c['okey'], c['unfused_norms'], first)
    assert y64.dtype == y16.dtype == torch.float64
    return y64, y16
