"""Exact networks and exact solutions for the sampler-loop tests (no GPU needed).

The sampler loops are host arithmetic feeding scalars to a few elementwise kernels; a bf16 network hides every coefficient that moves the
result by less than ~1 %.  Here the network is a closed form evaluated by the SAME function on both sides of a comparison, in the dtype of
its input, so that the product (fp32 on the device) and the oracle (float64 tensors on the CPU) differ by roundings only:

  rational_net      elementwise, from + * / only (no libm): nonlinear in x, depends on the noise label, the context and the sample
  StubNetwork       rational_net behind the interface EulerEDMSampler's fused loop drives (prepare_context / context_cache / in_scale)
  gaussian_eps_net  the eps of the exact denoiser of N(mu(c), s^2) data, with the closed-form probability-flow solution under CFG
  linear_ode_field  dy/dt = -2 y + sin 3t and its exact value at t = 1 (the field the dopri5 test already uses)
"""
import math

import torch


# ----------------------------------------------------------------------------------------------------------------- measures
def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def rel_max(a, b):
    """max |a - b| over max |b|: one wrong tail element shows here, where rel-L2 over the tensor hides it"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


# ----------------------------------------------------------------------------------------------------------------- inputs
def exact_context(B, seed, rows=4, cols=8):
    """[B, rows, cols] context of multiples of 1/64 in [-0.5, 0.5): with rows * cols a power of two its per-sample mean is exact in fp32 in any
    summation order, so the context term of rational_net carries no CPU-vs-device difference."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32, 32, (B, rows, cols), generator=g).float() / 64.0


def _crossattn(c):
    if isinstance(c, dict):
        c = c['crossattn'] if 'crossattn' in c else c['c_crossattn']
    return c


def context_term(c, x, gain=40.0):
    """gain * the per-sample mean of the context, broadcast over x, in x's dtype"""
    c = _crossattn(c).to(x.dtype)
    return (c.reshape(c.shape[0], -1).mean(1) * gain).view(-1, *([1] * (x.ndim - 1)))


def _label(t, x, index_labels):
    tt = t.to(x.dtype)
    if index_labels or not t.is_floating_point():             # a table index (0..999): the oracle passes it as long, the product as float
        tt = tt / 1000
    return tt.view(-1, *([1] * (x.ndim - 1)))


# ----------------------------------------------------------------------------------------------------------------- rational network
def rational_net(x, t, c, index_labels=False):
    """x (0.5 + 0.4 tt) / (1 + 0.1 x^2) + m + 0.2 tt, tt the noise label (/ 1000 when it is a table index), m = 40 * the per-sample context
    mean.  x [N, ...] any float dtype (the result has it), t [N] long or float, c the crossattn tensor [N, ...] or a dict holding it."""
    tt = _label(t, x, index_labels)
    return x * (0.5 + 0.4 * tt) / (1 + 0.1 * x * x) + context_term(c, x) + 0.2 * tt


def sgm_net(index_labels=False):
    """the (x, t, cond) callable a Denoiser / the oracle's edm_denoise_cfg calls; index_labels: the product hands the table index as a float"""
    return lambda x, t, cond, **kw: rational_net(x, t, cond, index_labels)


class ContextNet:
    """The (x, t, context=...) form GaussianDiffusion._generic_eps calls (a denoiser without prepare_context: the U-Net route), with the
    `.mix(eps, x_in, s1m)` of the LSGM mixed prediction over a fixed per-channel logit: (1 - s) s1m x + s eps, s = sigmoid(logit), in place."""

    def __init__(self, channels):
        self.mixing_logit = torch.linspace(-1.5, 1.0, channels).view(1, channels, 1, 1)

    def __call__(self, x, t, context=None):
        return rational_net(x, t, context)

    def mix_coef(self, like):
        return torch.sigmoid(self.mixing_logit.double()).to(dtype=like.dtype, device=like.device)

    def mix(self, eps, x_in, s1m):
        s = self.mix_coef(eps)
        eps.copy_((1 - s) * (s1m * x_in) + s * eps)
        return eps


def velocity_field(x, t, **kw):
    """model_fn(x, t, **kw) for transport: rational_net as a velocity field; kw['context'] (optional) is its context"""
    c = kw.get('context')
    return rational_net(x, t, c if c is not None else torch.zeros(x.shape[0], 1, dtype=x.dtype, device=x.device))


class StubNetwork:
    """What EulerEDMSampler._fast needs of a network: prepare_context(ctx) and __call__(x, t, context_cache=, in_scale=, mod_cache=None,
    cfg_twins=False), which evaluates rational_net on cat([x, x]) * in_scale (the [uc ; c] twins of VanillaCFG) with the index label."""

    def __init__(self):
        self.calls = []

    def prepare_context(self, ctx):
        return {'ctx': ctx}

    def __call__(self, x, t, context_cache=None, in_scale=None, mod_cache=None, cfg_twins=False):
        assert cfg_twins and context_cache is not None and in_scale is not None
        self.calls.append(mod_cache)
        xin = torch.cat([x, x]) * in_scale.view(-1, *([1] * (x.ndim - 1)))
        return rational_net(xin, t, context_cache['ctx'], index_labels=True)


class StubNetworkWithTimesteps(StubNetwork):
    """+ prepare_timesteps(t_table): records the table it is handed; __call__ records each step's (mod_all, i) in self.calls"""

    def __init__(self):
        super().__init__()
        self.t_table = None

    def prepare_timesteps(self, t_table):
        self.t_table = t_table.clone()
        self.mod_all = {'table': self.t_table}
        return self.mod_all


# ----------------------------------------------------------------------------------------------------------------- Gaussian data
GAUSS_S = 0.5          # the data's standard deviation


def gaussian_eps_net(x_scaled, t, cond, s=GAUSS_S):
    """The network whose EpsScaling denoiser is exact for N(mu(c), s^2) data: with sigma = t (continuous Denoiser: c_noise = sigma),
    x = x_scaled * sqrt(sigma^2 + 1) (undoing c_in), D = (s^2 x + sigma^2 mu) / (s^2 + sigma^2) = x - sigma eps, so
    eps = sigma (x - mu) / (s^2 + sigma^2).  mu(c) = context_term(c)."""
    sig = t.to(x_scaled.dtype).view(-1, *([1] * (x_scaled.ndim - 1)))
    x = x_scaled * (sig * sig + 1) ** 0.5
    return sig * (x - context_term(cond, x_scaled)) / (s * s + sig * sig)


def gaussian_pf_solution(z, cond, uc, scale, sigma0, sigma=0.0, s=GAUSS_S):
    """The probability-flow ODE dx/dsigma = (x - D_g) / sigma of that denoiser under CFG scale g, D_g = D_u + g (D_c - D_u), is linear with
    mean mu_g = mu_u + g (mu_c - mu_u): x(sigma) = mu_g + (x0 - mu_g) sqrt((s^2 + sigma^2) / (s^2 + sigma0^2)), x0 = z sqrt(1 + sigma0^2).
    Evaluated in float64."""
    z = z.double()
    mu_u, mu_c = context_term(uc, z), context_term(cond, z)
    mu = mu_u + scale * (mu_c - mu_u)
    x0 = z * math.sqrt(1.0 + sigma0 ** 2)
    return mu + (x0 - mu) * math.sqrt((s * s + sigma * sigma) / (s * s + sigma0 * sigma0))


# ----------------------------------------------------------------------------------------------------------------- linear ODE
def linear_ode_field(y, t, **kw):
    """dy/dt = -2 y + sin 3t"""
    return -2.0 * y + torch.sin(3.0 * t.to(y.dtype)).view(-1, *([1] * (y.ndim - 1)))


def linear_ode_exact(y0, t=1.0):
    """y(t) = (y0 + 3/13) e^{-2t} + (2 sin 3t - 3 cos 3t) / 13"""
    return (y0.double() + 3.0 / 13.0) * math.exp(-2.0 * t) + (2.0 * math.sin(3.0 * t) - 3.0 * math.cos(3.0 * t)) / 13.0


# ================================================================================================================= the loop cases
# One table for tests/test_sampler_refs_cpu.py (the oracle on fp32 and on float64 tensors: the reference's own rounding noise per case and
# step) and tests/test_sampler_loops_gpu.py (the product on the device against the float64 oracle, bounded by BOUND_FACTOR x that noise).
SHAPES = [(3, 3, 5, 7), (2, 12, 32, 32)]     # odd batch + 315 elements (every vector tail, a CFG half that is no multiple of 4); the latent shape
SGM_STEPS, DIFF_STEPS, FLOW_STEPS = 8, 10, 9  # flow: 9 grid points = 8 steps
CFG = 3.0
BOUND_FACTOR, BOUND_CAP = 8.0, 1e-5
CHURN = dict(s_churn=2.0, s_tmin=0.6, s_tmax=5.0, s_noise=1.1)      # gamma 0.25 on steps 2..6 of the 8-step legacy table, none on 0, 1, 7
SDE_NORM, SDE_LAST = 0.7, 0.04

_INPUTS = {}


def inputs(shape):
    """z, the per-step draws, cond / uc contexts: generated once per shape on the CPU (fp32 values), fed to both sides"""
    if shape not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + shape[0])
        z = torch.randn(shape, generator=g)
        # DDPM / DDIM: z / 4 and contexts / 1024 (powers of two: the context mean stays exact).  Their first steps multiply x by
        # sqrt(1 / alphas_cumprod) = 158 and CFG over a clipped and an unclipped half expands errors 2.6 x per step, so the reference's own
        # fp32 noise in the max norm grows with |x| and with the context gap; these inputs keep it lowest (see profiles/sampler_loops.md)
        _INPUTS[shape] = dict(z=z, noise=[torch.randn(shape, generator=g) for _ in range(DIFF_STEPS)],
                              c=exact_context(shape[0], 7), uc=exact_context(shape[0], 8),
                              dz=z / 4, dc=exact_context(shape[0], 7) / 1024, duc=exact_context(shape[0], 8) / 1024)
    return _INPUTS[shape]


def _sgm_cases():
    c = {}
    for route in ('bind', 'closure', 'network_v'):
        c['euler-' + route] = dict(kind='euler', route=route)
    c['euler-network_v']['den'] = dict(scaling='v')
    c['euler-identity'] = dict(kind='euler', route='closure', scale=None)
    c['euler-churn'] = dict(kind='euler', route='closure', kw=CHURN)
    c['euler-vscaling'] = dict(kind='euler', route='bind', den=dict(scaling='v'))
    c['euler-vscaling-edmcnoise'] = dict(kind='euler', route='bind', den=dict(scaling='v_edm', quantize_c_noise=False))
    c['euler-edmscaling-continuous'] = dict(kind='euler', route='bind', den=dict(scaling='edm', discrete=False))
    c['fused-stub'] = dict(kind='euler', route='fused_bind')
    c['fused-stub-churn'] = dict(kind='euler', route='fused_network', kw=CHURN)
    c['fused-reference-lambda'] = dict(kind='euler', route='fused_lambda')
    c['fused-prepare-timesteps'] = dict(kind='euler', route='fused_timesteps', kw=CHURN)
    c['heun'] = dict(kind='heun', route='bind')
    c['heun-churn'] = dict(kind='heun', route='closure', kw=CHURN)
    c['heun-identity'] = dict(kind='heun', route='closure', scale=None)
    for kind in ('ancestral', 'dpmpp2s'):
        for eta, sn in ((1.0, 1.0), (0.6, 1.1), (0.0, 1.0), (1.5, 1.0)):       # eta > 1: the only place get_ancestral_step's min(sigma_to, .) binds
            c[f'{kind}-eta{eta}-sn{sn}'] = dict(kind=kind, route='closure', kw=dict(eta=eta, s_noise=sn))
    c['dpmpp2m'] = dict(kind='dpmpp2m', route='bind')
    for k in (1, 2, 3, 4):
        c[f'lms{k}'] = dict(kind='lms', route='bind', kw=dict(order=k))
    return c


SGM_CASES = _sgm_cases()
DDPM_CASES = {f'ddpm10-clip{int(cl)}': dict(clip=cl) for cl in (False, True)}
DDIM_CASES = {f'{spec}-{mt}-eta{eta}-s{sc}-clip{int(cl)}': dict(spec=spec, mean=mt, eta=eta, scale=sc, clip=cl)
              for spec in ('10', 'ddim10') for mt in ('EPSILON', 'V') for eta in (0.0, 0.5) for sc in (1.0, 3.0) for cl in (False, True)}
DDIM_CASES['ddim10-EPSILON-eta0.5-s3.0-uc-given'] = dict(spec='ddim10', mean='EPSILON', eta=0.5, scale=3.0, clip=False, uc=True)
DDIM_CASES['10-V-eta0.5-s3.0-mixing'] = dict(spec='10', mean='V', eta=0.5, scale=3.0, clip=True, mixing=True)
DDIM_CASES['ddim10-EPSILON-eta0.0-s1.0-mixing'] = dict(spec='ddim10', mean='EPSILON', eta=0.0, scale=1.0, clip=False, mixing=True)
ODE_METHODS = ('euler', 'heun', 'midpoint', 'rk4')
SDE_FORMS = ('sigma', 'linear', 'decreasing', 'inccreasing-decreasing')
SDE_CASES = {f'{m}-{f}-{l}': dict(method=m, form=f, last=l) for m in ('Euler', 'Heun') for f in SDE_FORMS for l in ('Mean', 'Euler', 'Tweedie', None)}
SDE_CASES['Euler-SBDM-Mean'] = dict(method='Euler', form='SBDM', last='Mean')
SDE_CASES['Heun-SBDM-Mean'] = dict(method='Heun', form='SBDM', last='Mean')


def oracle_sgm(case, shape, dtype, labels=None):
    """the per-step states of oracle/samplers.py for one SGM case, its tensors in `dtype`; labels: a list that receives the noise label of
    every network call"""
    from oracle import samplers as O
    inp = inputs(shape)
    fn = {'euler': O.edm_euler_sample, 'heun': O.edm_heun_sample, 'ancestral': O.euler_ancestral_sample, 'dpmpp2s': O.dpmpp2s_ancestral_sample,
          'dpmpp2m': O.dpmpp2m_sample, 'lms': O.linear_multistep_sample}[case['kind']]

    def net(x, t, c):
        if labels is not None:
            labels.append(float(t[0]))
        return rational_net(x, t, c)
    kw = dict(case.get('kw', {}))
    if case['kind'] in ('euler', 'heun', 'ancestral', 'dpmpp2s'):
        kw['step_noise'] = lambda i: inp['noise'][i]
    tr = []
    fn(net, inp['z'].to(dtype), {'crossattn': inp['c'].to(dtype)}, {'crossattn': inp['uc'].to(dtype)}, num_steps=SGM_STEPS,
       scale=case.get('scale', CFG), trace=tr, **kw, **case.get('den', {}))
    return tr


def _tables(spec):
    from oracle import samplers as O
    return O.SpacedTables(spec)


def oracle_ddpm(case, shape, dtype):
    from oracle import samplers as O
    inp = inputs(shape)
    tr = []
    O.ddpm_p_sample_loop(lambda x, t, c: rational_net(x, t, c), inp['dz'].to(dtype), inp['noise'], inp['dc'].to(dtype), _tables('10'),
                         clip_denoised=case['clip'], trace=tr)
    return tr


def oracle_ddim(case, shape, dtype, mixnet=None):
    from oracle import samplers as O
    inp = inputs(shape)
    tab = _tables(case['spec'])
    mixnet = mixnet or ContextNet(shape[1])

    def to_eps(e, xin, tin):
        ab = torch.tensor(tab.alphas_cumprod, dtype=torch.float32)[tin].view(-1, *([1] * (xin.ndim - 1)))
        if case['mean'] == 'V':
            e = torch.sqrt(ab) * e + torch.sqrt(1 - ab) * xin
        if case.get('mixing'):
            s = mixnet.mix_coef(e)
            e = (1 - s) * (torch.sqrt(1 - ab) * xin) + s * e
        return e
    tr = []
    O.ddim_sample_loop(lambda x, t, c: rational_net(x, t, c), inp['dz'].to(dtype), inp['dc'].to(dtype), tab, eta=case['eta'], cfg_scale=case['scale'],
                       ucond=inp['duc'].to(dtype) if case.get('uc') else None, noises=inp['noise'], clip_denoised=case['clip'], trace=tr, to_eps=to_eps)
    return tr


def oracle_ode(method, shape, dtype):
    from oracle import samplers as O
    inp = inputs(shape)
    tr = []
    O.flow_ode_sample(velocity_field, inp['z'].to(dtype), num_steps=FLOW_STEPS, method=method, trace=tr, context=inp['c'].to(dtype))
    return tr


SDE_SEED = 4321


def oracle_sde(case, shape, dtype):
    """the Wiener increments come from the global CPU generator, as in the reference: reseeded here, and by the caller of the product"""
    from oracle import samplers as O
    inp = inputs(shape)
    torch.manual_seed(SDE_SEED)
    return O.flow_sde_sample(velocity_field, inp['z'].to(dtype), num_steps=FLOW_STEPS, method=case['method'], diffusion_form=case['form'],
                             diffusion_norm=SDE_NORM, last_step=case['last'], last_step_size=SDE_LAST, context=inp['c'].to(dtype))


def reference_noise(run, *a):
    """[(rel-L2, rel-max)] per step of the oracle on fp32 tensors against the oracle on float64 tensors, and the float64 states.  A step
    whose float64 state is non-finite yields None."""
    lo, hi = run(*a, torch.float32), run(*a, torch.float64)
    assert len(lo) == len(hi) and all(h.dtype == torch.float64 and l.dtype == torch.float32 for l, h in zip(lo, hi))
    return [(rel_l2(l, h), rel_max(l, h)) if bool(torch.isfinite(h).all()) else None for l, h in zip(lo, hi)], hi, lo


def check_against(states, noise, hi, what):
    """every state of `states` (device or CPU tensors) against the float64 oracle `hi`: non-finite exactly where it is, and within
    min(BOUND_FACTOR x the reference's own noise of that step, BOUND_CAP) in both norms.  Returns the worst (rel-L2, rel-max)."""
    assert len(states) == len(hi), (what, len(states), len(hi))
    worst = [0.0, 0.0]
    for i, (s, h, nz) in enumerate(zip(states, hi, noise)):
        s = s.detach().cpu()
        assert s.shape == h.shape and s.dtype == torch.float32, (what, i, s.shape, s.dtype)
        assert torch.equal(torch.isfinite(s), torch.isfinite(h)), (what, i, 'finite where the reference is not, or the reverse')
        if nz is None:
            continue
        e = (rel_l2(s, h), rel_max(s, h))
        for k in (0, 1):
            bound = min(BOUND_FACTOR * nz[k], BOUND_CAP)              # never above the cap: where 8 x the noise would be, the cap is the bound
            assert e[k] <= bound, (what, 'step', i, ('rel-L2', 'rel-max')[k], e[k], 'bound', bound)
            worst[k] = max(worst[k], e[k])
    return tuple(worst)


# ----------------------------------------------------------------------------------------------------------------- convergence
def edm_sigmas(n, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """Karras' rho schedule (discretizer.py:27-39) + the appended zero, fp32 like the reference's"""
    ramp = torch.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return torch.cat([(hi + ramp * (lo - hi)) ** rho, torch.zeros(1)])


ORDER_CFG, ORDER_NS, ORDER_MARGIN = 2.0, (32, 64), 0.6
SGM_ORDERS = {'euler': 1, 'heun': 2, 'dpmpp2s-eta0': 2, 'dpmpp2m': 2, 'lms1': 1, 'lms2': 2, 'lms3': 3, 'lms4': 4}
FLOW_ORDERS = {'euler': 1, 'heun': 2, 'midpoint': 2, 'rk4': 4}
FLOW_ORDER_STEPS = {'euler': (17, 33), 'heun': (9, 17), 'midpoint': (9, 17), 'rk4': (5, 9)}       # grid points; see test_sampler_refs_cpu.py


def observed_order(err_coarse, err_fine):
    return math.log2(err_coarse / err_fine)


def oracle_gaussian(name, n, shape=SHAPES[0], dtype=torch.float64):
    """the oracle's final state on gaussian_eps_net (continuous Denoiser, EpsScaling, VanillaCFG(ORDER_CFG), EDM schedule of n sigmas) and the
    closed form it approximates"""
    from oracle import samplers as O
    inp = inputs(shape)
    fn, kw = {'euler': (O.edm_euler_sample, {}), 'heun': (O.edm_heun_sample, {}), 'dpmpp2s-eta0': (O.dpmpp2s_ancestral_sample, dict(eta=0.0)),
              'dpmpp2m': (O.dpmpp2m_sample, {}), 'lms1': (O.linear_multistep_sample, dict(order=1)),
              'lms2': (O.linear_multistep_sample, dict(order=2)), 'lms3': (O.linear_multistep_sample, dict(order=3)),
              'lms4': (O.linear_multistep_sample, dict(order=4))}[name]
    y = fn(gaussian_eps_net, inp['z'].to(dtype), {'crossattn': inp['c'].to(dtype)}, {'crossattn': inp['uc'].to(dtype)}, num_steps=n,
           scale=ORDER_CFG, sigmas=edm_sigmas, discrete=False, **kw)
    return y, gaussian_pf_solution(inp['z'], inp['c'], inp['uc'], ORDER_CFG, float(edm_sigmas(n)[0]))
