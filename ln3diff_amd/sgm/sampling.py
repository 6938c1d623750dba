"""EDM-style sampling stack of the released T23D checkpoint, device-resident.

Mirrors the reference's sgm surface for this path (same class names / call signatures):
  LegacyDDPMDiscretization, EDMDiscretization   sgm/modules/diffusionmodules/discretizer.py:27-69
  Denoiser / DiscreteDenoiser + EpsScaling / VScaling / VScalingWithEDMcNoise / EDMScaling   sgm/modules/diffusionmodules/denoiser.py:13-78, denoiser_scaling.py:14-59
  VanillaCFG, IdentityGuider sgm/modules/diffusionmodules/guiders.py:24-57
  EulerEDMSampler, HeunEDMSampler, EulerAncestralSampler, DPMPP2SAncestralSampler, DPMPP2MSampler, LinearMultistepSampler
                             sgm/modules/diffusionmodules/sampling.py:82-365
The sigma tables are built on the host in fp64/fp32 exactly like the reference.

`_Sampler` owns what every sampler shares: the constructor, `_resolve` for the `denoiser` / `network=` arguments, the set-up and the loop
`for i: self._step(run, i)` with its `trace`.  A sampler is its `_step` over the shared helpers plus what `_begin` adds to the run's
state; `_EDMSampler` adds the noise injection Euler and Heun share.  Every update is ONE ln3d_lincomb launch with the guidance
x_u + s (x_c - x_u) folded into its coefficients (the updates are linear in x and the denoised halves); sigma is one number per step
(s_in * sigma in the reference), so the coefficients are host float64 scalars.
EulerEDMSampler alone has a second, fused loop (`_fast`), taken when `denoiser` is recognisably this package's DiscreteDenoiser over one
of its networks (`_find_pair`): context K/V once per call, the timestep sub-network once per schedule, per step one network call on
[uc ; c] (2B) with c_in folded into the patch-embed kernel and ONE fused kernel for denoiser-combine + CFG + Euler update
(ln3d_edm_euler_step).
"""
import dis
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops


def make_beta_schedule(n_timestep=1000, linear_start=0.00085, linear_end=0.0120):
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2
    return betas.numpy()


def generate_roughly_equally_spaced_steps(num_substeps, max_step):
    return np.linspace(max_step - 1, 0, num_substeps, endpoint=False).astype(int)[::-1]


class LegacyDDPMDiscretization:
    def __init__(self, linear_start=0.00085, linear_end=0.0120, num_timesteps=1000):
        self.num_timesteps = num_timesteps
        self.alphas_cumprod = np.cumprod(1.0 - make_beta_schedule(num_timesteps, linear_start, linear_end), axis=0)

    def get_sigmas(self, n, device="cpu"):
        if n < self.num_timesteps:
            ac = self.alphas_cumprod[generate_roughly_equally_spaced_steps(n, self.num_timesteps)]
        elif n == self.num_timesteps:
            ac = self.alphas_cumprod
        else:
            raise ValueError
        sig = torch.tensor((1 - ac) / ac, dtype=torch.float32, device=device) ** 0.5
        return torch.flip(sig, (0,))

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        s = self.get_sigmas(n, device=device)
        if do_append_zero:
            s = torch.cat([s, s.new_zeros([1])])
        return s if not flip else torch.flip(s, (0,))


class EDMDiscretization(LegacyDDPMDiscretization):
    """discretizer.py:27-39: Karras' rho schedule, sigma_i = (sigma_max^(1/rho) + i / (n - 1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho."""

    def __init__(self, sigma_min=0.002, sigma_max=80.0, rho=7.0):
        self.sigma_min, self.sigma_max, self.rho = sigma_min, sigma_max, rho

    def get_sigmas(self, n, device="cpu"):
        ramp = torch.linspace(0, 1, n, device=device)
        lo, hi = self.sigma_min ** (1 / self.rho), self.sigma_max ** (1 / self.rho)
        return (hi + ramp * (lo - hi)) ** self.rho


class VanillaCFG:
    """guiders.py:24-42: prepare_inputs doubles the batch as [uc ; c]; __call__ = x_u + scale * (x_c - x_u)."""

    def __init__(self, scale):
        self.scale = scale

    def prepare_inputs(self, x, s, c, uc):
        c_out = {}
        for k in c:
            if k in ("vector", "crossattn", "concat"):
                c_out[k] = torch.cat((uc[k], c[k]), 0)
            else:
                assert c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


class IdentityGuider:
    """guiders.py:45-57 (the reference's default when no guider_config is given): no guidance, the batch is not doubled."""
    scale = None

    def prepare_inputs(self, x, s, c, uc):
        return x, s, {k: c[k] for k in c}


def _guided_terms(guider, den, B, coef):
    """(tensors, coefficients) of coef * guider(denoised) for one ln3d_lincomb: VanillaCFG's x_u + s (x_c - x_u) as two weighted halves,
    IdentityGuider's single batch as is."""
    if getattr(guider, 'scale', None) is None:
        return [den], [coef]
    sc = float(guider.scale)
    return [den[:B], den[B:]], [coef * (1.0 - sc), coef * sc]


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


class EpsScaling:
    """denoiser_scaling.py:29-37 (the released configuration): c_skip 1, c_out -sigma, c_in 1 / sqrt(sigma^2 + 1), c_noise sigma - evaluated in
    fp32 like the reference's tensors."""

    def __call__(self, sigma):
        s = _f32(sigma)
        return 1.0, float(-s), float(1.0 / (s ** 2 + 1.0) ** 0.5), float(s)


class VScaling:
    """denoiser_scaling.py:40-48"""

    def __call__(self, sigma):
        s = _f32(sigma)
        return float(1.0 / (s ** 2 + 1.0)), float(-s / (s ** 2 + 1.0) ** 0.5), float(1.0 / (s ** 2 + 1.0) ** 0.5), float(s)


class VScalingWithEDMcNoise(VScaling):
    """denoiser_scaling.py:51-59"""

    def __call__(self, sigma):
        c_skip, c_out, c_in, _ = super().__call__(sigma)
        return c_skip, c_out, c_in, float(0.25 * _f32(sigma).log())


class EDMScaling:
    """denoiser_scaling.py:14-26"""

    def __init__(self, sigma_data=0.5):
        self.sigma_data = float(sigma_data)

    def __call__(self, sigma):
        s, d = _f32(sigma), _f32(self.sigma_data)
        return (float(d ** 2 / (s ** 2 + d ** 2)), float(s * d / (s ** 2 + d ** 2) ** 0.5), float(1 / (s ** 2 + d ** 2) ** 0.5),
                float(0.25 * s.log()))


class Denoiser:
    """denoiser.py:13-42: c_skip * input + c_out * network(c_in * input, c_noise, cond) with the scaling's four factors; no quantisation
    (the network sees c_noise as a float).  One sigma per call is assumed to be shared by the batch (every sampler of this path)."""

    def __init__(self, scaling=None):
        self.scaling = scaling or EpsScaling()

    def quantize(self, sigma):
        """(sigma the scalings are evaluated at, None): the continuous denoiser passes sigma through"""
        return float(sigma), None

    def noise_label(self, c_noise):
        return float(c_noise)

    @torch.no_grad()
    def __call__(self, network, input, sigma, cond, **additional_model_inputs):
        """`network` is a ln3diff_amd DiT (c_in rides on its patch-embed kernel) or any callable (x, t, cond) -> output on the device."""
        sig, _ = self.quantize(float(sigma.reshape(-1)[0]))
        c_skip, c_out, c_in, c_noise = self.scaling(sig)
        n = input.shape[0]
        t = torch.full((n,), self.noise_label(c_noise), device=input.device, dtype=torch.float32)
        if hasattr(network, 'prepare_context'):
            eps = network(input, t, context=cond, in_scale=torch.full((n,), c_in, device=input.device, dtype=torch.float32),
                          **additional_model_inputs)
        else:
            eps = network(input * c_in, t, cond, **additional_model_inputs)
        out = torch.empty_like(input, dtype=torch.float32)
        xin = input.contiguous().float()
        if c_skip == 1.0:
            ops.lincomb(xin, [eps.contiguous().float()], [c_out], out)
        else:
            ops.lincomb(None, [xin, eps.contiguous().float()], [c_skip, c_out], out)
        return out

    def bind(self, network, **additional_model_inputs):
        """The closure DiffusionEngineLSGM.sample hands to its sampler (sgm_DiffusionEngine.py:401-403):
        `lambda input, sigma, c: self.denoiser(self.model, input, sigma, c, **kwargs)` - as an object the sampler can look into."""
        return BoundDenoiser(self, network, **additional_model_inputs)


class DiscreteDenoiser(Denoiser):
    """denoiser.py:45-78: sigma snapped to the ascending 1000-entry table before the scalings are evaluated, c_noise replaced by its table index
    (quantize_c_noise).  With EpsScaling (the released configuration) the network's timestep is the index of the snapped sigma."""

    def __init__(self, num_idx=1000, discretization=None, scaling=None, quantize_c_noise=True):
        super().__init__(scaling)
        self.discretization = discretization or LegacyDDPMDiscretization()
        self.sigmas = self.discretization(num_idx, do_append_zero=False, flip=True)
        self.num_idx = num_idx
        self.quantize_c_noise = bool(quantize_c_noise)

    def sigma_to_idx(self, sigma):
        return int((self.sigmas - float(sigma)).abs().argmin())

    def quantize(self, sigma):
        i = self.sigma_to_idx(sigma)
        s = float(self.sigmas[i])
        return s, self.sigma_to_idx(s)

    def noise_label(self, c_noise):
        return float(self.sigma_to_idx(c_noise)) if self.quantize_c_noise else float(c_noise)

    @property
    def fused_ok(self):
        """the fused network loop of EulerEDMSampler bakes EpsScaling + the index timestep in"""
        return type(self.scaling) is EpsScaling and self.quantize_c_noise


class BoundDenoiser:
    def __init__(self, denoiser, network, **additional_model_inputs):
        self.denoiser, self.network, self.kw = denoiser, network, additional_model_inputs

    def __call__(self, input, sigma, c):
        return self.denoiser(self.network, input, sigma, c, **self.kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# Which `denoiser` arguments the sampler may look into.  The engine's closure is recognised by EQUALITY of its code with the two
# functions below, compiled by the interpreter that compiled the caller's: nothing here names an instruction.
def _engine_closures():
    """sgm_DiffusionEngine.py:401-403 as the engine writes it, and the same expression without the forwarded inputs"""
    self, additional_model_inputs = None, {}
    return (lambda input, sigma, c: self.denoiser(self.model, input, sigma, c, **additional_model_inputs),
            lambda input, sigma, c: self.denoiser(self.model, input, sigma, c))


def _code_shape(fn):
    """What must be equal between `fn` and a template: the argument layout (no *args / **kwargs, no defaults) and every instruction
    with its argument.  Free variables are renamed by order of first appearance and arguments replaced by their position, so the
    caller's spelling of `self`, `additional_model_inputs`, `input`, `sigma`, `c` does not matter; attribute names, constants, the
    number and order of calls, a store, a nested function: all of that does.  None for something that has no code."""
    code = getattr(fn, '__code__', None)
    if code is None:
        return None
    free = {}

    def norm(op, v):
        if op in dis.hasfree and isinstance(v, str):
            return ('free', free.setdefault(v, len(free)))
        if op in dis.haslocal and isinstance(v, str):
            return ('local', code.co_varnames.index(v))
        return v
    return (code.co_argcount, code.co_kwonlyargcount, code.co_flags & 0x0C,
            bool(getattr(fn, '__defaults__', None) or getattr(fn, '__kwdefaults__', None)),
            [(i.opname, norm(i.opcode, i.argval)) for i in dis.get_instructions(code)])


_ENGINE_SHAPES = [_code_shape(f) for f in _engine_closures()]


def _is_reference_lambda(fn):
    """True when `fn`'s code is the engine's closure and nothing else (sgm_DiffusionEngine.py:401-403):
    `lambda input, sigma, c: self.denoiser(self.model, input, sigma, c, **additional_model_inputs)`, with or without the `**` part,
    under any names for its arguments and closure variables (_code_shape).  Anything else - an extra argument or keyword, another
    callee, a post-processed result, a wrapped network - is another code and is run as written (generic loop)."""
    shape = _code_shape(fn)
    return shape is not None and shape in _ENGINE_SHAPES


def _find_pair(denoiser):
    """(DiscreteDenoiser, ln3diff_amd network) behind the sampler's `denoiser` argument, or (None, None).
    Recognised (nothing heuristic): `BoundDenoiser` without extra inputs; a callable that opts in with
    `_ln3d_pair = (denoiser, network)`; a closure whose CODE is exactly the reference's lambda over an engine object with
    `.denoiser` / `.model` and an empty `additional_model_inputs` (_is_reference_lambda).  Anything else runs the generic loop."""
    if isinstance(denoiser, BoundDenoiser):
        return (denoiser.denoiser, denoiser.network) if not denoiser.kw and hasattr(denoiser.network, 'prepare_context') else (None, None)
    pair = getattr(denoiser, '_ln3d_pair', None)
    if pair is not None:
        den, net = pair
        return (den, net) if isinstance(den, DiscreteDenoiser) and hasattr(net, 'prepare_context') else (None, None)
    if not _is_reference_lambda(denoiser):
        return None, None
    den = net = None
    for cell in getattr(denoiser, '__closure__', None) or ():
        try:
            o = cell.cell_contents
        except ValueError:
            return None, None
        if isinstance(getattr(o, 'denoiser', None), DiscreteDenoiser) and hasattr(getattr(o, 'model', None), 'prepare_context'):
            if den is not None:
                return None, None
            den, net = o.denoiser, o.model
        elif isinstance(o, dict):
            if o:
                return None, None                             # **additional_model_inputs forwarded to the network: not the plain pair
        else:
            return None, None                                 # a cell the reference lambda does not have
    return (den, net) if den is not None else (None, None)


def _resolve(denoiser, network):
    """(call, pair) for the sampler's `denoiser` / `network=` arguments: call is (input, sigma, c) -> denoised; pair the (denoiser, network)
    it stands for - a Denoiser given with `network=`, or what _find_pair recognises - or None for any other callable, called as given."""
    den, net = (denoiser, network) if network is not None and isinstance(denoiser, Denoiser) else _find_pair(denoiser)
    if net is None:
        return denoiser, None
    return (lambda x, s, c: den(net, x, s, c)), (den, net)


# ---------------------------------------------------------------------------------------------------------------------------------
class _Sampler:
    """What every sampler shares.  `run` is the state of one call: n, table (the fp32 sigma table with its appended zero), sigmas (the
    same as floats), call and pair (_resolve), cond, uc, step_noise, B, x (the latent, updated in place) and what `_begin` / `_loop` add."""

    def __init__(self, num_steps=250, guider=None, discretization=None, **_):
        self.num_steps = num_steps
        self.guider = guider or VanillaCFG(6.5)
        self.discretization = discretization or LegacyDDPMDiscretization()

    @torch.no_grad()
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, *, network=None, trace=None, step_noise=None):
        """The reference's call (sampling.py:109): denoiser = the engine's closure (input, sigma, c) -> denoised, or a Denoiser with
        `network=`; x [B, ...] f32 device noise; cond / uc dicts with 'crossattn'.  Returns the final latent; trace receives a copy of
        it after every step; step_noise(i) ([B, ...] tensor) replaces the device draw of step i (parity runs feed the recorded stream)."""
        call, pair = _resolve(denoiser, network)
        n = self.num_steps if num_steps is None else num_steps
        table = self.discretization(n, device="cpu")
        x = (x * float(torch.sqrt(1.0 + table[0] ** 2.0))).contiguous()          # the reference's fp32 arithmetic
        run = SimpleNamespace(n=n, table=table, sigmas=[float(v) for v in table], call=call, pair=pair, cond=cond,
                              uc=cond if uc is None else uc, step_noise=step_noise, B=x.shape[0], x=x)
        self._begin(run)
        return self._loop(run, trace)

    def _begin(self, run):
        pass

    def _loop(self, run, trace):
        run.s_in = run.x.new_ones([run.B])
        for i in range(run.n):
            self._step(run, i)
            if trace is not None:
                trace.append(run.x.clone())
        return run.x

    def _den(self, run, x, sig, keep=False):
        """the denoised batch at noise level sig as the guider laid it out ([uc ; c] for VanillaCFG); keep = it must survive the next call"""
        out = run.call(*self.guider.prepare_inputs(x, run.s_in * sig, run.cond, run.uc)).contiguous().float()
        return out.clone() if keep else out

    @staticmethod
    def _noise(run, i):
        x = run.x
        return run.step_noise(i).to(x.device).float().contiguous() if run.step_noise is not None else torch.randn(x.shape, device=x.device)

    def _euler_to(self, run, den, sig, target, out):
        """out = x + (target - sig) / sig * (x - guided(den)): guider + to_d + euler_step in one combination"""
        r = (target - sig) / sig
        k, c = _guided_terms(self.guider, den, run.B, -r)
        ops.lincomb(run.x, [run.x] + k, [r] + c, out)

    def _affine(self, run, a, terms, out):
        """out = a x + sum coef * guided(den) over terms = [(coef, den), ...]"""
        ks, cs = [run.x], [a]
        for coef, den in terms:
            k, c = _guided_terms(self.guider, den, run.B, coef)
            ks, cs = ks + k, cs + c
        ops.lincomb(None, ks, cs, out)


class _EDMSampler(_Sampler):
    """sampling.py:82-130, the reference's EDMSampler: the noise injection Euler and Heun share.  The released configuration is
    s_churn = 0 (gamma = 0: deterministic); where s_tmin <= sigma_i <= s_tmax, gamma = min(s_churn / (num_sigmas - 1), sqrt 2 - 1),
    sigma_hat = sigma_i (1 + gamma), x += randn * s_noise * sqrt(sigma_hat^2 - sigma_i^2), and the denoiser runs at sigma_hat.
    use_graph is read by EulerEDMSampler's fused loop alone (None: follow LN3D_GRAPH)."""

    def __init__(self, num_steps=250, guider=None, discretization=None, s_churn=0.0, s_tmin=0.0, s_tmax=float('inf'), s_noise=1.0,
                 use_graph=None, **_):
        super().__init__(num_steps, guider, discretization)
        self.use_graph = use_graph
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = float(s_churn), float(s_tmin), float(s_tmax), float(s_noise)

    def _gammas(self, sigmas):
        """gamma per step (sampling.py:114-118): num_sigmas = len(sigmas) counts the appended zero."""
        n = len(sigmas)
        g = min(self.s_churn / (n - 1), 2 ** 0.5 - 1)
        return [g if (self.s_churn > 0 and self.s_tmin <= float(sigmas[i]) <= self.s_tmax) else 0.0 for i in range(n - 1)]

    def _begin(self, run):
        run.gammas = self._gammas(run.sigmas)

    def _churn(self, run, i):
        """sigma_hat of step i; where gamma > 0, x += randn * s_noise * sqrt(sigma_hat^2 - sigma^2) in place (sampling.py:96-99)"""
        sig, gamma = run.sigmas[i], run.gammas[i]
        if not gamma > 0:
            return sig
        sig_hat = sig * (gamma + 1.0)
        ops.lincomb(run.x, [self._noise(run, i)], [self.s_noise * (sig_hat ** 2 - sig ** 2) ** 0.5], run.x)
        return sig_hat


class EulerEDMSampler(_EDMSampler):
    """sampling.py:82-130,211-215: EDMSampler + the Euler step.
    Fused loop (context K/V, the timestep sub-network of the whole schedule and the CFG + Euler update fused): taken under VanillaCFG
    when the `denoiser` argument is recognisably this package's DiscreteDenoiser (EpsScaling, index timesteps) over one of its networks -
    `DiscreteDenoiser.bind(network)`, the reference's own lambda over an engine, or `network=` with a DiscreteDenoiser.  Any other
    callable runs the generic loop with the same arithmetic, one closure call per step.  Under noise injection the denoiser sees
    sigma_hat quantised to its table (c_out, c_in, the timestep); the Euler step itself is on sigma_hat."""

    def _step(self, run, i):
        sig = self._churn(run, i)
        self._euler_to(run, self._den(run, run.x, sig), sig, run.sigmas[i + 1], run.x)

    def _loop(self, run, trace):
        if run.pair is None or isinstance(self.guider, IdentityGuider) or not getattr(run.pair[0], 'fused_ok', False):
            return super()._loop(run, trace)
        return self._fast(*run.pair, run, trace)

    # ------------------------------------------------------------------ the fused loop: CFG-doubled, EpsScaling
    def _prepare(self, run, den, network):
        dev = run.x.device
        ctx = torch.cat((run.uc['crossattn'], run.cond['crossattn']), 0).to(dev)      # VanillaCFG: [uc, c]
        run.cache = network.prepare_context(ctx)
        run.t_dev, run.s_dev = (torch.empty(2 * run.B, device=dev, dtype=torch.float32) for _ in range(2))
        # the denoiser sees sigma_hat = sigma (1 + gamma), quantised to its table (denoiser.py:66-78); c_in is its scaling's, at that entry
        run.quant = [den.quantize(run.sigmas[i] * (run.gammas[i] + 1.0)) for i in range(run.n)]
        run.c_in = [den.scaling(sig_q)[2] for sig_q, _ in run.quant]
        run.graph = None

    def _mod_all(self, network, quant, n, B):
        if not hasattr(network, 'prepare_timesteps'):
            return None
        # timestep-only sub-network for the whole schedule in one pass
        t_table = torch.tensor([float(q[1]) for q in quant], dtype=torch.float32)[:, None].expand(n, 2 * B)
        return network.prepare_timesteps(t_table)

    def _fused_step(self, network, run, i, mod_all):
        sig, idx = run.quant[i]
        sig_hat = self._churn(run, i)
        run.t_dev.fill_(float(idx))
        run.s_dev.fill_(run.c_in[i])
        g = run.graph
        if g is not None:
            g['mod_step']['mod'].copy_(mod_all['mod'][i * g['mrows']:(i + 1) * g['mrows']])
            g['graph'].replay()
            eps2 = g['eps']
        elif mod_all is not None:      # cfg_twins: [uc ; c] are the same latents, timestep and c_in twice (VanillaCFG.prepare_inputs)
            eps2 = network(run.x, run.t_dev, context_cache=run.cache, in_scale=run.s_dev, mod_cache=(mod_all, i), cfg_twins=True)
        else:
            eps2 = network(run.x, run.t_dev, context_cache=run.cache, in_scale=run.s_dev, cfg_twins=True)
        if run.gammas[i] > 0:
            # denoised = x - sig_q (eps_u + s (eps_c - eps_u)); d = (x - denoised) / sigma_hat; x += d (sigma_next - sigma_hat): sig_q (the table
            # entry c_out uses) and sigma_hat differ here, which the fused kernel's single sigma cannot express - one linear combination instead
            sc = float(self.guider.scale)
            r = (run.sigmas[i + 1] - sig_hat) / sig_hat * sig
            e2 = eps2.reshape(2, -1)
            ops.lincomb(run.x, [e2[0].reshape(run.x.shape), e2[1].reshape(run.x.shape)], [r * (1.0 - sc), r * sc], run.x)
        else:
            ops.edm_euler_step(run.x, eps2, sig, run.sigmas[i + 1], float(self.guider.scale))

    _capture_streams = {}                             # ONE stream per device for warm-up and capture

    @classmethod
    def _capture_stream(cls, dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        if key not in cls._capture_streams:
            cls._capture_streams[key] = torch.cuda.Stream(device=dev)
        return cls._capture_streams[key]

    def _capture(self, network, run, mod_all):
        """Optional HIP-graph replay of the network evaluation (LN3D_GRAPH=1 or use_graph=True): the ~220 launches of a forward
        are captured once and replayed per step; what changes between steps goes through fixed device buffers (x in place,
        t_dev, s_dev, the step's modulation rows copied into mod_step)."""
        dev = run.x.device
        mrows = mod_all['rows']
        mod_step = {'mod': torch.empty_like(mod_all['mod'][:mrows]), 'rows': mrows, 'epoch': mod_all.get('epoch')}
        mod_step['mod'].copy_(mod_all['mod'][:mrows])
        run.t_dev.fill_(float(run.quant[0][1]))
        run.s_dev.fill_(1.0)
        side = self._capture_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                     # warm-up outside the capture: workspaces (allocated and zeroed here, once), kernel attributes
            network(run.x, run.t_dev, context_cache=run.cache, in_scale=run.s_dev, mod_cache=(mod_step, 0), cfg_twins=True)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eps_g = network(run.x, run.t_dev, context_cache=run.cache, in_scale=run.s_dev, mod_cache=(mod_step, 0), cfg_twins=True)
        run.graph = {'graph': graph, 'eps': eps_g, 'mod_step': mod_step, 'mrows': mrows}

    def _fast(self, den, network, run, trace):
        self._prepare(run, den, network)
        mod_all = self._mod_all(network, run.quant, run.n, run.B)
        want_graph = self.use_graph if self.use_graph is not None else bool(os.environ.get('LN3D_GRAPH'))
        if want_graph and mod_all is not None and run.n > 2:
            self._capture(network, run, mod_all)
        for i in range(run.n):
            self._fused_step(network, run, i, mod_all)
            if trace is not None:
                trace.append(run.x.clone())
        return run.x


class HeunEDMSampler(_EDMSampler):
    """sampling.py:218-236: EDMSampler's step (noise injection included) + the trapezoidal correction, a second network evaluation per step
    except onto sigma = 0."""

    def _begin(self, run):
        super()._begin(run)
        run.xe = torch.empty_like(run.x)

    def _step(self, run, i):
        x, xe, nxt = run.x, run.xe, run.sigmas[i + 1]
        sig = self._churn(run, i)
        d1 = self._den(run, x, sig, keep=True)
        self._euler_to(run, d1, sig, nxt, xe)                                                    # the Euler step
        if nxt < 1e-14:
            x.copy_(xe)
        else:                                                                                    # x + dt ((x - D) / sig + (x_e - D2) / nxt) / 2
            d2 = self._den(run, xe, nxt)
            a, b = (nxt - sig) / (2.0 * sig), (nxt - sig) / (2.0 * nxt)
            k1, c1 = _guided_terms(self.guider, d1, run.B, -a)
            k2, c2 = _guided_terms(self.guider, d2, run.B, -b)
            ops.lincomb(x, [x] + k1 + [xe] + k2, [a] + c1 + [b] + c2, x)


def _ancestral(sig, nxt, eta):
    """sampling_utils.get_ancestral_step (sampling_utils.py:22-31) on scalars"""
    if not eta:
        return nxt, 0.0
    up = min(nxt, eta * (nxt ** 2 * (sig ** 2 - nxt ** 2) / sig ** 2) ** 0.5)
    return (nxt ** 2 - up ** 2) ** 0.5, up


class EulerAncestralSampler(_Sampler):
    """sampling.py:133-170, 239-246: Euler step to sigma_down, then s_noise * sigma_up of fresh noise where the next sigma is not 0
    (the reference draws at every step)."""

    def __init__(self, eta=1.0, s_noise=1.0, **kw):
        super().__init__(**kw)
        self.eta, self.s_noise = float(eta), float(s_noise)

    def _ancestral_noise(self, run, i, nxt, up):
        if nxt > 0.0:
            ops.lincomb(run.x, [self._noise(run, i)], [self.s_noise * up], run.x)

    def _step(self, run, i):
        sig, nxt = run.sigmas[i], run.sigmas[i + 1]
        down, up = _ancestral(sig, nxt, self.eta)
        self._euler_to(run, self._den(run, run.x, sig), sig, down, run.x)
        self._ancestral_noise(run, i, nxt, up)


class DPMPP2SAncestralSampler(EulerAncestralSampler):
    """sampling.py:249-287: exponential-integrator midpoint step in t = -log sigma towards sigma_down (second evaluation at sigma(t + h / 2)),
    the Euler step when sigma_down is 0, then the ancestral noise."""

    def _begin(self, run):
        run.x2 = torch.empty_like(run.x)

    def _step(self, run, i):
        sig, nxt = run.sigmas[i], run.sigmas[i + 1]
        down, up = _ancestral(sig, nxt, self.eta)
        d1 = self._den(run, run.x, sig)
        if down < 1e-14:
            self._euler_to(run, d1, sig, down, run.x)
        else:
            t, t_next = -math.log(sig), -math.log(down)
            h = t_next - t
            sm = t + 0.5 * h
            m1, m2 = math.exp(-sm) / math.exp(-t), math.expm1(-0.5 * h)
            m3, m4 = math.exp(-t_next) / math.exp(-t), math.expm1(-h)
            self._affine(run, m1, [(-m2, d1)], run.x2)                                            # x2 = m1 x - m2 D
            d2 = self._den(run, run.x2, math.exp(-sm))
            self._affine(run, m3, [(-m4, d2)], run.x)                                             # x = m3 x - m4 D2
        self._ancestral_noise(run, i, nxt, up)


class _NoDrawSampler(_Sampler):
    """the samplers that draw nothing: `step_noise` and any other keyword are accepted and ignored, like the reference's **kwargs"""

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, *, network=None, trace=None, **_):
        return super().__call__(denoiser, x, cond, uc, num_steps, network=network, trace=trace)


class DPMPP2MSampler(_NoDrawSampler):
    """sampling.py:290-365: second-order multistep - the previous step's denoised output extrapolates the current one by the ratio of the two
    log-sigma steps; the first step and the step onto sigma = 0 are first order (that last step returns the denoised sample itself)."""

    def _begin(self, run):
        run.old = None

    def _step(self, run, i):
        sig, nxt = run.sigmas[i], run.sigmas[i + 1]
        d1 = self._den(run, run.x, sig, keep=True)
        t = -math.log(sig)
        if nxt < 1e-14:                                   # t_next = +inf: mult1 = 0, mult2 = expm1(-inf) = -1
            m1, m2, h = 0.0, -1.0, float('inf')
        else:
            h = -math.log(nxt) - t
            m1, m2 = nxt / sig, math.expm1(-h)
        if run.old is None or nxt < 1e-14:
            self._affine(run, m1, [(-m2, d1)], run.x)
        else:
            r = (t + math.log(run.sigmas[i - 1])) / h
            m3, m4 = 1.0 + 1.0 / (2.0 * r), 1.0 / (2.0 * r)
            self._affine(run, m1, [(-m2 * m3, d1), (m2 * m4, run.old)], run.x)
        run.old = d1


def linear_multistep_coeff(order, t, i, j):
    """The Adams-Bashforth weight of derivative j steps back for the step t[i] -> t[i + 1]: the integral over that interval of the Lagrange
    basis polynomial through the last `order` nodes t[i], t[i - 1], ... (sampling_utils.py:7-19 evaluates the same integral with scipy's
    adaptive quadrature at epsrel 1e-4; the integrand is a polynomial of degree < order, so the closed form below is that value exactly)."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")
    nodes = [float(t[i - k]) for k in range(order)]
    basis = np.poly1d([1.0])
    for k in range(order):
        if k != j:
            basis = basis * np.poly1d([1.0, -nodes[k]]) / (nodes[j] - nodes[k])
    prim = basis.integ()
    return float(prim(float(t[i + 1])) - prim(float(t[i])))


class LinearMultistepSampler(_NoDrawSampler):
    """sampling.py:172-208: Adams-Bashforth in sigma over the last `order` derivatives d = (x - denoised) / sigma; one evaluation per step.
    Each d is one ln3d_lincomb (guidance folded in), the update another.  The weights are the closed-form integrals of the Lagrange
    basis (the reference integrates the same polynomials numerically)."""

    def __init__(self, order=4, **kw):
        super().__init__(**kw)
        self.order = int(order)

    def _begin(self, run):
        run.ds = []
        run.sig_np = np.asarray(run.table, dtype=np.float32)      # the reference's fp32 sigma table (sigmas.cpu().numpy())

    def _step(self, run, i):
        ds = run.ds
        d1 = self._den(run, run.x, run.sigmas[i])
        d = torch.empty_like(run.x) if len(ds) < self.order else ds.pop(0)
        inv = 1.0 / run.sigmas[i]
        self._affine(run, inv, [(-inv, d1)], d)
        ds.append(d)
        cur = min(i + 1, self.order)
        coeffs = [linear_multistep_coeff(cur, run.sig_np, i, j) for j in range(cur)]
        ops.lincomb(run.x, list(reversed(ds))[:cur], coeffs, run.x)
