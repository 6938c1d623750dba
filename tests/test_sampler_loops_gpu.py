"""The sampler LOOPS on the device, per step, against oracle/samplers.py run on float64 tensors - with an exact network.

The kernels under the loops (ln3d_lincomb, ln3d_axpby, ln3d_edm_euler_step, ln3d_ddpm_step, ln3d_ddim_step) are tested per element
elsewhere; the golden tests compare final latents through a bf16 DiT at rel-L2 < 1e-2, which lets every loop coefficient that moves the
result by less than ~1 % pass (a LinearMultistepSampler that is plain Euler: 6e-3).  Here the network is tests/sampler_refs.py's closed-form
rational_net, the same function on both sides, so what is compared is the host arithmetic of the loops and the kernels it feeds:

  * every trace= entry (every state of sample_ode / sample_sde), both shapes of sampler_refs.SHAPES, the draws generated once on the CPU;
  * bound per case and step: min(8 x the oracle's own fp32-vs-float64 deviation on that case and step, 1e-5), in rel-L2 AND in
    max-abs / max-abs(reference); the fp32 oracle run is computed here, on the CPU;
  * convergence orders against closed forms (no oracle): the Gaussian probability-flow solution for the sgm samplers, the linear ODE for
    the fixed-grid flow methods; each higher-order sgm sampler must beat Euler at N = 64.

Measured on the MI355X, worst over steps, cases and both shapes, device-vs-float64 [the reference's own fp32-vs-float64 deviation]:
  family (tests)   rel-L2               rel-max
  sgm    (56)      3.1e-7 [2.2e-7]      8.7e-7 [7.2e-7]
  DDPM   (4)       1.9e-7 [2.2e-7]      3.5e-7 [3.1e-7]
  DDIM   (70)      4.7e-7 [5.7e-7]      1.4e-6 [1.2e-6]
  ODE    (8)       1.1e-7 [6.0e-8]      2.9e-7 [1.6e-7]
  SDE    (68)      1.3e-7 [8.3e-8]      3.0e-7 [2.1e-7]
The device stays within 2.3 x the reference's deviation in every case; the per-case values are in profiles/sampler_loops.md, and each test
prints its own.  Orders measured: Euler 0.99, Heun 2.10, 2S 1.99, 2M 2.16, LMS 0.99 / 1.88 / 2.71 / 3.48; flow 1.02, 2.12, 2.12, 4.29.
No graph capture, no dopri5, no DiT weights in this module.
"""
import pytest
import torch

import sampler_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(t):
    return t.to(DEV)


def _report(what, worst, noise):
    fin = [nz for nz in noise if nz is not None]
    ref = (max(n[0] for n in fin), max(n[1] for n in fin)) if fin else (float('nan'),) * 2
    print(f'{what}: device-vs-float64 rel-L2 {worst[0]:.2e} rel-max {worst[1]:.2e}   [reference fp32-vs-float64 {ref[0]:.2e} {ref[1]:.2e}]')


# ------------------------------------------------------------------------------------------------------------------------ sgm samplers
def _denoiser(S, den):
    den = dict(den or {})
    scaling = {'eps': S.EpsScaling, 'v': S.VScaling, 'v_edm': S.VScalingWithEDMcNoise, 'edm': S.EDMScaling}[den.get('scaling', 'eps')]()
    if not den.get('discrete', True):
        return S.Denoiser(scaling), False
    q = den.get('quantize_c_noise', True)
    return S.DiscreteDenoiser(scaling=scaling, quantize_c_noise=q), q


def _reference_lambda(engine, additional_model_inputs):
    return lambda input, sigma, c: engine.denoiser(engine.model, input, sigma, c, **additional_model_inputs)


def _run_sgm(case, shape, labels=None, steps=R.SGM_STEPS, net_fn=None, z=None, sampler_kw=None):
    """the product's per-step states for one case of R.SGM_CASES; returns (trace, the stub network or None)"""
    from ln3diff_amd.sgm import sampling as S
    inp = R.inputs(shape)
    cls = {'euler': S.EulerEDMSampler, 'heun': S.HeunEDMSampler, 'ancestral': S.EulerAncestralSampler, 'dpmpp2s': S.DPMPP2SAncestralSampler,
           'dpmpp2m': S.DPMPP2MSampler, 'lms': S.LinearMultistepSampler}[case['kind']]
    scale = case.get('scale', R.CFG)
    guider = S.IdentityGuider() if scale is None else S.VanillaCFG(scale)
    sampler = cls(num_steps=steps, guider=guider, use_graph=False, **dict(case.get('kw', {})), **(sampler_kw or {}))
    den, index_labels = _denoiser(S, case.get('den'))
    base = net_fn or R.sgm_net(index_labels)

    def net(x, t, c, **kw):                       # a plain callable: no prepare_context, so a bound pair still runs the generic loop
        if labels is not None:
            labels.append(float(t[0]))
        return base(x, t, c)
    route, stub, kw = case['route'], None, {}
    if route == 'bind':
        arg = den.bind(net)
    elif route == 'closure':
        arg = lambda input, sigma, c: den(net, input, sigma, c)
    elif route == 'network_v':
        arg, kw = den, dict(network=net)
    else:
        stub = R.StubNetworkWithTimesteps() if route == 'fused_timesteps' else R.StubNetwork()
        if route == 'fused_network':
            arg, kw = den, dict(network=stub)
        elif route == 'fused_lambda':
            engine = type('Engine', (), {})()
            engine.denoiser, engine.model = den, stub
            arg = _reference_lambda(engine, {})
            assert S._find_pair(arg) == (den, stub)
        else:
            arg = den.bind(stub)
    cond, uc = {'crossattn': _dev(inp['c'])}, {'crossattn': _dev(inp['uc'])}
    tr = []
    y = sampler(arg, _dev(inp['z'] if z is None else z).clone(), cond, None if scale is None else uc, trace=tr,
                step_noise=lambda i: inp['noise'][i % len(inp['noise'])], **kw)       # (the order runs take more steps; their draws carry weight 0)
    assert torch.equal(y, tr[-1])
    return tr, stub


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("name", list(R.SGM_CASES))
def test_sgm_loop_per_step_vs_float64_oracle(hip_lib, name, shape):
    case = R.SGM_CASES[name]
    noise, hi, _ = R.reference_noise(R.oracle_sgm, case, shape)
    ref_labels, labels = [], []
    R.oracle_sgm(case, shape, torch.float64, labels=ref_labels)
    tr, stub = _run_sgm(case, shape, labels)
    _report(f'sgm {name} {shape}', R.check_against(tr, noise, hi, (name, shape)), noise)
    if stub is None:                              # the network saw the reference's noise labels (table indices, sigma or 0.25 log sigma), call for call
        assert len(labels) == len(ref_labels) and torch.allclose(torch.tensor(labels), torch.tensor(ref_labels), rtol=1e-6, atol=1e-6)
    else:                                         # the fused loop ran: one stub call per step
        assert len(stub.calls) == R.SGM_STEPS
    if case['route'] == 'fused_timesteps':
        # the timestep sub-network is handed the whole schedule once: the oracle's quantised index sequence, [n, 2B]; step i gets (mod_all, i)
        B = shape[0]
        assert stub.t_table.shape == (R.SGM_STEPS, 2 * B)
        assert stub.t_table[:, 0].tolist() == ref_labels and bool((stub.t_table == stub.t_table[:, :1]).all())
        assert all(c[0] is stub.mod_all and c[1] == i for i, c in enumerate(stub.calls)), stub.calls
    elif stub is not None:
        assert all(c is None for c in stub.calls)


def test_churn_window_splits_the_steps(hip_lib):
    from ln3diff_amd.sgm import sampling as S
    s = S.EulerEDMSampler(num_steps=R.SGM_STEPS, **R.CHURN)
    g = s._gammas(s.discretization(R.SGM_STEPS))
    assert [i for i in range(R.SGM_STEPS) if g[i] > 0] == [2, 3, 4, 5, 6] and R.CHURN['s_noise'] != 1.0


# ------------------------------------------------------------------------------------------------------------------------ DDPM / DDIM
def _diffusion(spec, mean='EPSILON'):
    from ln3diff_amd.guided_diffusion import gaussian_diffusion as gd
    from ln3diff_amd.guided_diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, spec), betas=gd.get_named_beta_schedule('linear', 1000),
                           model_mean_type=getattr(gd.ModelMeanType, mean), model_var_type=gd.ModelVarType.FIXED_LARGE)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("name", list(R.DDPM_CASES))
def test_ddpm_loop_per_step_vs_float64_oracle(hip_lib, name, shape):
    case, inp = R.DDPM_CASES[name], R.inputs(shape)
    noise, hi, _ = R.reference_noise(R.oracle_ddpm, case, shape)
    tr = []
    _diffusion('10').p_sample_loop(R.ContextNet(shape[1]), shape, cond=_dev(inp['dc']), noise=_dev(inp['dz']), clip_denoised=case['clip'],
                                   step_noise=lambda k: inp['noise'][k], trace=tr)
    _report(f'ddpm {name} {shape}', R.check_against(tr, noise, hi, (name, shape)), noise)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("name", list(R.DDIM_CASES))
def test_ddim_loop_per_step_vs_float64_oracle(hip_lib, name, shape):
    """the generic (no prepare_context) route: v-prediction and the mixed prediction are brought to eps by the loop itself"""
    case, inp = R.DDIM_CASES[name], R.inputs(shape)
    net = R.ContextNet(shape[1])
    noise, hi, _ = R.reference_noise(lambda c, s, d: R.oracle_ddim(c, s, d, net), case, shape)
    tr = []
    _diffusion(case['spec'], case['mean']).ddim_sample_loop(
        net, shape, cond={'c_crossattn': _dev(inp['dc'])}, noise=_dev(inp['dz']), clip_denoised=case['clip'], eta=case['eta'],
        mixing_normal=bool(case.get('mixing')), unconditional_guidance_scale=case['scale'],
        unconditional_conditioning=_dev(inp['duc']) if case.get('uc') else None, step_noise=lambda k: inp['noise'][k], trace=tr)
    _report(f'ddim {name} {shape}', R.check_against(tr, noise, hi, (name, shape)), noise)


# ------------------------------------------------------------------------------------------------------------------------ flow matching
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("method", R.ODE_METHODS)
def test_flow_ode_trajectory_vs_float64_oracle(hip_lib, method, shape):
    from ln3diff_amd.transport import Sampler, create_transport
    inp = R.inputs(shape)
    noise, hi, _ = R.reference_noise(R.oracle_ode, method, shape)
    traj = Sampler(create_transport()).sample_ode(sampling_method=method, num_steps=R.FLOW_STEPS)(_dev(inp['z']), R.velocity_field,
                                                                                                  context=_dev(inp['c']))
    assert traj.shape == (R.FLOW_STEPS, *shape)
    _report(f'ode {method} {shape}', R.check_against(list(traj), noise, hi, (method, shape)), noise)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("name", list(R.SDE_CASES))
def test_flow_sde_states_vs_float64_oracle(hip_lib, name, shape):
    """every returned state; non-finite exactly where the reference is: everywhere for SBDM (D(0) is infinite), in the last two states of
    Heun with last_step=None (the grid ends at t = 1 and the second Heun stage divides by 1 - t = 0; the reference raises nothing)"""
    from ln3diff_amd.transport import Sampler, create_transport
    case, inp = R.SDE_CASES[name], R.inputs(shape)
    noise, hi, _ = R.reference_noise(R.oracle_sde, case, shape)
    fn = Sampler(create_transport()).sample_sde(sampling_method=case['method'], diffusion_form=case['form'], diffusion_norm=R.SDE_NORM,
                                                last_step=case['last'], last_step_size=R.SDE_LAST, num_steps=R.FLOW_STEPS)
    torch.manual_seed(R.SDE_SEED)                 # the Wiener increments come from the global CPU generator, as in the reference
    xs = fn(_dev(inp['z']), R.velocity_field, context=_dev(inp['c']))
    finite = [nz is not None for nz in noise]
    if case['form'] == 'SBDM':
        assert not any(finite)
    elif case['method'] == 'Heun' and case['last'] is None:
        assert finite == [True] * (R.FLOW_STEPS - 2) + [False, False]
    else:
        assert all(finite)
    _report(f'sde {name} {shape}', R.check_against(xs, noise, hi, (name, shape)), noise)


def test_sde_constant_form_still_raises_typeerror(hip_lib):
    from ln3diff_amd.transport import Sampler, create_transport
    z = _dev(R.inputs(R.SHAPES[0])['z'])
    for method in ('Euler', 'Heun'):
        with pytest.raises(TypeError):
            Sampler(create_transport()).sample_sde(sampling_method=method, diffusion_form='constant', num_steps=3)(z, R.velocity_field)


# ------------------------------------------------------------------------------------------------------------------------ convergence orders
_ORDER_ERRS = {}


def _gaussian_errors(name):
    """the product's error against the closed-form probability-flow solution at N = 32, 64 (continuous Denoiser, EpsScaling, VanillaCFG(2),
    EDMDiscretization(0.002, 80, 7)); computed once per sampler"""
    if name not in _ORDER_ERRS:
        from ln3diff_amd.sgm import sampling as S
        case = {'euler': dict(kind='euler'), 'heun': dict(kind='heun'), 'dpmpp2s-eta0': dict(kind='dpmpp2s', kw=dict(eta=0.0)),
                'dpmpp2m': dict(kind='dpmpp2m')}.get(name) or dict(kind='lms', kw=dict(order=int(name[3:])))
        case.update(route='bind', scale=R.ORDER_CFG, den=dict(discrete=False))
        shape = R.SHAPES[0]
        inp = R.inputs(shape)
        errs = []
        for n in R.ORDER_NS:
            disc = S.EDMDiscretization(0.002, 80.0, 7.0)
            assert torch.equal(disc(n), R.edm_sigmas(n))
            tr, _ = _run_sgm(case, shape, steps=n, net_fn=R.gaussian_eps_net, sampler_kw=dict(discretization=disc))
            exact = R.gaussian_pf_solution(inp['z'], inp['c'], inp['uc'], R.ORDER_CFG, float(disc(n)[0]))
            errs.append(R.rel_l2(tr[-1], exact))
        _ORDER_ERRS[name] = errs
    return _ORDER_ERRS[name]


@pytest.mark.parametrize("name", list(R.SGM_ORDERS))
def test_sgm_sampler_converges_at_its_nominal_order(hip_lib, name):
    """p = log2(err_32 / err_64) within +-0.6 of nominal (the pre-asymptotic gap at these N: the float64 oracle gives 0.99, 2.10, 1.99, 2.16,
    0.99, 1.88, 2.71, 3.48), and every higher-order sampler beats Euler at N = 64 - what the golden tests cannot tell."""
    errs = _gaussian_errors(name)
    p = R.observed_order(*errs)
    print(f'order {name}: err32 {errs[0]:.3e} err64 {errs[1]:.3e} p {p:.2f} (nominal {R.SGM_ORDERS[name]})')
    assert abs(p - R.SGM_ORDERS[name]) <= R.ORDER_MARGIN, (name, errs, p)
    if R.SGM_ORDERS[name] > 1:
        assert errs[1] < _gaussian_errors('euler')[1], (name, errs, _gaussian_errors('euler'))


@pytest.mark.parametrize("method", list(R.FLOW_ORDERS))
def test_flow_method_converges_at_its_nominal_order(hip_lib, method):
    """the linear ODE dy/dt = -2 y + sin 3t at the two grids of FLOW_ORDER_STEPS (picked on the CPU so that the float64 oracle's error at
    the finer one is >= 100 x 1.2e-7 x |y|: the fp32 state's rounding is out of the picture); nominal orders 1, 2, 2, 4, margin as above
    (float64 oracle: 1.02, 2.12, 2.12, 4.29)"""
    from ln3diff_amd.transport import Sampler, create_transport
    y0 = R.inputs(R.SHAPES[0])['z']
    exact = R.linear_ode_exact(y0)
    errs = []
    for n in R.FLOW_ORDER_STEPS[method]:
        y = Sampler(create_transport()).sample_ode(sampling_method=method, num_steps=n)(_dev(y0), R.linear_ode_field, return_trajectory=False)[-1]
        errs.append(float((y.double().cpu() - exact).abs().max()))
    p = R.observed_order(*errs)
    print(f'order flow {method}: errors {errs[0]:.3e} {errs[1]:.3e} p {p:.2f} (nominal {R.FLOW_ORDERS[method]})')
    assert errs[1] >= 100 * 1.2e-7 * float(exact.abs().max())
    assert abs(p - R.FLOW_ORDERS[method]) <= R.ORDER_MARGIN, (method, errs, p)


# ------------------------------------------------------------------------------------------------------------------------ streams
def test_heun_loop_on_a_side_stream_gives_the_same_bits(hip_lib):
    """every wrapper launches on torch.cuda.current_stream(): the Heun loop (lincomb with 2..6 terms, churn included) inside
    torch.cuda.stream(side) equals the default-stream run bit for bit"""
    case, shape = R.SGM_CASES['heun-churn'], R.SHAPES[1]
    ref, _ = _run_sgm(case, shape)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tr, _ = _run_sgm(case, shape)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(tr) == len(ref) and all(torch.equal(a, b) for a, b in zip(tr, ref))
