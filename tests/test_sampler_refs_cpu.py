"""The references of tests/test_sampler_loops_gpu.py, checked on the CPU (no GPU, no product code).

1. oracle/samplers.py on fp32 tensors and on float64 tensors, with the closed-form rational_net, agrees per step: the fp32-vs-float64
   deviation of every case and step is the reference's own rounding noise.  The GPU module bounds the device result by BOUND_FACTOR (8) x
   that deviation, clamped at BOUND_CAP (1e-5), so here it has to be small: 8 x it must stay below the cap in rel-L2 everywhere, and in
   rel-max everywhere but DDPM / DDIM, where it sits at the cap (see test_ddpm_ddim_oracle_fp32_vs_float64_per_step).  Measured worst deviation per family (rel-L2 /
   rel-max, both shapes): sgm 2.2e-7 / 7.4e-7, DDPM 2.2e-7 / 3.1e-7, DDIM 5.6e-7 / 1.2e-6, flow ODE 6.0e-8 / 1.6e-7, flow SDE 8.3e-8 / 2.1e-7.
2. The float64 oracle on the exact Gaussian denoiser converges to the closed-form probability-flow solution at each sampler's nominal
   order; the float64 fixed-grid flow oracle converges to the linear ODE's exact value at orders 1, 2, 2, 4.
"""
import math

import pytest
import torch

import sampler_refs as R


def _family(run, cases, cap_norms=(0, 1)):
    """every case on both shapes; asserts BOUND_FACTOR x the noise <= BOUND_CAP in the norms of cap_norms (0 rel-L2, 1 rel-max)"""
    worst, over = (0.0, 0.0), 0
    for shape in R.SHAPES:
        for name, case in cases.items():
            noise, hi, lo = R.reference_noise(run, case, shape)
            finite = [nz for nz in noise if nz is not None]
            # the fp32 oracle against the float64 one, by the rule the device is held to (finite in the same places; here factor 1 of itself)
            R.check_against(lo, noise, hi, (name, shape))
            for k in cap_norms:
                assert all(R.BOUND_FACTOR * nz[k] <= R.BOUND_CAP for nz in finite), (name, shape, noise)
            over += any(R.BOUND_FACTOR * nz[1] > R.BOUND_CAP for nz in finite)
            if finite:
                worst = (max(worst[0], max(nz[0] for nz in finite)), max(worst[1], max(nz[1] for nz in finite)))
            yield name, shape, noise, hi
    print('worst fp32-vs-float64 deviation (rel-L2, rel-max):', worst, '; cases whose 8 x rel-max noise exceeds the cap:', over)


def test_sgm_oracle_fp32_vs_float64_per_step():
    for name, shape, noise, hi in _family(R.oracle_sgm, R.SGM_CASES):
        assert len(hi) == R.SGM_STEPS and all(nz is not None for nz in noise), name
    # the churn window really splits the steps, the cases really differ
    from oracle import samplers as O
    sig = O.legacy_ddpm_sigmas(R.SGM_STEPS)
    churned = [i for i in range(R.SGM_STEPS) if R.CHURN['s_tmin'] <= float(sig[i]) <= R.CHURN['s_tmax']]
    assert 0 < len(churned) < R.SGM_STEPS and churned == [2, 3, 4, 5, 6]
    fin = {n: R.oracle_sgm(c, R.SHAPES[0], torch.float64)[-1] for n, c in R.SGM_CASES.items()}
    for a, b in (('euler-bind', 'heun'), ('euler-bind', 'dpmpp2m'), ('euler-bind', 'lms2'), ('lms2', 'lms3'), ('lms3', 'lms4'),
                 ('euler-bind', 'euler-churn'), ('euler-bind', 'euler-identity'), ('euler-bind', 'euler-vscaling'),
                 ('ancestral-eta1.0-sn1.0', 'ancestral-eta0.6-sn1.1'), ('dpmpp2s-eta1.0-sn1.0', 'dpmpp2s-eta0.0-sn1.0')):
        assert R.rel_l2(fin[a], fin[b]) > 10 * R.BOUND_CAP, (a, b)           # apart by far more than any bound of the GPU module
    assert R.rel_l2(fin['euler-bind'], fin['lms1']) < 1e-12          # LMS-1 is Euler
    assert R.rel_l2(fin['euler-bind'], fin['ancestral-eta0.0-sn1.0']) < 1e-12


def test_ddpm_ddim_oracle_fp32_vs_float64_per_step():
    # rel-max: 8 x the noise of the CFG-3 cases sits at the cap (measured 9.8e-6; with z, contexts of order 1 it is 3.6e-5) - CFG multiplies the
    # roundings of the two halves by 2 and 3 at every step, and the max over 24576 elements collects them.  check_against clamps the bound at
    # the cap, so nothing is ever compared more loosely than 1e-5; only the rel-L2 condition is asserted for this family.
    for name, shape, noise, hi in _family(R.oracle_ddpm, R.DDPM_CASES, cap_norms=(0,)):
        assert len(hi) == R.DIFF_STEPS
    for name, shape, noise, hi in _family(R.oracle_ddim, R.DDIM_CASES, cap_norms=(0,)):
        assert len(hi) == R.DIFF_STEPS
    f = lambda n: R.oracle_ddim(R.DDIM_CASES[n], R.SHAPES[0], torch.float64)[-1]
    base = f('10-EPSILON-eta0.0-s1.0-clip0')
    for other in ('ddim10-EPSILON-eta0.0-s1.0-clip0', '10-V-eta0.0-s1.0-clip0', '10-EPSILON-eta0.5-s1.0-clip0', '10-EPSILON-eta0.0-s3.0-clip0',
                  '10-EPSILON-eta0.0-s1.0-clip1'):
        assert R.rel_l2(f(other), base) > 1e-3, other
    assert R.rel_l2(f('ddim10-EPSILON-eta0.5-s3.0-uc-given'), f('ddim10-EPSILON-eta0.5-s3.0-clip0')) > 1e-3
    assert R.rel_l2(f('ddim10-EPSILON-eta0.0-s1.0-mixing'), f('ddim10-EPSILON-eta0.0-s1.0-clip0')) > 1e-3


def test_flow_oracle_fp32_vs_float64_per_step():
    for name, shape, noise, hi in _family(lambda m, s, d: R.oracle_ode(m, s, d), {m: m for m in R.ODE_METHODS}):
        assert len(hi) == R.FLOW_STEPS
    for name, shape, noise, hi in _family(R.oracle_sde, R.SDE_CASES):
        case = R.SDE_CASES[name]
        assert len(hi) == R.FLOW_STEPS
        finite = [nz is not None for nz in noise]
        if case['form'] == 'SBDM':                                    # D(0) is infinite: nothing finite from the first step on
            assert not any(finite), name
        elif case['method'] == 'Heun' and case['last'] is None:       # the grid ends at t = 1: the last Heun stage divides by 1 - t = 0
            assert finite == [True] * (R.FLOW_STEPS - 2) + [False, False], name
        else:
            assert all(finite), name


@pytest.mark.parametrize("name", list(R.SGM_ORDERS))
def test_float64_oracle_converges_to_the_gaussian_closed_form(name):
    errs = []
    for n in R.ORDER_NS:
        y, exact = R.oracle_gaussian(name, n)
        errs.append(R.rel_l2(y, exact))
    p = R.observed_order(*errs)
    print(name, 'errors', errs, 'order', p)
    assert abs(p - R.SGM_ORDERS[name]) <= R.ORDER_MARGIN, (name, errs, p)
    assert errs[1] > 1e-5                                             # far above the fp32 floor: the device run measures the same thing
    if R.SGM_ORDERS[name] > 1:
        y, exact = R.oracle_gaussian('euler', R.ORDER_NS[1])
        assert errs[1] < R.rel_l2(y, exact), name


@pytest.mark.parametrize("method", list(R.FLOW_ORDERS))
def test_float64_flow_oracle_converges_to_the_linear_ode(method):
    """The step counts of FLOW_ORDER_STEPS were picked here: the error at the finer one must stay >= 100 x 1.2e-7 x |y| so that the fp32
    device run measures the method's error and not its rounding."""
    from oracle import samplers as O
    y0 = R.inputs(R.SHAPES[0])['z'].double()
    exact = R.linear_ode_exact(y0)
    errs = []
    for n in R.FLOW_ORDER_STEPS[method]:
        y = O.flow_ode_sample(R.linear_ode_field, y0, num_steps=n, method=method)
        errs.append(float((y - exact).abs().max()))
    p = R.observed_order(*errs)
    print(method, 'errors', errs, 'order', p)
    assert errs[1] >= 100 * 1.2e-7 * float(exact.abs().max()), (method, errs)
    assert abs(p - R.FLOW_ORDERS[method]) <= R.ORDER_MARGIN, (method, errs, p)


def test_exact_pieces():
    x = torch.randn(4, 3, 5, 7)
    c = R.exact_context(4, 3)
    t = torch.tensor([999, 500, 20, 0])
    a, b = R.rational_net(x, t, c), R.rational_net(x, t.float(), {'crossattn': c}, index_labels=True)
    assert torch.equal(a, b) and a.dtype == torch.float32
    assert R.rational_net(x.double(), t, c).dtype == torch.float64
    assert float(c.reshape(4, -1).mean(1).abs().min()) > 0 and torch.equal(c.flip(1, 2).reshape(4, -1).mean(1), c.reshape(4, -1).mean(1))
    assert not torch.allclose(R.rational_net(2 * x, t, c) - R.context_term(c, x), 2 * (a - R.context_term(c, x)))       # nonlinear in x
    # the Gaussian denoiser: D(x, sigma) = x - sigma eps is the posterior mean
    sig = torch.full((4,), 3.0, dtype=torch.float64)
    xd = x.double()
    eps = R.gaussian_eps_net(xd / math.sqrt(10.0), sig, c)
    mu = R.context_term(c, xd)
    assert torch.allclose(xd - 3.0 * eps, (0.25 * xd + 9.0 * mu) / 9.25, rtol=1e-12, atol=1e-12)
    # the closed form solves dx/dsigma = (x - D_g) / sigma: check by a centred difference
    z, uc, g, s0 = x.double(), R.exact_context(4, 5), 2.0, 80.0
    h, sg = 1e-4, 1.5
    xs = [R.gaussian_pf_solution(z, c, uc, g, s0, sigma=v) for v in (sg - h, sg, sg + h)]
    sv = torch.full((4,), sg, dtype=torch.float64)
    eu, ec = (R.gaussian_eps_net(xs[1] / math.sqrt(sg * sg + 1), sv, cc) for cc in (uc, c))
    assert torch.allclose((xs[2] - xs[0]) / (2 * h), eu + g * (ec - eu), rtol=1e-6, atol=1e-6)
    # the linear ODE's exact solution, the same way
    y0 = torch.randn(5, 2).double()
    tv = torch.full((5,), 0.4, dtype=torch.float64)
    d = (R.linear_ode_exact(y0, 0.4 + h) - R.linear_ode_exact(y0, 0.4 - h)) / (2 * h)
    assert torch.allclose(d, R.linear_ode_field(R.linear_ode_exact(y0, 0.4), tv), rtol=1e-6, atol=1e-6)
    assert torch.allclose(R.linear_ode_exact(y0, 0.0), y0)
