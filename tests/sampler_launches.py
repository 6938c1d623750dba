"""What the sgm sampler loops LAUNCH, recorded on the CPU (no GPU, no library): every case of sampler_refs.SGM_CASES runs with
ops.lincomb and ops.edm_euler_step replaced by stand-ins that log the call and compute the same combination with torch on the host.

The log of one run, in order (state values are left out: no coefficient depends on them, so the log is the same on every CPU):
  ['lincomb', y is None, y is out, [terms that alias out], number of terms, [coefficient.hex(), ...]]
  ['edm_euler_step', sigma.hex(), sigma_next.hex(), cfg_scale.hex()]
  ['net', noise label float(t[0]), rows of t]                                   a generic-route network call
  ['net', label, rows, in_scale[0].hex(), the mod_cache step index or None]     a fused-route (stub) network call
  ['prepare_timesteps', the schedule's labels t_table[:, 0], [n, 2B]]
  ['step_noise', i]
Coefficients are logged as the host float64 handed to ctypes, which is stricter than the fp32 the kernel receives.

    python tests/sampler_launches.py --write --commit <id>     regenerates tests/golden/sampler_launches.json from the checked-out code

tests/test_sampler_launches_cpu.py compares the current code with that file entry by entry."""
import contextlib
import json
import os
import sys

import torch

import sampler_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sampler_launches.json')


def _same(a, b):
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape)


@contextlib.contextmanager
def recording_ops(log):
    from ln3diff_amd import ops

    def lincomb(y, ks, cs, out):
        log.append(['lincomb', y is None, y is not None and _same(y, out), [j for j, k in enumerate(ks) if _same(k, out)], len(ks),
                    [float(c).hex() for c in cs]])
        acc = torch.zeros_like(out) if y is None else y.clone()
        for k, c in zip(ks, cs):
            acc += k.reshape(out.shape) * torch.tensor(float(c), dtype=torch.float32)
        out.copy_(acc)

    def edm_euler_step(x, eps2, sigma, sigma_next, cfg_scale):
        log.append(['edm_euler_step', float(sigma).hex(), float(sigma_next).hex(), float(cfg_scale).hex()])
        s, sn, g = (torch.tensor(float(v), dtype=torch.float32) for v in (sigma, sigma_next, cfg_scale))
        e = eps2.reshape(2, *x.shape)
        den_u, den_c = e[0] * (-s) + x, e[1] * (-s) + x
        den = den_u + g * (den_c - den_u)
        x.copy_(x + (x - den) / s * (sn - s))

    saved = ops.lincomb, ops.edm_euler_step
    ops.lincomb, ops.edm_euler_step = lincomb, edm_euler_step
    try:
        yield
    finally:
        ops.lincomb, ops.edm_euler_step = saved


def _stub(with_timesteps, log):
    class Stub(R.StubNetworkWithTimesteps if with_timesteps else R.StubNetwork):
        def __call__(self, x, t, context_cache=None, in_scale=None, mod_cache=None, cfg_twins=False):
            log.append(['net', float(t[0]), int(t.shape[0]), float(in_scale[0]).hex(), None if mod_cache is None else int(mod_cache[1])])
            return super().__call__(x, t, context_cache=context_cache, in_scale=in_scale, mod_cache=mod_cache, cfg_twins=cfg_twins)

        if with_timesteps:
            def prepare_timesteps(self, t_table):
                log.append(['prepare_timesteps', t_table[:, 0].tolist(), list(t_table.shape)])
                return super().prepare_timesteps(t_table)
    return Stub()


def record(case, shape):
    """the launch log of one case of R.SGM_CASES on `shape`: the routes of tests/test_sampler_loops_gpu.py::_run_sgm, on the CPU"""
    from ln3diff_amd.sgm import sampling as S
    inp, log = R.inputs(shape), []
    cls = {'euler': S.EulerEDMSampler, 'heun': S.HeunEDMSampler, 'ancestral': S.EulerAncestralSampler, 'dpmpp2s': S.DPMPP2SAncestralSampler,
           'dpmpp2m': S.DPMPP2MSampler, 'lms': S.LinearMultistepSampler}[case['kind']]
    scale = case.get('scale', R.CFG)
    sampler = cls(num_steps=R.SGM_STEPS, guider=S.IdentityGuider() if scale is None else S.VanillaCFG(scale), use_graph=False,
                  **dict(case.get('kw', {})))
    dk = dict(case.get('den') or {})
    scaling = {'eps': S.EpsScaling, 'v': S.VScaling, 'v_edm': S.VScalingWithEDMcNoise, 'edm': S.EDMScaling}[dk.get('scaling', 'eps')]()
    index_labels = dk.get('discrete', True) and dk.get('quantize_c_noise', True)
    den = S.DiscreteDenoiser(scaling=scaling, quantize_c_noise=index_labels) if dk.get('discrete', True) else S.Denoiser(scaling)

    def net(x, t, c, **kw):
        log.append(['net', float(t[0]), int(t.shape[0])])
        return R.rational_net(x, t, c, index_labels)

    def step_noise(i):
        log.append(['step_noise', int(i)])
        return inp['noise'][i]
    route, kw = case['route'], {}
    if route == 'bind':
        arg = den.bind(net)
    elif route == 'closure':
        arg = lambda input, sigma, c: den(net, input, sigma, c)
    elif route == 'network_v':
        arg, kw = den, dict(network=net)
    else:
        stub = _stub(route == 'fused_timesteps', log)
        if route == 'fused_network':
            arg, kw = den, dict(network=stub)
        elif route == 'fused_lambda':
            self = type('Engine', (), {})()
            self.denoiser, self.model = den, stub
            additional_model_inputs = {}
            arg = lambda input, sigma, c: self.denoiser(self.model, input, sigma, c, **additional_model_inputs)
            assert S._find_pair(arg) == (den, stub)
        else:
            arg = den.bind(stub)
    cond, uc = {'crossattn': inp['c']}, {'crossattn': inp['uc']}
    tr = []
    with recording_ops(log):
        y = sampler(arg, inp['z'].clone(), cond, None if scale is None else uc, trace=tr, step_noise=step_noise, **kw)
    assert len(tr) == R.SGM_STEPS and torch.equal(y, tr[-1]) and bool(torch.isfinite(y).all())
    return json.loads(json.dumps(log))            # what a reader of the golden gets: lists, floats, strings


def record_all():
    return {str(shape): {name: record(case, shape) for name, case in R.SGM_CASES.items()} for shape in R.SHAPES}


def write(path, commit):
    logs = record_all()
    with open(path, 'w') as f:                    # one line per case: a change shows as that case's line
        f.write('{"generated_from": %s,\n "logs": {\n' % json.dumps(commit))
        for si, (shape, cases) in enumerate(logs.items()):
            f.write('  %s: {\n' % json.dumps(shape))
            f.write(',\n'.join('   %s: %s' % (json.dumps(n), json.dumps(log, separators=(',', ':'))) for n, log in cases.items()))
            f.write('\n  }%s\n' % (',' if si + 1 < len(logs) else ''))
        f.write(' }\n}\n')
    return logs


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--commit', default='unknown', help='the commit whose code is checked out (stored in the file)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    logs = write(GOLDEN, a.commit) if a.write else record_all()
    n = sum(len(log) for cases in logs.values() for log in cases.values())
    print('%d runs, %d entries, %d launches' % (sum(len(c) for c in logs.values()), n, sum(e[0] in ('lincomb', 'edm_euler_step')
                                                                                          for c in logs.values() for l in c.values() for e in l)))
