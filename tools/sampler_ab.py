#!/usr/bin/env python
"""Bitwise A/B listing for changes to the host side of the sgm samplers (ln3diff_amd/sgm/sampling.py): one sha256 line per trace entry
for every case of tests/sampler_refs.SGM_CASES on both of its shapes (the exact stub networks of the loop tests), and the final latent
of a tiny real DiT_TriLatent through EulerEDMSampler's routes (bind, the reference's lambda, network=, noise injection, graph replay).
Run it on two trees that load the same libln3d_hip.so and compare the listings:

    python tools/sampler_ab.py [--tree OTHER_CHECKOUT] > listing.txt

Only the samplers' public surface and the tests' own helpers are used, so the same file runs against an older checkout (--tree)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout to import ln3diff_amd and tests/ from')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
for p in (os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import ln3diff_amd  # noqa: E402
assert os.path.abspath(ln3diff_amd.__file__).startswith(ROOT + os.sep), (ln3diff_amd.__file__, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def loops():
    import sampler_refs as R
    from test_sampler_loops_gpu import _run_sgm
    for shape in R.SHAPES:
        for name, case in R.SGM_CASES.items():
            tr, _ = _run_sgm(case, shape)
            for i, x in enumerate(tr):
                print(f'loop/{name} {list(shape)} step{i} {sha(x)}')


def tiny_dit():
    from ln3diff_amd.sgm import sampling as S
    from ln3diff_amd.synth import synth_input
    from test_samplers_gpu import _tiny
    m = _tiny()
    z = synth_input('z', (2, 12, 32, 32), 41).cuda()
    cond = {'crossattn': synth_input('c', (2, 77, 768), 41).cuda()}
    uc = {'crossattn': torch.zeros_like(cond['crossattn'])}
    den = S.DiscreteDenoiser()
    g = torch.Generator().manual_seed(5)
    draws = [torch.randn(2, 12, 32, 32, generator=g) for _ in range(12)]
    self = type('Engine', (), {})()
    self.denoiser, self.model = den, m
    additional_model_inputs = {}
    ref = lambda input, sigma, c: self.denoiser(self.model, input, sigma, c, **additional_model_inputs)
    assert S._find_pair(ref) == (den, m)

    def run(name, arg, graph=False, kw=None, **call_kw):
        sampler = S.EulerEDMSampler(num_steps=12, guider=S.VanillaCFG(6.5), use_graph=graph, **(kw or {}))
        y = sampler(arg, z.clone(), cond, uc, step_noise=lambda i: draws[i], **call_kw)
        print(f'dit/{name} final {sha(y)}')
    run('bind', den.bind(m))
    run('reference_lambda', ref)
    run('network', den, network=m)
    run('churn', den.bind(m), kw=dict(s_churn=2.0, s_tmin=0.6, s_tmax=5.0, s_noise=1.1))
    run('graph_replay', den.bind(m), graph=True)


if __name__ == '__main__':
    loops()
    tiny_dit()
