#!/usr/bin/env python
"""Bitwise A/B listing for changes to the host side of the DiT denoiser family (ln3diff_amd/dit/): runs every dispatch form of the
T23D and I23D denoisers at the test suite's smallest shapes and prints, per case,

  trace   one line per call of a public callable of ln3diff_amd.ops, in call order: the op, every scalar argument with the defaults
          spelled out (also the ones the wrapper computes: a GEMM's M and ldo, the attention's scale), and for every tensor its
          dtype, element count, storage offset and a label (s0, s1, ...) given to its storage at its first use in the case
  sha     the sha256 of every output and of every tensor of the prepared context / timestep caches
  packed  the packed operands by content (one line per distinct dtype, shape, sha256)

Run it on two trees that load the same libln3d_hip.so and diff the listings:

    python tools/dit_family_ab.py [--tree OTHER_CHECKOUT] > listing.txt

Only the public surface is used (the registries' classes, prepare_context / prepare_timesteps / forward / forward_with_cfg /
set_matmul_precision, `_packed`, tests/dit_token_refs.py), so the same file runs against an older checkout (--tree)."""
import argparse
import hashlib
import inspect
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout to import ln3diff_amd and tests/ from')
ap.add_argument('--only', default='', help='run the cases whose name starts with this')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
for p in (os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import ln3diff_amd  # noqa: E402
from ln3diff_amd import ops  # noqa: E402
assert os.path.abspath(ln3diff_amd.__file__).startswith(ROOT + os.sep), (ln3diff_amd.__file__, ROOT)
import dit_token_refs as R  # noqa: E402
from conftest import load_synth  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def tensors(node, path=''):
    if isinstance(node, torch.Tensor):
        yield path, node
    elif isinstance(node, ops.MX):
        yield path + '.q', node.q
        yield path + '.s', node.s
    elif isinstance(node, (dict, list, tuple)):
        for k, v in (node.items() if isinstance(node, dict) else enumerate(node)):
            yield from tensors(v, f'{path}.{k}' if path else str(k))


def out(case, name, node):
    for path, t in tensors(node, name):
        print(f'{case} sha {path} {str(t.dtype)[6:]}{list(t.shape)} {sha(t)}')


def packed(case, P):
    """The packed operands by content: one line per distinct (dtype, shape, sha256) in the dict, sorted.  Key names are left out and
    equal tensors count once, so a renamed key or one copy serving two keys does not show; a changed, missing or new value does."""
    for line in sorted({f'{str(t.dtype)[6:]}{list(t.shape)} {sha(t)}' for _, t in tensors(P)}):
        print(f'{case} packed {line}')


# ------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """Wraps every public callable of ln3diff_amd.ops; each call is printed (under the current case) and passed through."""

    def __init__(self):
        self.case, self.labels = '-', {}
        for name, fn in list(vars(ops).items()):
            if not name.startswith('_') and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
                setattr(ops, name, self.wrap(name, fn))

    def begin(self, case):
        self.case, self.labels = case, {}          # {storage address: (label, the storage: kept alive so the address is not reused)}

    def tensor(self, t):
        st = t.untyped_storage()
        label = self.labels.setdefault(st.data_ptr(), (f's{len(self.labels)}', st))[0]
        return f'{str(t.dtype)[6:]}:{t.numel()}@{t.storage_offset()}:{label}'

    def value(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, ops.MX):
            return f'MX({self.tensor(v.q)},{self.tensor(v.s)})'
        if isinstance(v, torch.device):
            return 'device'
        if isinstance(v, (list, tuple)):
            return '[' + ','.join(self.value(w) for w in v) + ']'
        return repr(v)

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def call(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            v = dict(b.arguments)
            if name in ('gemm', 'gemm_mx'):        # the defaults the wrapper computes
                w = v['w'].q if name == 'gemm_mx' else v['w']
                rows = v['x'].q.shape[0] if name == 'gemm_mx' else v['x'].numel() // w.shape[1]
                v['M'] = int(v['M'] if v['M'] is not None else rows)
                v['ldo'] = int(v['ldo'] if v['ldo'] is not None else w.shape[0])
            if name == 'attention' and v['scale'] is None:
                v['scale'] = v['Dh'] ** -0.5
            print(f'{self.case} trace {name} ' + ' '.join(f'{key}={self.value(val)}' for key, val in v.items()))
            return fn(*a, **k)
        call.__name__ = name
        return call


REC = Recorder()


# ------------------------------------------------------------------------------------------------ cases
def _env(names, on):
    for k in names:
        if on:
            os.environ[k] = '1'
        else:
            os.environ.pop(k, None)


def _build(c, precision=None):
    m = R.build_t23d(c['net']) if c['kind'] == 't23d' else R.build_i23d(c['net'])
    load_synth(m, 0)
    if precision is not None:
        m.set_matmul_precision(precision)
    return m.cuda()


def _cuda(v):
    return {k: w.cuda() for k, w in v.items()} if isinstance(v, dict) else v.cuda()


def token_case(cid, name=None, precision=None):
    """one case of dit_token_refs, as tests/test_dit_tokens_gpu.py runs it, twice: on a cold and on the warm workspace"""
    c = R.case(cid)
    name = name or cid
    REC.begin(name)
    _env(c['env'], True)
    try:
        m = _build(c, precision)
        cc = m.prepare_context(_cuda(c['ctx']))
        kw = {}
        if c['kind'] == 't23d':
            if c['t_table'] is not None:
                mc = m.prepare_timesteps(c['t_table'])
                out(name, 'mod_cache', mc)
                kw['mod_cache'] = (mc, c['step'])
            if c['in_scale'] is not None:
                kw['in_scale'] = c['in_scale'].cuda()
            if c['cfg_twins']:
                kw['cfg_twins'] = True
        for ws in ('cold', 'warm'):
            out(name, f'forward/{ws}', m(c['x'].cuda(), c['t'].cuda(), context_cache=cc, **kw))
        out(name, 'context', cc)
        packed(name, m._packed)
    finally:
        _env(c['env'], False)


def with_cfg():
    c = R.case('i23d-pixart-default')
    REC.begin('with_cfg')
    m = _build(c)
    out('with_cfg', 'forward_with_cfg', m.forward_with_cfg(c['x'].cuda(), c['t'].cuda(), context=_cuda(c['ctx']), cfg_scale=4.0))


def pcd_shrink():
    """768 points and then 512 on one instance and one prepared context: the appended-token cache is re-keyed (akv_N) and the
    zero-padded scratch shrinks its written extent"""
    c = R.case('i23d-pcd-default')
    REC.begin('pcd_shrink')
    m = _build(c)
    cc = m.prepare_context(_cuda(c['ctx']))
    for n in (768, 512):
        out('pcd_shrink', f'forward/{n}', m(c['x'][:, :n].contiguous().cuda(), c['t'].cuda(), context_cache=cc))
        out('pcd_shrink', f'context/{n}', cc)


def sampler():
    """a 4-step EulerEDMSampler CFG run through the bound denoiser (the fused loop), as tests/test_samplers_gpu.py builds it"""
    from ln3diff_amd.sgm.sampling import EulerEDMSampler, DiscreteDenoiser, VanillaCFG
    from ln3diff_amd.synth import synth_input
    REC.begin('sampler')
    m = _build(R.case('t23d-small-plain'))
    S = R.T23D_SIZES['small']['input_size']
    z = synth_input('z', (2, 12, S, S), 41).cuda()
    cond = {'crossattn': synth_input('c', (2, 77, 768), 41).cuda()}
    uc = {'crossattn': torch.zeros_like(cond['crossattn'])}
    y = EulerEDMSampler(num_steps=4, guider=VanillaCFG(6.5))(DiscreteDenoiser().bind(m), z, cond, uc)
    out('sampler', 'final_latent', y)
    print('sampler latent ' + ' '.join(f'{v:.9g}' for v in y.flatten()[:8].tolist()))


CASES = [(cid, lambda cid=cid: token_case(cid)) for cid in R.CASE_IDS]
CASES += [('with_cfg', with_cfg), ('pcd_shrink', pcd_shrink)]
CASES += [(f'mxfp8-{size}-{form}', lambda size=size, form=form: token_case(f't23d-{size}-{form}', f'mxfp8-{size}-{form}', 'mxfp8'))
          for size in ('small', 'fused') for form in ('plain', 'cfg_fold', 'twins_fold')]
CASES += [('sampler', sampler)]

if __name__ == '__main__':
    with torch.no_grad():
        for name, run in CASES:
            if name.startswith(args.only):
                run()
                sys.stdout.flush()
