"""Every token of the DiT denoisers' forward(), in every dispatch form, against the float64 oracle (tests/dit_token_refs.py).

One forward of a depth-2 network with synthetic weights per case (head size 72: depth 1).  The whole-tensor gates of test_dit_gpu.py /
test_i23d_gpu.py (rel-L2 < 2e-2 against fp32, < 1e-3 between two forms) cannot see one token wrong by a few percent, one layer reading
its neighbour's slice or one sample reading another's modulation row; here every (sample, plane, patch) group of the output is held to

    rho_t = ||y_hip - y16||_t / max(||y16 - y64||_t, 0.1 median)  <=  CAP

where y64 is the float64 oracle and y16 the float64 oracle with the kernels' arithmetic (bf16 GEMM / attention operands and the
rounding points oracle.dit.operand_rounding names): the HIP forward may be no further from
the bf16-operand restatement than CAP times what operand rounding itself does to that token.  The oracle never folds, caches or
dedups, so fold / no fold, cfg_twins, mod_cache in both layouts, the appended-token K / V cache, fused and unfused cross-attention and
q-norm are all held to the same answer - and each case asserts which path it took, from what the code exposes (cc['fold'], 'const' in
cc, mc['rows'], cc['akv'], ops.heads_norm_fusable), so that no case silently tests another form.
"""
import pytest
import torch

import dit_token_refs as R
from conftest import load_synth

pytestmark = pytest.mark.gpu

# CAP.  The rule is twice the worst measured rho, rounded up to one digit, and never above 1.0: a forward further from the bf16-operand
# restatement than operand rounding itself moves the token means a rounding point the oracle lacks, or a wrong kernel.  Twice the worst
# value below is 1.8, so the ceiling decides: CAP = 1.0, one cap for all cases (the classes differ by less than 2x).
#
# What was missing, found with this test at rho up to 1.3 and now restated by oracle.dit.operand_rounding(kernel_arith=True,
# unfused_norms=...) (its docstring names each): the fp32 argument of the timestep embedding; q scaled by scale * log2(e) and rounded
# a second time in the streaming attention kernel; the probabilities rounded against the kernels' RUNNING reference instead of the row
# maximum; the second rounding in front of a qk-norm that runs unfused; the polynomial erf of the fc1 epilogue.  With those a single
# block agrees with the HIP block to rho ~ 0.001 at the median.  What is left is rounding-boundary flips: where an fp32 accumulator lands
# on the other side of a bf16 boundary than the float64 one, that element is off by a whole ulp, the self-attention of the next layer
# spreads it over the sample, and every rounding behind it flips with a probability ~ sqrt(perturbation / ulp).  The point-cloud variant's
# tokens have a third of the norm of the tri-plane ones under the same weights, so the same flip is three times the relative perturbation:
# its median rho is 0.24 where the others have 0.001 .. 0.09.
#
# measured: worst rho of every case on gfx950 (MI355X), tile choice left to the library
MEASURED = {
    't23d-small-plain': 0.370, 't23d-small-cfg_fold': 0.483, 't23d-small-cfg_nofold': 0.483, 't23d-small-oddfold': 0.189,
    't23d-small-modcache_shared': 0.339, 't23d-small-modcache_ragged': 0.334, 't23d-small-twins_fold': 0.409,
    't23d-small-twins_nofold': 0.409, 't23d-small-lc1': 0.020, 't23d-small-lc64': 0.355, 't23d-small-lc65': 0.468, 't23d-small-lc100': 0.284,
    't23d-fused-plain': 0.392, 't23d-fused-cfg_fold': 0.505, 't23d-fused-cfg_nofold': 0.505, 't23d-fused-oddfold': 0.256,
    't23d-fused-modcache_shared': 0.475, 't23d-fused-modcache_ragged': 0.415, 't23d-fused-twins_fold': 0.553,
    't23d-fused-twins_nofold': 0.553, 't23d-fused-lc1': 0.123, 't23d-fused-lc64': 0.489, 't23d-fused-lc65': 0.457, 't23d-fused-lc100': 0.344,
    'i23d-pixart-default': 0.499, 'i23d-pixart-cache_off': 0.523, 'i23d-pixart-fold_on': 0.420, 'i23d-pixart-fold_off': 0.361,
    'i23d-pixart-fold3': 0.373, 'i23d-h72-default': 0.268, 'i23d-plain-default': 0.309, 'i23d-mvcond-default': 0.183,
    'i23d-noclip-default': 0.530, 'i23d-t23d_pixart-default': 0.181, 'i23d-pcd-default': 0.872,
}
CAP = 1.0
assert set(MEASURED) == set(R.CASE_IDS) and CAP <= 1.0


def _check(cid, y_hip, ntok):
    c = R.case(cid)
    y64, y16 = R.oracle_pair(cid)
    rho, d = R.token_rho(y_hip, y16, y64, c['patch'])
    assert rho.numel() == ntok                                                                    # every token, none left out
    where, worst = R.worst_token(rho)
    print(f'{cid}: worst token (sample, plane, patch) = {where}, rho = {worst:.3f}; median rho {float(rho.median()):.3f}; '
          f'd median {float(d.median()):.3e} (measured: worst {MEASURED[cid]}); per sample (max, median): '
          + ', '.join(f'({float(r.max()):.2f}, {float(r.median()):.2f})' for r in rho))
    assert torch.isfinite(rho).all()
    assert worst <= CAP, (cid, where, worst)


@pytest.mark.parametrize("cid", [i for i in R.CASE_IDS if i.startswith('t23d-')])
def test_t23d_every_token(hip_lib, monkeypatch, cid):
    c = R.case(cid)
    for k in c['env']:
        monkeypatch.setenv(k, '1')
    m = R.build_t23d(c['net'])
    load_synth(m, 0)
    m = m.cuda()
    Bn, Bx = c['t'].shape[0], c['x'].shape[0]
    cc = m.prepare_context(c['ctx'].cuda())
    assert cc['fold'] == c['fold'] and ('const' in cc) == (c['fold'] > 0), (cc['fold'], c['fold'])
    N, H = 3 * (m.input_size // m.patch_size) ** 2, m.num_heads
    fused_cross = N % 192 == 0 and (H * 64) % 256 == 0 and cc['Lc'] <= 96 and 'kp' in cc          # forward()'s three conditions
    assert fused_cross == c['fused_cross'] == (c['net'] == 'fused' and c['ctx'].shape[1] <= 96)
    kw = {}
    ld = None
    if c['t_table'] is not None:
        mc = m.prepare_timesteps(c['t_table'])
        assert mc['rows'] == c['rows'] and mc['mod'].shape[0] == c['t_table'].shape[0] * c['rows']
        kw['mod_cache'] = (mc, c['step'])
        ld = 0 if mc['rows'] == 1 else 1
    if c['in_scale'] is not None:
        kw['in_scale'] = c['in_scale'].cuda()
    if c['cfg_twins']:
        kw['cfg_twins'] = True
    dedup0 = c['cfg_twins'] and 2 * Bx == Bn and ld == 0 and cc['fold'] in (0, Bn // 2)          # forward()'s condition
    assert dedup0 == c['dedup0']
    y = m(c['x'].cuda(), c['t'].cuda(), context_cache=cc, **kw).cpu()
    _check(cid, y, Bn * N)


@pytest.mark.parametrize("cid", [i for i in R.CASE_IDS if i.startswith('i23d-')])
def test_i23d_every_token(hip_lib, monkeypatch, cid):
    from ln3diff_amd import ops
    from ln3diff_amd.dit.dit_models_xformers import attn_head_pad
    c = R.case(cid)
    for k in c['env']:
        monkeypatch.setenv(k, '1')
    m = R.build_i23d(c['net'])
    load_synth(m, 0)
    m = m.cuda()
    cc = m.prepare_context({k: v.cuda() for k, v in c['ctx'].items()})
    assert cc['fold'] == c['fold'] and ('const' in cc) == (c['fold'] > 0), (cc['fold'], c['fold'])
    Bn, N, H = c['t'].shape[0], m._num_tokens(c['x']), m.num_heads
    # cross-attention q-norm inside the query projection's epilogue, or as a separate pass (forward()'s fuse_cq)
    assert ops.heads_norm_fusable((Bn - cc['fold']) * N, H * 64, N, 64) == c['fuse_cq']
    Dh = m.embed_dim // H
    if c['net'] == 'h72':
        assert Dh == 72 and attn_head_pad(72) != 72                                               # padded heads, dh_true / attn_out_dim
    # the qk-norms this form runs as a pass of their own (a second bf16 rounding the oracle restates, dit_token_refs._i23d_case)
    Ld = cc['dino'].shape[1]
    unfused = set()
    if Dh != 64:
        unfused.add('self_qk')
    elif c['akv'] and not ops.heads_norm_fusable(Bn * Ld, 3 * H * attn_head_pad(Dh), Ld, Dh, attn_head_pad(Dh)):
        unfused.add('appended_k')
    if not c['fuse_cq']:
        unfused.add('cross_q')
    assert unfused == set(c['unfused_norms']), (unfused, c['unfused_norms'])
    y = m(c['x'].cuda(), c['t'].cuda(), context_cache=cc).cpu()
    assert (cc.get('akv') is not None) == c['akv'], cc.get('akv') is None                                 # the appended-token K / V cache
    _check(cid, y, Bn * N)
