"""Calibration of the ray-marcher's stage bounds (tests/render_refs.py) WITHOUT a GPU: no constant there is fitted to a kernel.

* the project's fp32 oracle (oracle/render.py: fp32 torch, serial cumsum / cumprod, no fma - other summation orders than the kernels')
  fed the same inputs must sit inside every stage bound and use at most half of it.  Worst fraction over the scenes below:
      limits 0.36  coarse_coords 0.42  coarse_sigma 0.003  fine_depths 0.35  fine_coords 0.50  fine_sigma 0.003  feature_volume 0.37
      weights 0.32  rgb 0.05  wsum 0.07  visibility 0.04  depth 0.002
  (coords: o + z d is two roundings in the oracle - exactly the two the scale counts - so 0.5 is its ceiling by construction;
  feature_volume reaches 0.37 only in the 'hidden' scene, where sigmoid saturates and the absolute 3-ulp term of the colour is all
  that is left of the bound; the kernels' measured fractions stand beside these in tests/test_render_stages_gpu.py);
* a torch emulation of the decoder's split-bf16 products (hi / lo exactly as split_bf16 of csrc/render.hip) must sit inside the
  decoder bound; the same emulation with the hi*lo and lo*hi terms dropped (plain truncated-bf16 products) must fail it;
* five seeded faults must fail the stage they belong to - among them one ray of 4 096 composited from two swapped samples, which the
  image-level rel-L2 < 2e-3 of the existing render tests does not see;
* no ray is excluded from a comparison except from `limits`, where the float64 slab test must have a margin (render_refs.slab_limits):
  the share without one is asserted <= 1e-3 per scene."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_refs as rr
from conftest import rel_l2
from oracle import render as orender


def _orbit_cams(V):
    from ln3diff_amd.synth import orbit_cameras
    return orbit_cameras(V)


SCENES = {
    'explicit_vpc2': dict(V=3, M=65, views_per_call=2),
    'cams': dict(V=2, res=8, cams='orbit'),
    'numeric_shapenet': dict(V=2, M=33, S=48, NI=48, numeric=(0.6, 1.8), box_warp=1.2, bbox=None, white_back=False),
    'opaque_80': dict(V=2, M=40, sigma_bias=12.0, S=80, NI=80),
    'empty_vpc2': dict(V=5, M=13, sigma_bias=-10.0, views_per_call=2),
    'hidden': dict(V=1, M=40, plane_scale=8.0, hidden_gain=4.0, H=8, W=8),
    'edges_128': dict(V=1, M=31, S=128, NI=128, H=8, W=8, jitter_edge=True),
}


def _scene(name):
    kw = dict(SCENES[name])
    if kw.get('cams') == 'orbit':
        kw['cams'] = _orbit_cams(kw['V'])
    return rr.make_scene(7, **kw)


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("merged", [True, False])
def test_fp32_oracle_is_inside_every_stage_bound(name, merged):
    inp = _scene(name)
    out = rr.oracle_outputs(inp)
    if not merged:
        out.update(weights=None, all_coords=None, feature_volume=None)       # the lane = sample kernel's output set: the reference sorts itself
    rep = rr.check_render(inp, out, 'fp32 oracle')
    rep.raise_if_failed()
    assert rep.notes.get('limits_without_margin', 0.0) <= 1e-3
    for stage, frac in rep.worst.items():
        assert frac <= 0.5, (stage, frac)


# ---------------------------------------------------------------- the decoder's arithmetic
def _split(x):
    hi = (x.contiguous().view(torch.int32) & -65536).view(torch.float32)           # truncated to bf16
    return hi, (x - hi).bfloat16().float()                                         # RNE bf16 of the remainder


def _mm_split(x, w, cross):
    xh, xl = _split(x)
    wh, wl = _split(w)
    r = xh @ wh.t()
    return r + xl @ wh.t() + xh @ wl.t() if cross else r


def _emulated_sigma(inp, pts, cross):
    LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
    planes = inp['planes'][:1].permute(0, 1, 4, 2, 3).contiguous()
    feat = orender.sample_planes(planes, pts[None], inp['box_warp']).mean(1)[0]
    w0, b0, w1, b1 = inp['dec']
    h = _mm_split(feat, w0 * np.float32(1 / np.sqrt(np.float32(32)) * LOG2E), cross) + b0 * np.float32(LOG2E)
    sp = torch.where(h > 128, h, torch.log2(1 + torch.exp2(h)))
    return (_mm_split(sp, w1 * np.float32(1 / 8 * LN2), cross) + b1)[:, 0]


@pytest.mark.parametrize("plane_scale,hidden_gain", [(2.0, 1.0), (8.0, 4.0)])
def test_split_bf16_products_meet_the_decoder_bound_and_plain_bf16_does_not(plane_scale, hidden_gain):
    inp = rr.make_scene(3, V=1, M=1, H=16, W=24, plane_scale=plane_scale, hidden_gain=hidden_gain)
    pts = (torch.rand(4099, 3, generator=torch.Generator().manual_seed(5)) - 0.5) * 0.9
    ref = rr.decoder(inp['planes'][0], pts, inp['dec'], inp['box_warp'])
    rep = rr.Report('split-bf16 emulation')
    rep.cmp('sigma', _emulated_sigma(inp, pts, True), ref['sigma'], ref['sigma_scale'], rr.DEC_ULPS, 1, 4099)
    rep.raise_if_failed()
    assert rep.worst['sigma'] <= 0.5
    bad = rr.Report('plain bf16 products')
    bad.cmp('sigma', _emulated_sigma(inp, pts, False), ref['sigma'], ref['sigma_scale'], rr.DEC_ULPS, 1, 4099)
    assert 'sigma' in bad.failed and bad.worst['sigma'] > 10


# ---------------------------------------------------------------- seeded faults
def _sample_pdf_shifted(bins, weights, u, shift, eps=1e-5):
    """oracle.render.sample_pdf with the bin index off by `shift`"""
    n_s = weights.shape[1]
    weights = weights + eps
    pdf = weights / weights.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    inds = torch.searchsorted(cdf, u.contiguous(), right=True) + shift
    below, above = (inds - 1).clamp(0, n_s), inds.clamp(0, n_s)
    cb, ca, bb, ba = cdf.gather(1, below), cdf.gather(1, above), bins.gather(1, below), bins.gather(1, above)
    den = ca - cb
    den = torch.where(den < eps, torch.ones_like(den), den)
    return bb + (u - cb) / den * (ba - bb)


def _coarse_pdf_inputs(inp, out):
    V, M, S = inp['V'], inp['M'], inp['S']
    z = out['coarse_depths'].reshape(V, M, S, 1)
    _, _, _, w = orender.ray_march(torch.zeros(V, M, S, 3), out['coarse_sigma'].reshape(V, M, S, 1), z, inp['white_back'])
    w = F.max_pool1d(w.reshape(V * M, 1, S - 1), 2, 1, padding=1)
    w = F.avg_pool1d(w, 2, 1).squeeze(1) + 0.01
    z = z.reshape(V * M, S)
    return 0.5 * (z[:, :-1] + z[:, 1:]), w[:, 1:-1]


def test_fault_inverse_cdf_bin_off_by_one():
    inp = _scene('explicit_vpc2')
    out = rr.oracle_outputs(inp)
    bins, w = _coarse_pdf_inputs(inp, out)
    same = _sample_pdf_shifted(bins, w, inp['u_fine'], 0)
    assert torch.equal(same.reshape(-1), out['fine_depths'].reshape(-1))                 # the copy IS the oracle's
    out['fine_depths'] = _sample_pdf_shifted(bins, w, inp['u_fine'], 1).reshape(out['fine_depths'].shape)
    rep = rr.check_render(inp, out, 'bin + 1')
    assert 'fine_depths' in rep.failed, rep.worst


def test_fault_last_interval_repeated_with_nonzero_alpha():
    """the lane that owns no further interval (lane 63 / element 127) marches its own last element again with the alpha of the interval
    before: w' = a T_last, with a = w_last / (w_last + T_last).  Without the bbox filter: with it the last samples of a ray lie outside the
    box, carry the fill density and alpha is 0 whatever is marched."""
    inp = _scene('numeric_shapenet')
    assert not inp['white_back']
    out = rr.oracle_outputs(inp)
    R = inp['V'] * inp['M']
    w_last, vis = out['weights'].reshape(R, -1)[:, -1], out['visibility'].reshape(R)
    a = w_last / (w_last + vis)
    extra = a * vis
    c_last = out['feature_volume'].reshape(R, -1, 3)[:, -1]
    out['wsum'] = (out['wsum'].reshape(R) + extra).reshape(out['wsum'].shape)
    out['visibility'] = (vis * (1 - a)).reshape(out['visibility'].shape)
    rgb = out['rgb'].permute(0, 2, 1).reshape(R, 3) + 2 * extra[:, None] * c_last
    out['rgb'] = rgb.reshape(inp['V'], inp['M'], 3).permute(0, 2, 1).contiguous()
    rep = rr.check_render(inp, out, 'repeated last interval')
    assert {'wsum', 'visibility', 'rgb'} <= set(rep.failed), rep.worst


def test_fault_border_taps_clamped_instead_of_zero_padded():
    inp = rr.make_scene(7, V=1, M=40, H=8, W=8)
    out = rr.oracle_outputs(inp)
    pts = out['coarse_coords'].reshape(1, -1, 3)
    cs = (2 / inp['box_warp']) * pts
    planes = inp['planes'][0].permute(0, 3, 1, 2).contiguous()                           # [3, C, H, W]
    grid = torch.stack([cs[0][:, [0, 1]], cs[0][:, [1, 2]], cs[0][:, [2, 0]]])[:, None]  # [3, 1, P, 2]
    feats = F.grid_sample(planes, grid, mode='bilinear', padding_mode='border', align_corners=False)[:, :, 0].permute(0, 2, 1)[None]
    sd = {'net.0.weight': inp['dec'][0], 'net.0.bias': inp['dec'][1], 'net.2.weight': inp['dec'][2], 'net.2.bias': inp['dec'][3]}
    _, sigma = orender.osg_decoder(sd, feats)
    inb = ((pts >= inp['bbox'][0]) & (pts <= inp['bbox'][1])).all(-1)
    sigma = torch.where(inb[..., None], sigma, torch.full_like(sigma, rr.FILL_SIGMA))
    out['coarse_sigma'] = sigma.reshape(out['coarse_sigma'].shape)
    rep = rr.check_render(inp, out, 'border padding')
    assert 'coarse_sigma' in rep.failed, rep.worst


def test_fault_depth_clamp_over_the_launch_instead_of_the_call_group():
    inp = _scene('empty_vpc2')
    out = rr.oracle_outputs(inp)
    V, M = inp['V'], inp['M']
    depth = out['depth'].reshape(V, M).clone()
    lo_launch = min(float(out['coarse_depths'].min()), float(out['fine_depths'].min()))
    changed = 0
    for g0 in range(0, V, 2):
        d = depth[g0:g0 + 2]
        lo = float(min(out['coarse_depths'].reshape(V, -1)[g0:g0 + 2].min(), out['fine_depths'].reshape(V, -1)[g0:g0 + 2].min()))
        at_lo = d == lo                                   # empty rays: sum w z ~ 0, clamped to the group's nearest sample
        changed += int(at_lo.sum()) if lo != lo_launch else 0
        d[at_lo] = lo_launch
    assert changed > 0
    out['depth'] = depth
    rep = rr.check_render(inp, out, 'launch-wide clamp')
    assert 'depth' in rep.failed, rep.worst


def test_fault_one_ray_of_4096_with_two_swapped_samples_passes_rel_l2_but_not_the_bound():
    inp = rr.make_scene(11, V=1, M=4096, S=16, NI=16, H=16, W=24, sigma_bias=2.0)
    out = rr.oracle_outputs(inp)
    rr.check_render(inp, out, 'fp32 oracle, 4 096 rays').raise_if_failed()
    R, NT = 4096, 32
    ws = out['wsum'].reshape(R)
    ray = int((ws - ws[ws > 0.5].median()).abs().argmin())
    z = torch.cat([out['coarse_depths'].reshape(R, 16), out['fine_depths'].reshape(R, 16)], 1)[ray]
    sig = torch.cat([out['coarse_sigma'].reshape(R, 16), out['fine_sigma'].reshape(R, 16)], 1)[ray]
    zs, idx = torch.sort(z)
    sigs, cols = sig[idx], out['feature_volume'].reshape(R, NT, 3)[ray]
    i = int(out['weights'].reshape(R, NT - 1)[ray].argmax())
    sw = list(range(NT))
    sw[i], sw[i + 1] = sw[i + 1], sw[i]
    rgb, depth, vis, w = orender.ray_march(cols[sw].reshape(1, 1, NT, 3), sigs[sw].reshape(1, 1, NT, 1), zs[sw].reshape(1, 1, NT, 1), True)
    ref_img = out['rgb'].clone()
    out['rgb'] = out['rgb'].clone()
    out['rgb'][0, :, ray] = rgb.reshape(3)
    out['wsum'] = out['wsum'].clone()
    out['wsum'].reshape(R)[ray] = w.sum()
    e = rel_l2(out['rgb'], ref_img)
    print(f"swapped samples {i}, {i + 1} of ray {ray}: image rel-L2 {e:.3g}, pixel moved by {float((out['rgb'] - ref_img).abs().max()):.3g}")
    assert 0 < e < 2e-3                                   # the existing image-level tests pass this image
    rep = rr.check_render(inp, out, 'two swapped samples')
    assert 'rgb' in rep.failed and 'wsum' in rep.failed and f"rays affected [{ray}]" in rep.failed['rgb'], rep.failed


def test_pair_bound_passes_two_sound_implementations_and_fails_the_swapped_ray():
    """render_refs.check_pair, the direct comparison the GPU file makes between the two kernels: the fp32 oracle's merged and
    un-merged output sets (the same numbers, two references: given colours / decoded colours, given order / own sort) agree inside
    it; with one ray's rgb and wsum moved as two swapped samples move them, they do not."""
    inp = rr.make_scene(11, V=1, M=256, S=16, NI=16, H=16, W=24, sigma_bias=2.0)
    out = rr.oracle_outputs(inp)
    plain = dict(out, weights=None, all_coords=None, feature_volume=None)
    ra, rb = rr.check_render(inp, plain, 'un-merged'), rr.check_render(inp, out, 'merged')
    rep = rr.check_pair(ra, rb)
    rep.raise_if_failed()
    assert {'limits', 'coarse_sigma', 'fine_depths', 'rgb', 'wsum', 'visibility', 'depth'} <= set(rep.worst)
    bad = dict(plain, rgb=plain['rgb'].clone(), wsum=plain['wsum'].clone())
    ray = int(out['wsum'].reshape(-1).argmax())
    bad['rgb'][0, :, ray] += 0.02                         # the size of the swapped-sample fault above (pixel moved by 0.0198)
    bad['wsum'].reshape(-1)[ray] -= 0.01
    rep = rr.check_pair(rr.check_render(inp, bad, 'un-merged, one ray moved'), rb)
    assert {'rgb', 'wsum'} <= set(rep.failed) and f"rays affected [{ray}]" in rep.failed['rgb'], rep.failed
