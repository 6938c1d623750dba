"""Volume-composited normals on the GPU (mode 1 of ln3d_surface_normals, include/ln3d_normals.h): the kernel per ray and component against
the float64 reference of tests/normal_composite_refs.py on SYNTHETIC weights and coordinates (no render involved, no sample on a texel
centre, nothing left out), the skip rule, bit-reproducibility, the f16 entry point, spaces and thresholds, the agreement with mode 0, and
the module seams (Triplane.forward, ImportanceRenderer.forward, the launcher) behind a real render."""
import os

import numpy as np
import pytest
import torch

import normal_composite_refs as cr
import normal_refs as nr
import render_refs as rr
from test_normals_cpu import GRAD_BOUND_ULPS, MARGIN
from test_normals_gpu import _cams, _g, _same, _triplane

pytestmark = pytest.mark.gpu

H, W, BOX = 16, 16, 0.9
V = 4
PIDX = (1, 0, 1, 1)


def _scene(seed, gain=1.0):
    inp = rr.make_scene(seed, 1, M=1, H=H, W=W, NP=2, plane_scale=2.0, hidden_gain=gain)
    return inp['planes'], inp['dec']


def _launch(planes, dec, coords, w, wsum, M, T, floor=0.0, thr=0.5, space='world', cams=None, pidx=PIDX):
    """-> (accum [R, 3], normal [R, 3]) on the CPU; the NaN tail behind both outputs is checked"""
    from ln3diff_amd import ops
    nv = len(pidx)
    n = nv * 3 * M
    nrm, acc = torch.full((n + 8,), float('nan'), device='cuda'), torch.full((n + 8,), float('nan'), device='cuda')
    ops.surface_normals(_g(planes), H, W, torch.tensor(pidx, dtype=torch.int32, device='cuda'), tuple(_g(t) for t in dec), BOX, None, _g(wsum), nrm,
                        cams=_g(cams), n_views=nv, rays_per_view=M, mask_threshold=thr, space=space, mode='composited',
                        weights=_g(w.reshape(nv, M, T - 1)), coords=_g(coords.reshape(nv, M, T, 3)), weight_floor=floor, accum=acc)
    torch.cuda.synchronize()
    nrm, acc = nrm.cpu(), acc.cpu()
    assert torch.isnan(nrm[n:]).all() and torch.isnan(acc[n:]).all(), "the NaN tail behind an output was written"
    rows = lambda t: t[:n].reshape(nv, 3, M).permute(0, 2, 1).reshape(nv * M, 3)               # noqa: E731
    return rows(acc), rows(nrm)


def _inputs(T, M, seed, nv=V):
    R = nv * M
    coords = nr.sample_points(R * T, seed, H, W, BOX, MARGIN).reshape(R, T, 3)
    assert float(nr.texel_margin(coords.reshape(-1, 3), H, W, BOX).min()) >= MARGIN          # nothing is left out: the excluded share is 0
    w = cr.make_weights(R, T, seed)
    g = torch.Generator().manual_seed(seed + 1)
    wsum = torch.rand(R, generator=g)                                                         # the mask is an input of its own
    wsum[::11] = float('nan')
    return coords, w, wsum.float()


def _check_normal(acc, nrm, wsum, thr):
    """normal = unit(the kernel's own accum) in float64 to 4 fp32 ulps; exactly 0 under the mask, for N = 0 and for a non-finite N"""
    on = wsum >= thr
    ok = torch.isfinite(acc).all(-1) & (acc.abs().amax(-1) > 0)
    assert bool((nrm[~(on & ok)] == 0).all())
    want = cr.unit64(acc)
    assert bool(((nrm.double() - want).abs()[on & ok] <= 4 * nr.F32_EPS).all()), float((nrm.double() - want).abs()[on & ok].max())
    return on & ok


@pytest.mark.parametrize("M", [1, 5, 300])
@pytest.mark.parametrize("T", [2, 63, 64, 65, 128, 192, 256])
def test_kernel_against_float64_per_ray_and_component(hip_lib, T, M):
    planes, dec = _scene(500 + T, gain=12.0 if T % 2 else 1.0)
    coords, w, wsum = _inputs(T, M, 1000 * T + M)
    R = V * M
    ray_plane = torch.tensor(PIDX).repeat_interleave(M)
    ref = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS)
    acc, nrm = _launch(planes, dec, coords, w, wsum, M, T)
    assert acc.shape == (R, 3) and not torch.isnan(acc).any() and not torch.isnan(nrm).any()         # the NaN weight is skipped, not summed
    err = (acc.double() - ref['accum']).abs()
    frac = torch.where(err == 0, torch.zeros_like(err), err / ref['bound'].clamp(min=1e-300))
    print(f"[normals-composite] T={T} M={M}: accum worst {float(frac.max()):.3g} of the bound, {int(ref['active'].sum())} / {R * T} samples evaluated")
    assert bool((frac <= 1).all()), (int((frac > 1).sum()), float(frac.max()))
    assert bool((acc[0] == 0).all())                                                                  # the all-zero ray
    assert int(torch.isnan(w[1]).sum()) == 1 and int((w[2] != 0).sum()) == 1
    live = _check_normal(acc, nrm, wsum, 0.5)
    assert M == 1 or (0 < int(live.sum()) < R)


def test_weight_floor_applies_the_stated_rule(hip_lib):
    T, M = 128, 40
    planes, dec = _scene(61)
    coords, w, wsum = _inputs(T, M, 62)
    ray_plane = torch.tensor(PIDX).repeat_interleave(M)
    om = cr.omegas(w)
    floor = float(om[om > 0].median())                      # an fp32 value that occurs: `>` is decided on equal bits too
    ref = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS, floor=floor)
    full = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS)
    assert 0 < int(ref['active'].sum()) < int(full['active'].sum())
    acc, nrm = _launch(planes, dec, coords, w, wsum, M, T, floor=floor)
    err = (acc.double() - ref['accum']).abs()
    assert bool((err <= ref['bound']).all()), float((err / ref['bound'].clamp(min=1e-300)).max())
    assert not bool(((acc.double() - full['accum']).abs() <= full['bound']).all())         # and it is not the unfloored sum
    _check_normal(acc, nrm, wsum, 0.5)


def test_two_runs_and_the_f16_entry_give_the_same_bits(hip_lib):
    T, M = 192, 60
    planes, dec = _scene(71, gain=12.0)
    coords, w, wsum = _inputs(T, M, 72)
    a = _launch(planes, dec, coords, w, wsum, M, T)
    b = _launch(planes, dec, coords, w, wsum, M, T)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    h = _launch(planes.half(), dec, coords, w, wsum, M, T)
    f = _launch(planes.half().float(), dec, coords, w, wsum, M, T)
    for x, y in zip(h, f):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[0], f[0])                      # the rounded planes are other planes


def test_camera_space_and_threshold(hip_lib):
    T, M = 65, 64                                           # explicit M = res * res: the rays themselves are never read
    planes, dec = _scene(81)
    coords, w, wsum = _inputs(T, M, 82)
    cams = _cams(V)
    acc, n = _launch(planes, dec, coords, w, wsum, M, T, cams=cams)
    acc_c, nc = _launch(planes, dec, coords, w, wsum, M, T, cams=cams, space='camera')
    assert torch.equal(acc.view(torch.int32), acc_c.view(torch.int32))                     # accum stays in world space
    Rm = cams[:, :16].reshape(V, 4, 4)[:, :3, :3].double().repeat_interleave(M, 0)        # [R, 3 (world), 3 (camera)]
    want = torch.einsum('rkc,rk->rc', Rm, n.double())
    assert float((nc.double() - want).abs().max()) <= 4 * nr.F32_EPS
    on = wsum >= 0.5
    assert bool((nc[~on] == 0).all()) and int(on.sum()) > 0
    _, n9 = _launch(planes, dec, coords, w, wsum, M, T, thr=0.9)
    on9 = wsum >= 0.9
    assert 0 < int(on9.sum()) < int(on.sum())
    assert torch.equal(n9[on9].view(torch.int32), n[on9].view(torch.int32)) and bool((n9[~on9] == 0).all())


def test_grid_stride_more_rays_than_wavefronts(hip_lib):
    """the launch has at most 4096 blocks of four waves: 4 x 4200 rays at T = 2 make every wave take a second ray"""
    T, M = 2, 4200
    planes, dec = _scene(91)
    coords, w, wsum = _inputs(T, M, 92)
    assert V * M > 4096 * 4
    ray_plane = torch.tensor(PIDX).repeat_interleave(M)
    ref = cr.composite64(planes, ray_plane, coords, w, dec, BOX, GRAD_BOUND_ULPS)
    acc, nrm = _launch(planes, dec, coords, w, wsum, M, T)
    err = (acc.double() - ref['accum']).abs()
    assert bool((err <= ref['bound']).all()), float((err / ref['bound'].clamp(min=1e-300)).max())
    assert int((acc[4096 * 4:] != 0).any(-1).sum()) > 100
    _check_normal(acc, nrm, wsum, 0.5)


def test_agrees_with_the_surface_mode_at_one_point(hip_lib):
    """all T coordinates of a ray are one point p and sum omega = 1: the composited unit normal is the mode-0 normal at p, to 8 ulps
    (mode 0 reaches p as o + (depth / wsum) d with o = p, depth = 0)"""
    from ln3diff_amd import ops
    T, M = 65, 50
    planes, dec = _scene(95, gain=12.0)
    R = V * M
    p = nr.sample_points(R, 96, H, W, BOX, MARGIN, spread=0.45)
    coords = p[:, None, :].expand(R, T, 3).contiguous()
    w = torch.zeros(R, T - 1)
    w[:, 10], w[:, 11], w[:, 40] = 0.5, 0.25, 0.25
    assert bool((cr.omegas(w).double().sum(-1) == 1).all())
    ones = torch.ones(R)
    _, nc = _launch(planes, dec, coords, w, ones, M, T)
    n0 = torch.full((V, 3, M), float('nan'), device='cuda')
    ops.surface_normals(_g(planes), H, W, torch.tensor(PIDX, dtype=torch.int32, device='cuda'), tuple(_g(t) for t in dec), BOX,
                        torch.zeros(V, M, device='cuda'), _g(ones.reshape(V, M)), n0, ray_o=_g(p.reshape(V, M, 3)),
                        ray_d=_g(torch.ones(V, M, 3)), n_views=V, rays_per_view=M)
    n0 = n0.cpu().permute(0, 2, 1).reshape(R, 3)
    has = n0.abs().amax(-1) > 0
    assert int(has.sum()) > R // 2 and bool((nc[~has] == 0).all())
    assert float((nc.double() - n0.double()).abs().max()) <= 8 * nr.F32_EPS


# ---------------------------------------------------------------- module seams
def _end_to_end():
    inp = rr.make_scene(55, 3, H=H, W=24, NP=2, plane_scale=2.0, sigma_bias=6.0, res=8, cams=_cams(3), views_per_call=1)
    tp = _triplane(inp['dec'])
    kw = dict(c=_g(inp['cams']), planes_channel_last=_g(inp['planes']), plane_index=_g(inp['plane_index']), jitter=inp['jitter'],
              u_fine=inp['u_fine'], views_per_call=1)
    return inp, tp, kw


def test_triplane_forward_composited(hip_lib):
    from ln3diff_amd import ops, _lib
    from ln3diff_amd.nsr.triplane import render_call_kwargs
    inp, tp, kw = _end_to_end()
    a = tp(**kw)
    s = tp(return_normals=True, **kw)
    b = tp(return_normals=True, normal_mode='composited', **kw)
    assert set(b) == set(a) | {'image_normal', 'image_normal_raw'} and set(s) == set(a) | {'image_normal'}
    assert b['image_normal'].shape == b['image_normal_raw'].shape == (3, 3, 8, 8)
    _same(a, b)                                                         # image_raw / image_depth / weights_samples / ...: bit for bit
    assert not torch.equal(b['image_normal'], s['image_normal'])
    # the test's own composition: a generic render that returns weights / all_coords, then the composited launch
    Vn, M, T = 3, 64, 128
    dev = dict(planes=_g(inp['planes']), pidx=_g(inp['plane_index']), cams=_g(inp['cams']), dec=tuple(_g(t) for t in inp['dec']))
    d = {k: torch.empty(Vn * M * n, device='cuda') for k, n in (('rgb', 3), ('depth', 1), ('wsum', 1), ('lim', 2))}
    wts, crd = torch.empty(Vn, M, T - 1, device='cuda'), torch.empty(Vn, M, T, 3, device='cuda')
    ops.render_triplane(dev['planes'], H, 24, dev['pidx'], dev['cams'], 8, dev['dec'], _g(inp['jitter']), _g(inp['u_fine']), d['rgb'], d['depth'],
                        d['wsum'], d['lim'], torch.zeros(_lib.RENDER_SCRATCH_FLOATS, device='cuda'), views_per_call=1, weights=wts, all_coords=crd,
                        **render_call_kwargs(tp.rendering_kwargs))
    nrm, acc = torch.empty(Vn, 3, M, device='cuda'), torch.empty(Vn, 3, M, device='cuda')
    ops.surface_normals(dev['planes'], H, 24, dev['pidx'], dev['dec'], BOX, None, a['weights_samples'], nrm, cams=dev['cams'], res=8,
                        mode='composited', weights=wts, coords=crd, accum=acc)
    assert torch.equal(b['image_normal'].reshape(Vn, 3, M).view(torch.int32), nrm.view(torch.int32))
    assert torch.equal(b['image_normal_raw'].reshape(Vn, 3, M).view(torch.int32), acc.view(torch.int32))
    on = (a['weights_samples'] >= 0.5).expand(3, 3, 8, 8)
    assert int(on.sum()) > 0 and bool((b['image_normal'][~on] == 0).all())
    ln = b['image_normal'].norm(dim=1)[on[:, 0]]
    assert bool((((ln - 1).abs() <= 1e-6) | (ln == 0)).all())
    assert bool((b['image_normal_raw'].norm(dim=1) <= a['weights_samples'][:, 0] * (1 + 1e-5) + 1e-6).all())        # |N| <= sum omega <= wsum
    # a scratch budget that forces one call per chunk gives the bits of one chunk
    c = tp(return_normals=True, normal_mode='composited', normal_scratch_bytes=1, **kw)
    _same(b, c)
    with pytest.raises(ValueError, match="normal_mode 'volume'"):
        tp(return_normals=True, normal_mode='volume', **kw)


def test_importance_renderer_reuses_return_meta(hip_lib):
    inp, tp, _ = _end_to_end()
    o, d = rr.orbit_rays(3, 65, 5, spread=0.5)
    j, u = torch.rand(3, 65, 64, generator=torch.Generator().manual_seed(2)), torch.rand(3 * 65, 64, generator=torch.Generator().manual_seed(3))
    call = lambda **kw: tp.renderer(None, None, _g(o), _g(d), tp.rendering_kwargs, planes_channel_last=_g(inp['planes']), jitter=j, u_fine=u,     # noqa: E731
                                    plane_index=_g(inp['plane_index']), decoder_weights_dev=tp._decoder_dev(torch.device('cuda', 0)), **kw)
    plain = call(return_normals=True, normal_mode='composited')
    meta = call(return_normals=True, normal_mode='composited', return_meta=True)
    surf = call(return_normals=True)
    assert plain['normal_samples'].shape == plain['normal_samples_raw'].shape == (3, 65, 3) and 'normal_samples_raw' not in surf
    for k in ('normal_samples', 'normal_samples_raw'):
        assert torch.equal(plain[k].contiguous().view(torch.int32), meta[k].contiguous().view(torch.int32)), k
    assert not torch.equal(plain['normal_samples'], surf['normal_samples'])
    for k in ('feature_samples', 'depth_samples', 'weights_samples'):                      # the fast-path render of the plain call keeps its bits
        assert torch.equal(plain[k].contiguous().view(torch.int32), surf[k].contiguous().view(torch.int32)), k


def test_render_video_given_triplane_composited(hip_lib):
    """the pipeline seam: [B, V, ...] views of both normal keys, every other key bit-equal, image_normal = unit(image_normal_raw); a
    normal_mode without return_normals is refused at every level alike"""
    from test_normals_gpu import _small_ae
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    ae, _ = _small_ae()
    cams = orbit_cameras(3).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(6, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16, **kw)     # noqa: E731
    a, s, b = run(), run(return_normals=True), run(return_normals=True, normal_mode='composited')
    assert 'image_normal_raw' not in s and b['image_normal'].shape == b['image_normal_raw'].shape == (2, 3, 3, 16, 16)
    for k in ('image_raw', 'image_depth', 'weights_samples', 'image_mask'):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(b['image_normal'], s['image_normal'])
    raw, nrm = b['image_normal_raw'].cpu().permute(0, 1, 3, 4, 2).reshape(-1, 3), b['image_normal'].cpu().permute(0, 1, 3, 4, 2).reshape(-1, 3)
    on = (b['weights_samples'].cpu().reshape(-1) >= 0.5) & (raw.abs().amax(-1) > 0)
    assert int(on.sum()) > 0 and bool((nrm[~on] == 0).all())
    assert float((nrm.double() - cr.unit64(raw))[on].abs().max()) <= 4 * nr.F32_EPS
    with pytest.raises(ValueError, match="needs return_normals=True"):
        run(normal_mode='composited')
    tp = ae.decoder.triplane_decoder
    with pytest.raises(ValueError, match="needs return_normals=True"):
        tp(c=cams, planes_channel_last=torch.zeros(1, 3, 8, 8, 32, device='cuda'), plane_index=torch.zeros(3, dtype=torch.int32, device='cuda'),
           normal_mode='composited')


def test_entry_point_normal_map_mode(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    import json
    flags = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 4 --image_size 32 --num_views 2 --mesh_grid 24 --dit_model_arch DiT-B/2 "
             "--trainer_name sgm_legacy --save_normal_maps true")
    run(create_argparser(True).parse_args((flags + f" --logdir {tmp_path}/s").split()))
    run(create_argparser(True).parse_args((flags + f" --normal_map_mode composited --logdir {tmp_path}/c").split()))
    files = sorted(os.listdir(tmp_path / 's'))
    assert files == sorted(os.listdir(tmp_path / 'c')) and 'normal_sample0.npy' in files
    for f in files:
        a, b = open(tmp_path / 's' / f, 'rb').read(), open(tmp_path / 'c' / f, 'rb').read()
        if f.startswith('normal_sample'):
            na, nb = np.load(tmp_path / 's' / f), np.load(tmp_path / 'c' / f)
            assert na.shape == nb.shape == (2, 3, 32, 32) and nb.dtype == np.float32 and np.isfinite(nb).all() and not np.array_equal(na, nb)
            ln = np.linalg.norm(nb, axis=1)
            assert bool(((np.abs(ln - 1) <= 1e-5) | (ln == 0)).all())
        elif f == 'args.json':
            ja, jb = json.loads(a), json.loads(b)
            assert 'normal_map_mode' not in ja and jb.pop('normal_map_mode') == 'composited'
            ja.pop('logdir'), jb.pop('logdir')
            assert ja == jb
        else:
            assert a == b, f
