"""Surface normals on the GPU (include/ln3d_normals.h): the density gradient per component against the float64 reference inside the bound
calibrated in tests/test_normals_cpu.py, the per-ray surface points and normals behind a real ln3d_render_triplane call, the module
seams (Triplane.forward, render_video_given_triplane), vertex normals of the exported mesh and the launcher's two flags.

The gradient jumps where a projected coordinate crosses a texel centre, so points are compared where the reference ALONE says the
bilinear piece is not in doubt (normal_refs.texel_margin); the left-out share is asserted."""
import numpy as np
import pytest
import torch

import normal_refs as nr
import render_refs as rr
from test_normals_cpu import GRAD_BOUND_ULPS, MARGIN, parse_obj

pytestmark = pytest.mark.gpu

H, W, BOX = 16, 24, 0.9
RAY_MARGIN = 1e-3                # rays: about 12 * 1e-3 = 1.2 % of the surface points lie this close to a texel centre
MAX_EXCLUDED = 0.05


def _g(t):
    return None if t is None else t.cuda().contiguous()


def _scene(seed, V=3, **kw):
    kw.setdefault('sigma_bias', 6.0)
    if kw.get('cams') is None:
        kw.setdefault('M', 1)
    return rr.make_scene(seed, V, H=H, W=W, NP=2, plane_scale=2.0, **kw)


def _grad(plane, pts, dec, f16=False):
    from ln3diff_amd import ops
    P = pts.shape[0]
    sigma, grad = torch.full((P + 8,), float('nan'), device='cuda'), torch.full((3 * P + 8,), float('nan'), device='cuda')
    ops.query_points_grad(_g(plane.half() if f16 else plane), H, W, _g(pts), tuple(_g(t) for t in dec), BOX, sigma, grad)
    torch.cuda.synchronize()
    sigma, grad = sigma.cpu(), grad.cpu()
    assert torch.isnan(sigma[P:]).all() and torch.isnan(grad[3 * P:]).all(), "the NaN tail behind an output was written"
    return sigma[:P], grad[:3 * P].reshape(P, 3)


@pytest.mark.parametrize("P,gain", [(1, 1.0), (63, 1.0), (64, 12.0), (65, 1.0), (257, 12.0), (4096 + 3, 1.0), (4096 + 3, 12.0)])
def test_query_points_grad_per_component(hip_lib, P, gain):
    """hidden_gain 12 puts a few percent of the hidden units on softplus' linear branch (h > 20)"""
    inp = _scene(100 + P, hidden_gain=gain)
    plane, dec = inp['planes'][1], inp['dec']
    pts = nr.sample_points(P, 7 * P + int(gain), H, W, BOX, MARGIN)
    if gain > 1:          # the reference alone says that this scene has hidden units on the linear branch
        assert bool((nr.grad_f32(plane, pts, dec, BOX, 'no_linear_branch') != nr.grad_f32(plane, pts, dec, BOX)).any())
    assert pts.shape[0] == P and float(nr.texel_margin(pts, H, W, BOX).min()) >= MARGIN
    sigma, grad = _grad(plane, pts, dec)
    ref = nr.sigma_and_grad(plane, pts, dec, BOX)
    # sigma: its own fp32 forward pass (not shade64's), held to the bound render_refs.check_query holds the existing query's sigma to
    dd = rr.decoder(plane, pts, dec, BOX)
    rep = rr.Report('query_points_grad_kernel')
    rep.cmp('query_sigma', sigma, dd['sigma'], dd['sigma_scale'], rr.DEC_ULPS, 1, P)
    rep.raise_if_failed()
    # gradient: every component of every point
    err = (grad.double() - ref['grad']).abs()
    bound = GRAD_BOUND_ULPS * nr.F32_EPS * ref['scale']
    frac = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    print(f"[normals] query P={P} gain={gain}: worst {float(frac.max()):.3g} of the bound, {int(ref['all_padding'].sum())} points all padding")
    assert frac.numel() == 3 * P and bool(torch.isfinite(grad).all())
    assert bool((frac <= 1).all()), (int((frac > 1).sum()), float(frac.max()), pts[(frac > 1).any(-1)][:4])
    assert bool((grad[ref['all_padding']] == 0).all())
    if P > 64:
        assert int(ref['all_padding'].sum()) > 0 and int((~ref['all_padding']).sum()) > 0
    # binary16 texels: the f16 entry point on the rounded planes = the f32 entry point on their widened values, bit for bit
    s16, g16 = _grad(plane, pts, dec, f16=True)
    s32, g32 = _grad(plane.half().float(), pts, dec)
    assert torch.equal(s16.view(torch.int32), s32.view(torch.int32)) and torch.equal(g16.view(torch.int32), g32.view(torch.int32))


# ---------------------------------------------------------------- surface normals behind a render
def _render(inp):
    from ln3diff_amd import ops, _lib
    V, M = inp['V'], inp['M']
    d = {k: torch.empty(V * M * n, device='cuda') for k, n in (('rgb', 3), ('depth', 1), ('wsum', 1), ('lim', 2))}
    dev = dict(planes=_g(inp['planes']), pidx=_g(inp['plane_index']), cams=_g(inp['cams']), ray_o=_g(inp['ray_o']), ray_d=_g(inp['ray_d']),
               dec=tuple(_g(t) for t in inp['dec']))
    ops.render_triplane(dev['planes'], H, W, dev['pidx'], dev['cams'], inp['res'], dev['dec'], _g(inp['jitter']), _g(inp['u_fine']), d['rgb'],
                        d['depth'], d['wsum'], d['lim'], torch.zeros(_lib.RENDER_SCRATCH_FLOATS, device='cuda'), box_warp=BOX,
                        ray_o=dev['ray_o'], ray_d=dev['ray_d'], n_views=V, views_per_call=inp['views_per_call'],
                        rays_per_view=0 if inp['cams'] is not None else M)
    return dev, d['depth'], d['wsum']


def _normals(inp, dev, depth, wsum, planes=None, space='world', thr=0.5):
    from ln3diff_amd import ops
    V, M = inp['V'], inp['M']
    nrm, pts = torch.full((V * 3 * M + 8,), float('nan'), device='cuda'), torch.full((V * M * 3 + 8,), float('nan'), device='cuda')
    ops.surface_normals(dev['planes'] if planes is None else planes, H, W, dev['pidx'], dev['dec'], BOX, depth, wsum, nrm, cams=dev['cams'],
                        res=inp['res'], ray_o=dev['ray_o'], ray_d=dev['ray_d'], n_views=V, rays_per_view=0 if inp['cams'] is not None else M,
                        mask_threshold=thr, space=space, points=pts)
    torch.cuda.synchronize()
    nrm, pts = nrm.cpu(), pts.cpu()
    assert torch.isnan(nrm[V * 3 * M:]).all() and torch.isnan(pts[V * M * 3:]).all(), "the NaN tail behind an output was written"
    assert not torch.isnan(nrm[:V * 3 * M]).any() and not torch.isnan(pts[:V * M * 3]).any()
    return nrm[:V * 3 * M].reshape(V, 3, M).permute(0, 2, 1).contiguous(), pts[:V * M * 3].reshape(V, M, 3)


def _check_surface(inp, tag, thr=0.5):
    """both stages of ln3d_surface_normals on one scene -> (dev, depth, wsum, normals [V,M,3], mask [V,M])"""
    V, M = inp['V'], inp['M']
    dev, depth, wsum = _render(inp)
    n, p = _normals(inp, dev, depth, wsum, thr=thr)
    dep, ws = depth.cpu().reshape(V, M), wsum.cpu().reshape(V, M)
    on = ws >= thr
    assert bool((n[~on] == 0).all()) and bool((p[~on] == 0).all()), "a ray below the mask threshold is not exactly 0"
    # stage 1: the surface point, within render_refs.positions' budget with z = depth / wsum carrying the division's half ulp
    if inp['cams'] is not None:
        o, d, sd = rr.camera_rays(inp['cams'], inp['res'])
    else:
        o, d = inp['ray_o'].double(), inp['ray_d'].double()
        sd = torch.zeros_like(d)
    z = torch.where(on, dep.double() / ws.double(), torch.zeros_like(dep, dtype=torch.float64))[..., None]
    pref, sc = rr.positions(o, d, sd, z, 0.5 * z.abs())
    pref, sc = pref[:, :, 0], sc[:, :, 0]
    if inp['cams'] is None:
        assert torch.equal(pref[on], nr.surface_points(o, d, dep, ws)[0][on])
    f1 = ((p.double() - pref).abs() / (rr.STAGE_ULPS * nr.F32_EPS * sc).clamp(min=1e-300))[on]
    # stage 2: the normal at the kernel's own point
    pidx = inp['plane_index'].long()
    worst, left_out, compared = 0.0, 0, 0
    for v in range(V):
        sel = on[v].nonzero().reshape(-1)
        if sel.numel() == 0:
            continue
        pts = p[v, sel]
        ref = nr.sigma_and_grad(inp['planes'][int(pidx[v])], pts, inp['dec'], BOX)
        keep = nr.texel_margin(pts, H, W, BOX) >= RAY_MARGIN
        left_out += int((~keep).sum())
        has = ref['grad'].norm(dim=-1) > 0
        assert bool((n[v, sel][~has & keep] == 0).all())
        k = keep & has
        err = (n[v, sel][k].double() - nr.unit_outward(ref['grad'][k])).abs()
        frac = err / nr.normal_bound(ref['grad'][k], ref['scale'][k], GRAD_BOUND_ULPS)
        assert bool((frac <= 1).all()), (tag, v, int((frac > 1).sum()), float(frac.max()))
        unit = n[v, sel][k].double().norm(dim=-1)
        assert bool(((unit - 1).abs() <= 4 * nr.F32_EPS).all())
        worst, compared = max(worst, float(frac.max()) if frac.numel() else 0.0), compared + int(keep.sum())
    n_on = int(on.sum())
    print(f"[normals] {tag}: {n_on} / {V * M} rays on the surface, points worst {float(f1.max()) if n_on else 0:.3g}, normals worst {worst:.3g} of "
          f"the bound, {left_out} left out (texel margin < {RAY_MARGIN})")
    assert n_on == 0 or bool((f1 <= 1).all()), float(f1.max())
    assert left_out <= MAX_EXCLUDED * n_on, (left_out, n_on)              # a scene beyond the cap gets another seed, not a wider cap
    assert compared + left_out == n_on, "a ray on the surface was neither compared nor counted as left out"
    return dev, depth, wsum, n, on


@pytest.mark.parametrize("M", [1, 65, 300])
def test_surface_normals_explicit_rays(hip_lib, M):
    inp = _scene(300 + M, M=M, rays=rr.orbit_rays(3, M, 300 + M, spread=0.8))
    _, _, _, _, on = _check_surface(inp, f"explicit M={M}")            # asserts the left-out share <= 5 %: with 3 rays that means none
    if M > 1:
        assert 0 < int(on.sum()) < on.numel()          # both sides of the mask threshold occur


def _cams(V):
    from ln3diff_amd.synth import orbit_cameras
    return torch.cat([orbit_cameras(V, radius=(1.7719, 2.2, 1.5)[v % 3], elevation_deg=15.0 + 11 * v)[v:v + 1] for v in range(V)])


def test_surface_normals_camera_rays_spaces_and_f16(hip_lib):
    cams = _cams(3)
    inp = _scene(41, res=8, cams=cams, views_per_call=1, hidden_gain=12.0)
    dev, depth, wsum, n, on = _check_surface(inp, "cameras res=8")
    assert int(on.sum()) > 20
    # camera space = R^T x the world result, R the rotation of the view's cam2world
    nc, _ = _normals(inp, dev, depth, wsum, space='camera')
    R = cams[:, :16].reshape(3, 4, 4)[:, :3, :3].double()
    want = torch.einsum('vrc,vmr->vmc', R, n.double())
    assert float((nc.double() - want).abs().max()) <= 4 * nr.F32_EPS
    assert bool((nc[~on] == 0).all())
    # a higher threshold only removes rays
    n9, _ = _normals(inp, dev, depth, wsum, thr=0.999)
    on9 = wsum.cpu().reshape(3, -1) >= 0.999
    assert torch.equal(n9[on9], n[on9]) and bool((n9[~on9] == 0).all())
    # binary16 texels: same bits as the f32 entry point on the widened values (depth / wsum of the f32 render are only inputs here)
    p16 = dev['planes'].half()
    a, pa = _normals(inp, dev, depth, wsum, planes=p16)
    b, pb = _normals(inp, dev, depth, wsum, planes=p16.float())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(pa.view(torch.int32), pb.view(torch.int32))


def test_empty_scene_gives_an_all_zero_map(hip_lib):
    inp = _scene(77, M=65, sigma_bias=-60.0)
    dev, depth, wsum = _render(inp)
    assert float(wsum.max()) < 0.5
    n, p = _normals(inp, dev, depth, wsum)
    assert bool((n == 0).all()) and bool((p == 0).all())


# ---------------------------------------------------------------- module seams
def _triplane(dec):
    from ln3diff_amd.nsr.triplane import Triplane
    tp = Triplane(img_resolution=8)
    for layer, w, b in ((tp.decoder.net[0], dec[0], dec[1]), (tp.decoder.net[2], dec[2], dec[3])):
        layer.weight.data.copy_(w)
        layer.bias.data.copy_(b)
    return tp.cuda()


def _same(a, b, path=''):
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], path + k + '.')
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), path + k


def test_triplane_forward_return_normals_changes_no_other_key(hip_lib):
    inp = _scene(55, res=8, cams=_cams(3), views_per_call=1)
    tp = _triplane(inp['dec'])
    kw = dict(c=_g(inp['cams']), planes_channel_last=_g(inp['planes']), plane_index=_g(inp['plane_index']), jitter=inp['jitter'],
              u_fine=inp['u_fine'], views_per_call=1, return_debug=True)
    a, b = tp(**kw), tp(return_normals=True, **kw)
    assert set(b) == set(a) | {'image_normal'} and b['image_normal'].shape == (3, 3, 8, 8)
    _same(a, b)
    n = b['image_normal'].cpu()
    on = (b['weights_samples'].cpu() >= 0.5).expand(3, 3, 8, 8)
    assert int(on.sum()) > 0 and bool((n[~on] == 0).all())
    nn = n.norm(dim=1)[on[:, 0]]
    assert bool((((nn - 1).abs() <= 1e-6) | (nn == 0)).all())
    c = tp(return_normals=True, normal_space='camera', normal_mask_threshold=0.9, **kw)['image_normal'].cpu()
    assert bool((c[(b['weights_samples'].cpu() < 0.9).expand(3, 3, 8, 8)] == 0).all()) and not torch.equal(c, n)
    # the explicit-ray seam and the point query
    o, d = rr.orbit_rays(3, 65, 5, spread=0.5)
    r = tp.renderer(None, None, _g(o), _g(d), tp.rendering_kwargs, planes_channel_last=_g(inp['planes']), plane_index=_g(inp['plane_index']),
                    decoder_weights_dev=tp._decoder_dev(torch.device('cuda', 0)), return_normals=True)
    assert r['normal_samples'].shape == (3, 65, 3) and bool(torch.isfinite(r['normal_samples']).all())
    pts = nr.sample_points(300, 3, H, W, BOX, MARGIN)
    q0, q1 = tp.query_points(_g(inp['planes'][0]), _g(pts)), tp.query_points(_g(inp['planes'][0]), _g(pts), with_grad=True)
    assert set(q1) == set(q0) | {'sigma_grad', 'normal'} and q1['normal'].shape == (300, 3)
    _same(q0, q1)
    ref = nr.sigma_and_grad(inp['planes'][0], pts, inp['dec'], BOX)
    has = ref['grad'].norm(dim=-1) > 0
    assert bool((q1['normal'].cpu()[~has] == 0).all()) and int(has.sum()) > 0
    err = (q1['normal'].cpu().double()[has] - nr.unit_outward(ref['grad'][has])).abs()
    assert bool((err <= nr.normal_bound(ref['grad'][has], ref['scale'][has], GRAD_BOUND_ULPS)).all())


def _small_ae():
    from test_decode_gpu import build_decoder
    from ln3diff_amd.nsr.script_util import AE
    from conftest import load_synth
    dec = build_decoder(128, 2, 2)
    load_synth(dec, 3)
    dec.triplane_decoder.decoder.net[2].bias.data[0] += 4.0
    return AE(None, dec.cuda(), 16), dec


def test_render_video_given_triplane_normal_maps(hip_lib, tmp_path):
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    ae, _ = _small_ae()
    cams = orbit_cameras(3).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(6, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16, **kw)
    a = run()
    b = run(return_normals=True, export_mesh=True, mesh_normals=True, mesh_size=24, mesh_thres=4.0, mesh_path=str(tmp_path / 'm{}.obj'))
    assert 'image_normal' not in a and b['image_normal'].shape == (2, 3, 3, 16, 16)
    for k in ('image_raw', 'image_depth', 'weights_samples', 'image_mask'):
        assert torch.equal(a[k], b[k]), k
    assert len(b['mesh']) == 2 and all(len(m) == 4 and m[3].shape == m[0].shape for m in b['mesh'])
    v, vn, _, _ = parse_obj(tmp_path / 'm1.obj')
    assert len(v) == len(vn) == b['mesh'][1][0].shape[0]            # (this synthetic sample may have no surface at the level: test_mesh_vertex_normals has one)


# ---------------------------------------------------------------- mesh
class _Seams:
    """the renderer seams of a decoder class around one Triplane (what mesh_from_grid asks of its `decoder`)"""
    def __new__(cls, tp):
        from ln3diff_amd.vit.vit_triplane import _RendererSeams

        class D(_RendererSeams):
            pass
        d = D()
        d.triplane_decoder, d.rendering_kwargs = tp, tp.rendering_kwargs
        return d


def test_mesh_vertex_normals(hip_lib, tmp_path):
    from ln3diff_amd.mesh import mesh_from_grid
    G = 24
    inp = _scene(91, sigma_bias=10.0)
    tp = _triplane(inp['dec'])
    dec = _Seams(tp)
    pcl = _g(inp['planes'][1:2])
    sigma = dec.triplane_decode_grid({'planes_channel_last': pcl}, G)['sigma'][0]
    three = mesh_from_grid(dec, {'planes_channel_last': pcl}, sigma, G, thr=10.0)
    v, f, col, vn = mesh_from_grid(dec, {'planes_channel_last': pcl}, sigma, G, thr=10.0, path=str(tmp_path / 'm.obj'), normals=True)
    assert len(three) == 3 and np.array_equal(three[0], v) and np.array_equal(three[1], f) and np.array_equal(three[2], col)
    assert f.shape[0] > 100 and vn.shape == v.shape and vn.dtype == np.float32
    ln = np.linalg.norm(vn.astype(np.float64), axis=1)
    assert bool(((np.abs(ln - 1) <= 1e-6) | (ln == 0)).all())
    # against the reference at the vertices, in box coordinates: (x, y, z) -> (x, z, -y) undone
    back = lambda a: torch.from_numpy(np.stack([a[:, 0], -a[:, 2], a[:, 1]], 1))
    pts, n_box = back(v).float(), back(vn).double()
    ref = nr.sigma_and_grad(inp['planes'][1], pts, inp['dec'], BOX)
    keep = nr.texel_margin(pts, H, W, BOX) >= RAY_MARGIN
    has = ref['grad'].norm(dim=-1) > 0
    assert int((~keep).sum()) <= MAX_EXCLUDED * len(v), (int((~keep).sum()), len(v))
    assert bool((n_box[keep & ~has] == 0).all())
    k = keep & has
    # the vertices went to the GPU as fp32 (x, y, z) and came back through an exact permutation: the kernel saw exactly `pts`
    err = (n_box[k] - nr.unit_outward(ref['grad'][k])).abs()
    frac = err / nr.normal_bound(ref['grad'][k], ref['scale'][k], GRAD_BOUND_ULPS)
    print(f"[normals] mesh: {len(v)} vertices, {int((~keep).sum())} left out, worst {float(frac.max()):.3g} of the bound")
    assert int(k.sum()) + int((~keep).sum()) + int((keep & ~has).sum()) == len(v) and bool((frac <= 1).all()), float(frac.max())
    # orientation: the faces' winding against the vertex normals
    p0, p1, p2 = (v[f[:, i]].astype(np.float64) for i in range(3))
    fnrm = np.cross(p1 - p0, p2 - p0)
    fnrm /= np.maximum(np.linalg.norm(fnrm, axis=1, keepdims=True), 1e-30)
    vmean = (vn[f[:, 0]] + vn[f[:, 1]] + vn[f[:, 2]]).astype(np.float64) / 3
    agree = float((fnrm * vmean).sum(1).mean())
    print(f"[normals] mesh: mean dot(face normal of the winding, vertex normals) = {agree:.3f}")
    assert agree > 0
    pv, pvn, pf, pfn = parse_obj(tmp_path / 'm.obj')
    assert len(pv) == len(pvn) == len(v) and np.array_equal(pf, f) and all(a == b for a, b in zip(pfn, pf.tolist()))


# ---------------------------------------------------------------- launcher
def test_entry_point_writes_mesh_normals_and_normal_maps(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    flags = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 4 --image_size 32 --num_views 2 --mesh_grid 24 --dit_model_arch DiT-B/2 "
             "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.0 --export_mesh_normals true --save_normal_maps true "
             f"--logdir {tmp_path}")
    run(create_argparser(True).parse_args(flags.split()))
    frames = np.load(tmp_path / "frames_rank0.npy")
    for i in range(2):
        nm = np.load(tmp_path / f"normal_sample{i}.npy")
        assert nm.shape == (2, 3, 32, 32) and nm.dtype == np.float32 and np.isfinite(nm).all()
        ln = np.linalg.norm(nm, axis=1)
        assert bool(((np.abs(ln - 1) <= 1e-5) | (ln == 0)).all())
        v, vn, _, fn = parse_obj(tmp_path / f"mesh_sample{i}.obj")
        assert len(v) == len(vn) and (len(v) == 0 or fn[0] is not None)
    assert frames.shape == (4, 3, 32, 32)
    with pytest.raises(SystemExit):
        run(create_argparser(True).parse_args((flags.replace("--export_mesh true", "--export_mesh false") + "/b").split()))
