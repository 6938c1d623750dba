"""Opt-in fp16 tri-plane texels on the GPU (include/ln3d_planes16.h, Triplane.set_plane_precision('fp16')).

A storage format, not a change of arithmetic, and tested as one:
  * the converter is torch's `x.permute(...).clamp(-65504, 65504).half()`, bit for bit;
  * on planes rounded to fp16 the f16 entry points return the bits of the f32 entry points run on the same values widened back to f32
    (widening is exact and the evaluation order is the same), for render_kernel, render_generic_kernel and query_points_kernel, every
    output and debug output; the same outputs then pass the float64 checks of tests/render_refs.py with the bounds calibrated there;
  * what rounding the planes does to a picture is measured at full size against the fp32 path's picture and gated at 1.5x the measured
    value (the MX-FP8 tests' convention); against the reference golden the fp16 picture passes the fp32 path's own gates.
"""
import numpy as np
import pytest
import torch

import render_refs as rr
import test_render_stages_gpu as st
from conftest import golden, rel_l2

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ converter
def _special_values(x):
    """values beyond +-65504, +-0, fp16 subnormals, exact ties (to even, both ways), the overflow tie 65520 and a NaN, spread over x"""
    f = x.view(-1)
    sub = 2.0 ** -24
    vals = [1e5, -1e5, 65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 65536.0, 3.0e38, -3.0e38, float('inf'), float('-inf'),
            0.0, -0.0, sub, -sub, 3 * sub, 1023 * sub, 0.5 * sub, -0.5 * sub, 0.25 * sub, 0.75 * sub, 1.5 * sub, 2.5 * sub, 1e-30, -1e-30,
            1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2048.0 + 1.0, 2048.0 + 3.0, 1.0 + 2.0 ** -11 + 2.0 ** -20,
            2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, float('nan')]
    g = torch.Generator().manual_seed(5)
    pos = torch.randperm(f.numel(), generator=g)[:len(vals) * 3]
    f[pos] = torch.tensor(vals * 3)
    return x


@pytest.mark.parametrize("shape", [(1, 32, 16, 24), (2, 32, 256, 256)])
def test_converter_is_torch_clamp_half_bit_for_bit(hip_lib, shape):
    from ln3diff_amd import ops
    NP, C, H, W = shape
    g = torch.Generator().manual_seed(H)
    x = torch.randn(NP, 3 * C, H, W, generator=g) * torch.logspace(-9, 5, W)          # subnormals to overflow, column by column
    x = _special_values(x)
    want = x.view(NP, 3, C, H, W).permute(0, 1, 3, 4, 2).clamp(-65504, 65504).half().contiguous()
    out = torch.full((NP * 3 * H * W * C + 64,), -1.0, dtype=torch.float16, device='cuda')
    ops.planes_to_channel_last_f16(x.cuda(), out, NP, C, H, W)
    out = out.cpu()
    assert (out[-64:] == -1.0).all(), "the tail behind the output was written"
    got = out[:-64].view(NP, 3, H, W, C)
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.shape[0] == 0, (bad.shape[0], bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    assert not torch.isinf(got).any() and int(torch.isnan(got).sum()) == 3
    # the element-wise converter (channel-last f32 planes of a decoder) rounds the same way
    cl = x.view(NP, 3, C, H, W).permute(0, 1, 3, 4, 2).contiguous()
    out2 = torch.empty(cl.shape, dtype=torch.float16, device='cuda')
    ops.planes_f32_to_f16(cl.cuda(), out2)
    assert torch.equal(out2.cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ storage only
SCENES = {
    # ---- render_kernel (Objaverse 64 + 64)
    'fast_np3_shuffled': (dict(V=5, M=13, views_per_call=1, NP=3, plane_index=[2, 0, 2, 1, 1], S=64, NI=64), False, 21),
    'fast_np3_shuffled_s22': (dict(V=5, M=40, views_per_call=2, NP=3, plane_index=[1, 2, 0, 0, 2], S=64, NI=64), False, 22),
    'fast_cams': (dict(V=5, res=7, cams='orbit', views_per_call=2, NP=2, S=64, NI=64), False, 23),
    'fast_inside_128': (dict(V=2, M=67, rays='inside', H=128, W=128, NP=2, plane_index=[1, 0], S=64, NI=64), False, 24),
    'fast_misses': (dict(V=3, M=90, rays='wide', views_per_call=2, S=64, NI=64), False, 25),
    'fast_edges_8x8': (dict(V=2, M=65, H=8, W=8, jitter_edge=True, S=64, NI=64), False, 26),
    # ---- render_generic_kernel
    'gen_64_merged': (dict(V=3, M=65, views_per_call=2, NP=2, plane_index=[1, 0, 1], S=64, NI=64), True, 27),
    'gen_48_afhq': (dict(V=2, M=67, S=48, NI=48, numeric=(2.25, 3.3), box_warp=1.0, bbox=None, white_back=False, rays='far'), True, 28),
    'gen_80_eg3d_inside': (dict(V=2, M=40, S=80, NI=80, numeric=(0.1, 1.9), box_warp=1.1, bbox=None, rays='inside'), True, 29),
    'gen_shapenet': (dict(V=2, M=65, numeric=(0.6, 1.8), box_warp=1.2, bbox=None, H=16, W=24, S=64, NI=64), True, 30),
    'gen_128_cams': (dict(V=5, res=5, cams='orbit', views_per_call=2, S=128, NI=128, NP=2), False, 31),
    # ---- binary16 subnormals and signed zeros among the texels (the widening inside v_fma_mix_f32 against the f32 path's packed multiply)
    'fast_subnormal_texels': (dict(V=3, M=70, NP=2, plane_index=[1, 0, 1], S=64, NI=64, tiny=True), False, 32),
    'gen_subnormal_texels': (dict(V=2, M=65, S=48, NI=80, H=8, W=8, tiny=True), True, 33),
}


def _with_tiny_texels(planes, seed):
    """a third of the texel values scaled into binary16's subnormal range (|x| < 2^-14, multiples of 2^-24), a tenth set to +-0"""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(planes.shape, generator=g)
    p = torch.where(r < 0.33, planes * 2.0 ** -17, planes)
    p = torch.where(r > 0.9, torch.zeros_like(p) * planes.sign(), p)
    h = p.half()
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    assert int(sub.sum()) > 0.2 * h.numel() and int((h == 0).sum()) > 0.05 * h.numel() and bool((torch.signbit(h) & (h == 0)).any())
    return p


def _scene(name):
    kw, merged, seed = SCENES[name]
    kw = dict(kw)
    V, M = kw['V'], kw.get('M')
    if kw.get('cams') == 'orbit':
        kw['cams'] = st._cams(V)
    rays = kw.pop('rays', None)
    tiny = kw.pop('tiny', False)
    if rays == 'inside':
        kw['rays'] = rr.orbit_rays(V, M, seed, inside=True)
    elif rays == 'wide':
        kw['rays'] = rr.orbit_rays(V, M, seed, spread=1.2)
    elif rays == 'far':
        kw['rays'] = rr.orbit_rays(V, M, seed, radius=2.7, spread=0.3)
    inp = rr.make_scene(seed, **kw)
    if tiny:
        inp['planes'] = _with_tiny_texels(inp['planes'], seed)
    return inp, merged


def _both_ways(inp, merged, tag):
    """the f16 entry on the planes rounded to fp16, the f32 entry on the same values widened: equal outputs, and inside the float64 bounds"""
    ph = inp['planes'].half()
    wide = dict(inp, planes=ph.float())
    k16, o16 = st._run(dict(inp, planes=ph), merged)
    k32, o32 = st._run(wide, merged)
    assert k16 == k32 and set(o16) == set(o32)
    for k in o16:
        if k == 'ray_limits' and inp['numeric'] is not None:           # numeric limits: the slab-limit scratch is not written
            continue
        ne = (o16[k] != o32[k]).nonzero().reshape(-1)
        assert torch.equal(o16[k], o32[k]), (f"{tag} {k16} {k}: {ne.numel()} of {o16[k].numel()} elements differ between the f16 entry and the f32 "
                                             f"entry on the widened planes, first at {int(ne[0])}: {float(o16[k][ne[0]])!r} vs {float(o32[k][ne[0]])!r}")
    rep = rr.check_render(wide, o16, k16)
    print(f"[plane16] {tag} {k16} bit-equal in {sorted(o16)}; vs float64 " + " ".join(f"{k}={v:.3g}" for k, v in rep.worst.items()))
    rep.raise_if_failed()
    assert rep.notes.get('limits_without_margin', 0.0) <= 1e-3
    return o16


@pytest.mark.parametrize("name", list(SCENES))
def test_f16_texels_are_storage_only(hip_lib, name):
    inp, merged = _scene(name)
    _both_ways(inp, merged, name)


def test_planes_rows_and_channels_are_told_apart(hip_lib):
    """a scene whose three planes, tap rows, tap columns and channels carry different magnitudes on every axis (H != W, NP = 2, a
    shuffled plane_index): a wrong plane stride, row stride, texel size or channel offset in the f16 path moves an output far outside
    the float64 bounds and away from the f32 path's bits"""
    for merged, sizes in ((False, dict(S=64, NI=64)), (True, dict(S=48, NI=80))):
        inp = rr.make_scene(40, V=3, M=70, H=16, W=24, NP=2, plane_index=[1, 0, 1], **sizes)
        NP, _, H, W, C = inp['planes'].shape
        scale = ((1 + torch.arange(3).float()).view(1, 3, 1, 1, 1) * (1 + 0.11 * torch.arange(H).float()).view(1, 1, H, 1, 1)
                 * (1 + 0.07 * torch.arange(W).float()).view(1, 1, 1, W, 1) * (0.4 + 0.05 * torch.arange(C).float()).view(1, 1, 1, 1, C)
                 * (1 + torch.arange(NP).float()).view(NP, 1, 1, 1, 1))
        inp['planes'] = inp['planes'].sign() * (0.25 + inp['planes'].abs()) * scale * 0.25
        out = _both_ways(inp, merged, 'layout')
        assert float(out['coarse_sigma'].max()) > -1e30                # points inside the box were shaded


@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (128, 128)])
@pytest.mark.parametrize("P", [1, 65, 257, 4099])
def test_query_points_f16_is_storage_only(hip_lib, P, H, W):
    from ln3diff_amd import ops, _lib
    inp = rr.make_scene(60 + P, V=1, M=1, H=H, W=W, plane_scale=3.0, hidden_gain=2.0 if P % 2 else 1.0)
    if P == 257:
        inp['planes'] = _with_tiny_texels(inp['planes'], P)            # binary16 subnormals and +-0 among the texels
    pts = st._query_points(P, H, W, 0.9, P)                            # texel centres, box faces, points off the planes, points inside
    ph = inp['planes'].half()
    dpts, dec = pts.cuda(), tuple(t.cuda() for t in inp['dec'])
    res = []
    for planes in (ph.cuda(), ph.float().cuda()):
        sigma, rgb = st._buf(P, 'cuda'), st._buf(3 * P, 'cuda')
        scal = torch.zeros(_lib.RENDER_SCRATCH_FLOATS, device='cuda')
        ops.query_points(planes[0], H, W, dpts, dec, 0.9, sigma, rgb, scal)
        torch.cuda.synchronize()
        sigma, rgb = sigma.cpu(), rgb.cpu()
        assert torch.isnan(sigma[P:]).all() and torch.isnan(rgb[3 * P:]).all(), "the NaN tail behind an output was written"
        res.append((sigma[:P], rgb[:3 * P]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    rep = rr.check_query(dict(inp, planes=ph.float()), pts, res[0][0], res[0][1])
    print(f"[plane16] query P={P} {H}x{W} bit-equal; vs float64 " + " ".join(f"{k}={v:.3g}" for k, v in rep.worst.items()))
    rep.raise_if_failed()


def test_f16_planes_between_the_two_offset_limits(hip_lib):
    """tap offsets are 32-bit BYTE offsets inside one tri-plane, so binary16 planes may hold twice the texels of f32 ones: a 2048 x 4096
    tri-plane (1.6 GB in binary16) is past the f32 entry's limit and inside the f16 entry's.  All-zero planes give the decoder's output
    at zero features whatever the tap weights are: the bits of the same query on 8 x 8 zero planes, box corners (the largest offsets)
    included."""
    from ln3diff_amd import ops, _lib
    H, W = 2048, 4096
    assert 0x7fffffff // (3 * 32 * 4) < H * W <= 0x7fffffff // (3 * 32 * 2)
    inp = rr.make_scene(70, V=1, M=1, H=8, W=8)
    dec = tuple(t.cuda() for t in inp['dec'])
    pts = st._query_points(257, 8, 8, 0.9, 3).cuda()
    res = []
    for h, w in ((H, W), (8, 8)):
        planes = torch.zeros(3, h, w, 32, dtype=torch.float16, device='cuda')
        sigma, rgb = st._buf(257, 'cuda'), st._buf(3 * 257, 'cuda')
        ops.query_points(planes, h, w, pts, dec, 0.9, sigma, rgb, torch.zeros(_lib.RENDER_SCRATCH_FLOATS, device='cuda'))
        torch.cuda.synchronize()
        res.append((sigma.cpu(), rgb.cpu()))
        del planes
    assert not torch.isnan(res[0][0][:257]).any() and torch.isnan(res[0][0][257:]).all()
    assert torch.equal(res[0][0][:257], res[1][0][:257]) and torch.equal(res[0][1][:3 * 257], res[1][1][:3 * 257])
    with pytest.raises(RuntimeError, match='bad argument'):              # the f32 entry refuses the size before it touches the planes
        ops.query_points(torch.zeros(3, 8, 8, 32, device='cuda'), H, W, pts, dec, 0.9, st._buf(257, 'cuda'), st._buf(3 * 257, 'cuda'),
                         torch.zeros(_lib.RENDER_SCRATCH_FLOATS, device='cuda'))
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ what the rounding does to a picture
def test_fp16_planes_full_size_picture(hip_lib):
    """full_chain_ditl2 (tests/test_fullsize_gpu.py part 1): the reference's 250-step DiT-L/2 latent, decoded ONCE, rendered for 2 cameras at
    256^2 from fp32 planes and from fp16 planes with the same jitter.  The fp16 picture is held to the gates the fp32 path has against
    the reference golden there, and to 1.5x its measured distance from the fp32 picture."""
    from test_fullsize_gpu import _l2_decoder
    from ln3diff_amd.nsr.triplane import draw_render_noise
    g = golden('full_chain_ditl2')
    gl = golden('full_edm_ditl2_250')
    ae, dec = _l2_decoder(int(g['dec_seed']))
    tp = dec.triplane_decoder
    div, stride = float(g['divider']), int(g['stride'])
    cams = torch.from_numpy(g['cams']).cuda()
    lat = {'latent_normalized_2Ddiffusion': torch.from_numpy(gl['final']).float().cuda() * div}
    lat.update(ae(latent=lat, behaviour='decode_after_vae_no_render'))
    pcl32 = lat['planes_channel_last']
    assert pcl32.dtype == torch.float32
    pcl16 = tp.set_plane_precision('fp16').cast_planes(pcl32)
    tp.set_plane_precision('fp32')
    assert pcl16.dtype == torch.float16 and pcl16.shape == pcl32.shape
    assert torch.equal(pcl16.cpu(), pcl32.cpu().clamp(-65504, 65504).half())

    def picture(pcl):
        gen = torch.Generator().manual_seed(int(g['jitter_seed']))
        js, us = zip(*[draw_render_noise(1, 256 * 256, 64, generator=gen) for _ in range(2)])
        return tp(c=cams, planes_channel_last=pcl, plane_index=torch.zeros(2, dtype=torch.int32, device='cuda'), jitter=torch.cat(js),
                  u_fine=torch.cat(us), neural_rendering_resolution=256, views_per_call=1)

    def errors(out):
        e = {}
        for key, gk in (('image_raw', 'image_raw_sub'), ('image_depth', 'image_depth_sub'), ('weights_samples', 'weights_sub')):
            e[key] = rel_l2(out[key][:, :, ::stride, ::stride].cpu(), g[gk].astype(np.float32))
        e['rgb_mean_abs'] = float((out['image_raw'].mean((2, 3)).cpu() - torch.from_numpy(g['rgb_mean'])).abs().max())
        e['mask_mean_abs'] = float((out['image_mask'].mean((1, 2, 3)).cpu() - torch.from_numpy(g['mask_mean'])).abs().max())
        return e

    o32, o16 = picture(pcl32), picture(pcl16)
    e32, e16 = errors(o32), errors(o16)
    q = {k: rel_l2(o16[k], o32[k]) for k in ('image_raw', 'image_depth', 'weights_samples')}
    print('fp16 planes, full_chain_ditl2 @ 256^2: vs reference golden fp32', e32, 'fp16', e16, '| fp16 picture vs fp32 picture', q,
          '| planes absmax', float(pcl32.abs().max()), 'rel-L2 of the rounded planes', rel_l2(pcl16.float(), pcl32))
    assert all(torch.isfinite(o16[k]).all() for k in q)
    # the fp32 path's gates against the reference golden (tests/test_fullsize_gpu.py, golden latent -> decode + render)
    assert max(e16['image_raw'], e16['image_depth'], e16['weights_samples']) < 5e-3, e16
    assert e16['rgb_mean_abs'] < 2e-3 and e16['mask_mean_abs'] < 2e-3, e16
    assert q['image_raw'] < PIC_GATE, q


# measured on MI355X: fp16 picture vs the fp32 picture, rel-L2 of image_raw 1.888e-6 (image_depth 1.55e-7, weights_samples 2.78e-7; the planes
# themselves move by 2.08e-4 rel-L2, |planes| <= 4.5; against the reference golden both pictures sit at 3.41e-4); gate 1.5x
PIC_GATE = 2.83e-6


# ------------------------------------------------------------------------------------------------------------ mesh, drivers, launcher
def test_export_mesh_on_fp16_planes(hip_lib, tmp_path):
    """tests/test_render_gpu.py's grid16 scene (synthetic 128^2 planes x 4, sigma bias 4) through export_mesh in both precisions.
    Measured on MI355X, 64^3 grid at threshold 4: 240 967 vertices / 456 836 faces from fp32 planes, 240 964 / 456 832 from fp16 ones."""
    from ln3diff_amd.mesh import export_mesh
    from ln3diff_amd.synth import synth_input
    from test_decode_gpu import build_decoder
    from test_render_gpu import _decoder_sd
    dec = build_decoder(128, 2, 2)
    dec.triplane_decoder.decoder.load_state_dict(_decoder_sd(4.0))
    dec = dec.cuda()
    tp = dec.triplane_decoder
    planes = synth_input('planes', (1, 96, 128, 128), 3, 4.0).cuda()
    n = {}
    for prec, dt in (('fp32', torch.float32), ('fp16', torch.float16)):
        pcl = tp.set_plane_precision(prec).to_channel_last(planes)
        assert pcl.dtype == dt
        n[prec] = export_mesh(dec, {'planes_channel_last': pcl}, str(tmp_path / f'{prec}.obj'), grid_size=64, thr=4.0)
    tp.set_plane_precision('fp32')
    print('export_mesh grid 64^3, threshold 4: (vertices, faces) fp32', n['fp32'], 'fp16', n['fp16'])
    assert n['fp32'][0] > 0 and n['fp16'][0] > 0 and n['fp16'][1] > 0
    assert abs(n['fp16'][0] - n['fp32'][0]) <= 0.01 * n['fp32'][0], n


def test_render_video_given_triplane_plane_precision(hip_lib):
    """the drivers' switch holds for the call: 'fp16' renders finite frames that differ from the fp32 ones and leaves the renderer's own
    setting as it was, None renders with the renderer's setting, 'fp32' reproduces the fp32 frames bit for bit; the mesh path takes
    the f16 planes too"""
    from test_decode_gpu import build_decoder
    from ln3diff_amd.nsr.script_util import AE
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from conftest import load_synth
    dec = build_decoder(128, 2, 2)
    load_synth(dec, 3)
    dec.triplane_decoder.decoder.net[2].bias.data[0] += 4.0
    dec = dec.cuda()
    ae = AE(None, dec, 64)
    tp = dec.triplane_decoder
    cams = orbit_cameras(3).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    gen = torch.Generator().manual_seed(1)
    j, u = draw_render_noise(6, 64 * 64, 64, generator=gen)
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=64, **kw)
    a = run()
    assert tp.plane_precision == 'fp32' and a['planes_channel_last'].dtype == torch.float32
    b = run(plane_precision='fp16', export_mesh=True, mesh_size=32, mesh_thres=4.0)
    assert tp.plane_precision == 'fp32' and b['planes_channel_last'].dtype == torch.float16       # the renderer's setting is restored
    assert b['image_raw'].shape == (2, 3, 3, 64, 64) and all(torch.isfinite(b[k]).all() for k in ('image_raw', 'image_depth', 'weights_samples'))
    assert len(b['mesh']) == 2
    print('mesh vertices per sample on f16 planes', [m[0].shape[0] for m in b['mesh']])
    assert not torch.equal(a['image_raw'], b['image_raw'])
    e = rel_l2(b['image_raw'], a['image_raw'])
    print('render_video_given_triplane fp16 vs fp32 frames rel-L2', e)
    assert e < 1e-2                                                    # the same pictures: fp16 rounds the planes by 2^-11 relative
    a2 = run()                                                          # None after an 'fp16' call: the renderer's own fp32 again
    assert a2['planes_channel_last'].dtype == torch.float32 and torch.equal(a2['image_raw'], a['image_raw'])
    tp.set_plane_precision('fp16')
    b2 = run()                                                          # None: the renderer's setting, here fp16
    assert tp.plane_precision == 'fp16' and torch.equal(b2['image_raw'], b['image_raw'])
    with pytest.raises(ValueError):
        run(plane_precision='bf16')
    c = run(plane_precision='fp32')
    assert tp.plane_precision == 'fp16'                                 # a per-call 'fp32' does not stick either
    tp.set_plane_precision('fp32')
    for k in ('image_raw', 'image_depth', 'weights_samples', 'image_mask'):
        assert torch.equal(c[k], a[k]), k


def test_launcher_runs_with_fp16_planes(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    flags = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 4 --image_size 32 --num_views 2 --mesh_grid 24 --dit_model_arch DiT-B/2 "
             "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.0")
    lat = run(create_argparser(True).parse_args((flags + f" --plane_precision fp16 --logdir {tmp_path}/h").split()))
    lat32 = run(create_argparser(True).parse_args((flags + f" --logdir {tmp_path}/s").split()))
    assert torch.equal(lat, lat32)                                     # the sampler does not see the planes
    fh, fs = np.load(tmp_path / "h" / "frames_rank0.npy"), np.load(tmp_path / "s" / "frames_rank0.npy")
    assert fh.shape == (4, 3, 32, 32) and np.isfinite(fh).all() and np.isfinite(np.load(tmp_path / "h" / "depth_rank0.npy")).all()
    assert not np.array_equal(fh, fs) and rel_l2(fh, fs) < 1e-2
    assert (tmp_path / "h" / "mesh_sample0.obj").exists() and (tmp_path / "h" / "mesh_sample1.obj").exists()
    import json
    assert json.load(open(tmp_path / "h" / "args.json"))['plane_precision'] == 'fp16'


def _frames(run, create_argparser, flags, tmp_path, tag, extra=()):
    args = create_argparser(False).parse_known_args(list(flags) + list(extra) + ['--logdir', str(tmp_path / tag)])[0]
    lat = run(args)
    return lat, np.load(tmp_path / tag / 'frames_rank0.npy')


def test_flag_reaches_the_shapenet_decoder_class(hip_lib, tmp_path):
    """tests/test_shapenet_decoder_gpu.py's car-launcher flags with --plane_precision fp16: the class renders through Triplane, so the same
    latent gives finite frames that are not the fp32 planes' frames"""
    from ln3diff_amd.entry import create_argparser, run
    flags = ("--num_samples 1 --image_size 32 --num_views 2 --create_dit false --trainer_name vpsde_crossattn --num_channels 128 "
             "--num_res_blocks 1 --num_heads 4 --channel_mult 1,2 --attention_resolutions 32,16 --denoise_in_channels 12 "
             "--denoise_out_channels 12 --roll_out false --predict_v true --pred_type v --mixed_prediction true --use_ddim true "
             "--timestep_respacing ddim3 --decoder_in_chans 32 --out_chans 96 --decoder_output_dim 32 --arch_decoder vitb --vae_p 2 "
             "--cfg shapenet_tuneray_aug_resolution_64_64_nearestSR --ray_start 0.6 --ray_end 1.8 "
             "--ae_classname vit.vit_triplane.RodinSR_256_fusionv5_ConvQuant_liteSR_dinoInit3DAttn").split()
    lat16, f16 = _frames(run, create_argparser, flags, tmp_path, 'h', ['--plane_precision', 'fp16'])
    lat32, f32 = _frames(run, create_argparser, flags, tmp_path, 's')
    print('ShapeNet decoder class, fp16 vs fp32 frames rel-L2', rel_l2(f16, f32))
    assert torch.equal(lat16, lat32) and f16.shape == (2, 3, 32, 32) and np.isfinite(f16).all()
    assert not np.array_equal(f16, f32)


def test_flag_reaches_the_ffhq_decoder_class(hip_lib, tmp_path):
    """tests/test_ffhq_decoder_gpu.py's launcher flags (3 DDIM steps) with --plane_precision fp16"""
    import shlex
    from test_ffhq_decoder_gpu import LAUNCHER
    from ln3diff_amd.entry import create_argparser, run
    flags = shlex.split(LAUNCHER)
    for name in ('--prompt', '--resume_checkpoint', '--logdir', '--logdir'):
        i = flags.index(name)
        del flags[i:i + 2]
    flags[flags.index('--timestep_respacing') + 1] = 'ddim3'
    flags += ['--num_views', '2']
    lat16, f16 = _frames(run, create_argparser, flags, tmp_path, 'h', ['--plane_precision', 'fp16'])
    lat32, f32 = _frames(run, create_argparser, flags, tmp_path, 's')
    print('FFHQ decoder class, fp16 vs fp32 frames rel-L2', rel_l2(f16, f32))
    assert torch.equal(lat16, lat32) and f16.shape == (2, 3, 128, 128) and np.isfinite(f16).all() and f16.std() > 0
    assert not np.array_equal(f16, f32)
