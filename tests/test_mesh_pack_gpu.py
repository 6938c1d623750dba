"""The binary mesh export of include/ln3d_meshpack.h on the GPU (csrc/meshpack.hip):
  - the six packers against the numpy restatement (tests/mesh_pack_refs.py), byte for byte, at nv, nf in {1, 2, 3, 4, 5, 63, 64, 65, 257, 1000}
    (every phase of the 4-record period of the PLY words, a partial last word, wave and block edges, more than one block), with and without
    normals, rotated by a RANDOM matrix (the real rotation cannot show a fused multiply-add: tests/test_mesh_pack_cpu.py), on positions
    with +-0, subnormals and +-1e30, colours at every k / 255 with both float32 neighbours, -0.5, 1.5, +-inf and NaN, and indices 0 and
    nv - 1.  Every output sits inside a larger buffer of 0xA5 bytes, none of which may change; the pad bytes behind a record must be 0;
  - the bounds with the extreme in the first lane, the last lane of a wavefront and of a block, a lone tail element, and behind the point where
    the grid stops growing and the threads stride;
  - mesh_from_grid / textured_mesh_from_grid end to end on the real field of tests/test_mesh_bake_gpu.py: every file parsed back by the
    readers of mesh_pack_refs and held to the returned tuple; the default and mesh_format='obj' write the same bytes;
  - the pipeline and the launcher: --mesh_format glb, with and without --mesh_texture_size, writes one .glb per sample."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_pack_refs as R
from test_mesh_bake_gpu import scene                                   # noqa: F401  (a module-scoped fixture: built once here, never written)

pytestmark = pytest.mark.gpu

GUARD = 64                                   # bytes in front of and behind every output that a call must leave alone


def _guarded(nbytes, dtype=torch.uint8, shape=None):
    """(whole, view): nbytes (a multiple of 4) inside a buffer of 0xA5 bytes, GUARD on either side; the view as dtype / shape"""
    assert nbytes % 4 == 0
    whole = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    view = whole[GUARD:GUARD + nbytes].view(dtype)
    return whole, (view if shape is None else view.view(shape))


def _intact(whole, what):
    w = whole.cpu().numpy()
    assert (w[:GUARD] == 0xA5).all() and (w[-GUARD:] == 0xA5).all(), '%s: a byte outside the output was written' % what
    return w[GUARD:-GUARD].tobytes()


@functools.lru_cache(maxsize=None)
def _case(n):
    """R.case(n) and its device copies: made once, shared, never written"""
    c = R.case(n)
    return c, {k: torch.from_numpy(v).cuda() for k, v in c.items()}, torch.from_numpy(c['R'].reshape(-1).copy()).cuda()


# ---------------------------------------------------------------- the packers
@pytest.mark.parametrize('normals', [False, True])
@pytest.mark.parametrize('n', R.SIZES)
def test_ply_records_equal_the_restatement(hip_lib, n, normals):
    from ln3diff_amd import ops
    c, g, rot = _case(n)
    want_v, want_f = R.ply_body(c['xyz'], c['normal'] if normals else None, c['rgb'], c['faces'], c['R'])
    assert len(want_v) == (n * (27 if normals else 15) + 3) // 4 * 4 and len(want_f) == (n * 13 + 3) // 4 * 4
    whole, out = _guarded(len(want_v))
    ops.pack_ply_vertices(g['xyz'], g['normal'] if normals else None, g['rgb'], rot, out)
    got = _intact(whole, 'pack_ply_vertices')
    assert got == want_v, 'first differing byte: %d of %d' % (next(i for i in range(len(got)) if got[i] != want_v[i]), len(got))
    if not normals:
        whole, out = _guarded(len(want_f))
        ops.pack_ply_faces(g['faces'], out)
        got = _intact(whole, 'pack_ply_faces')
        assert got == want_f, 'first differing byte: %d of %d' % (next(i for i in range(len(got)) if got[i] != want_f[i]), len(got))
        assert c['faces'].min() == 0 and c['faces'].max() == n - 1


@pytest.mark.parametrize('normals', [False, True])
@pytest.mark.parametrize('n', R.SIZES)
def test_gltf_sections_equal_the_restatement(hip_lib, n, normals):
    from ln3diff_amd import ops
    c, g, rot = _case(n)
    normal, gnormal = (c['normal'], g['normal']) if normals else (None, None)
    # untextured: positions, normals, colours; indices
    want = R.gltf_sections(c['xyz'], normal, c['rgb'], c['faces'], R=c['R'])
    pw, pos = _guarded(12 * n, torch.float32, (n, 3))
    nw, nrm = _guarded(12 * n, torch.float32, (n, 3)) if normals else (None, None)
    cw, rgba = _guarded(4 * n, torch.uint8, (n, 4))
    iw, idx = _guarded(12 * n, torch.int32)
    ops.pack_gltf_vertices(g['xyz'], gnormal, g['rgb'], rot, pos, nrm, rgba)
    ops.pack_gltf_indices(g['faces'], idx)
    assert _intact(pw, 'pos_out') == want['POSITION'].tobytes() and _intact(cw, 'rgba_out') == want['COLOR_0'].tobytes()
    assert _intact(iw, 'idx_out') == want['indices'].tobytes()
    if normals:
        assert _intact(nw, 'nrm_out') == want['NORMAL'].tobytes()
    b6w, b6 = _guarded(24, torch.float32)
    ops.position_bounds(pos, b6)
    assert _intact(b6w, 'bounds6') == R.bounds(want['POSITION']).tobytes()
    # textured: the same rows per face corner, and (u, 1 - v)
    want = R.gltf_sections(c['xyz'], normal, c['rgb'], c['faces'], uv=c['uv'], R=c['R'])
    pw, pos = _guarded(36 * n, torch.float32, (3 * n, 3))
    nw, nrm = _guarded(36 * n, torch.float32, (3 * n, 3)) if normals else (None, None)
    uw, uvo = _guarded(24 * n, torch.float32, (3 * n, 2))
    ops.pack_gltf_corners(g['xyz'], gnormal, g['faces'], g['uv'], rot, pos, nrm, uvo)
    assert _intact(pw, 'pos_out') == want['POSITION'].tobytes() and _intact(uw, 'uv_out') == want['TEXCOORD_0'].tobytes()
    if normals:
        assert _intact(nw, 'nrm_out') == want['NORMAL'].tobytes()


@pytest.mark.parametrize('n,at', [(1, 0), (257, 0), (257, 63), (257, 255), (257, 256), (1000, 999), (1024 * 256 + 257, 1024 * 256 + 256),
                                  (1024 * 256 + 257, 1024 * 256 - 1)])
def test_bounds_find_an_extreme_wherever_it_sits(hip_lib, n, at):
    from ln3diff_amd import ops
    pos = np.random.default_rng(n + at).uniform(-0.45, 0.45, (n, 3)).astype(np.float32)
    pos[at] = (-7.5, 9.25, -1e30)                                                          # a minimum, a maximum, a minimum
    pos[(at + n // 2) % n, 2] = 1e30 if n > 1 else pos[at, 2]
    if n > 2:
        pos[(at + 1) % n, 0], pos[(at + 2) % n, 0] = 0.0, -0.0                             # a tie in value: the keys order it
    whole, b6 = _guarded(24, torch.float32)
    ops.position_bounds(torch.from_numpy(pos).cuda(), b6)
    got = np.frombuffer(_intact(whole, 'bounds6'), np.float32)
    assert R.bits(got).tolist() == R.bits(R.bounds(pos)).tolist() and got[0] == -7.5 and got[4] == 9.25 and got[2] == np.float32(-1e30)
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, 0.0, -0.0]], np.float32)
    ops.position_bounds(torch.from_numpy(zeros).cuda(), b6)
    assert R.bits(b6.cpu().numpy()).tolist() == R.bits(np.array([-0.0, -0.0, -0.0, 0.0, 0.0, 0.0], np.float32)).tolist()


def test_a_misaligned_output_is_refused_before_a_launch(hip_lib):
    from ln3diff_amd import ops
    c, g, rot = _case(5)
    whole = torch.full((GUARD + 80 + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    for shift in (1, 2, 3):
        with pytest.raises(RuntimeError, match='bad argument'):
            ops.pack_ply_vertices(g['xyz'], None, g['rgb'], rot, whole[GUARD + shift:GUARD + shift + 76])
        with pytest.raises(RuntimeError, match='bad argument'):
            ops.pack_ply_faces(g['faces'], whole[GUARD + shift:GUARD + shift + 68])
    assert bool((whole == 0xA5).all())


# ---------------------------------------------------------------- end to end on a real field
def _box_and_query(scene, **opts):                                     # noqa: F811
    """what _coloured_mesh has on the device for these options, made again by the same calls: (box-space vertices, normals or None) numpy"""
    from ln3diff_amd.mesh import extract_isosurface
    G, normals = scene['G'], opts.get('normals', False)
    v, f = extract_isosurface(scene['sigma'].reshape(G, G, G), 10.0, 'cubes', opts.get('keep', 'all'), opts.get('min_faces', 0), opts.get('simplify_cell', 0.0))
    vtx = (v / (G - 1) * 2 - 1) * 0.45
    q = scene['dec'].forward_points(scene['pcl'], vtx[None], with_grad=normals)
    return vtx.cpu().numpy(), (q['normal'][0].float().cpu().numpy() if normals else None)


def _held_to_the_tuple(what, pos, box, v):
    """pos: the positions read from a file; box: the box-space vertices; v: the returned vertices"""
    assert np.array_equal(R.bits(pos), R.bits(R.rotate(R.ROT_X_M90, box))), what            # the restatement, exactly
    bound = 2 * 3 * 2.0 ** -24 * (np.abs(R.ROT_X_M90.astype(np.float64))[None] * np.abs(box.astype(np.float64))[:, None, :]).sum(-1)
    differ = int((R.bits(pos) != R.bits(v)).sum())
    print('[pack] %s: %d of %d position bit patterns differ from the returned vertices (0 expected)' % (what, differ, pos.size))
    assert (np.abs(pos.astype(np.float64) - v.astype(np.float64)) <= bound).all(), what


@pytest.mark.parametrize('opts', [{}, dict(normals=True), dict(simplify_cell=2.0), dict(normals=True, simplify_cell=2.0)])
@pytest.mark.parametrize('fmt', ['ply', 'glb'])
def test_mesh_from_grid_writes_what_it_returns(scene, tmp_path, fmt, opts):                # noqa: F811
    from ln3diff_amd.mesh import mesh_from_grid
    dec, d, sigma, G = scene['dec'], {'planes_channel_last': scene['pcl']}, scene['sigma'], scene['G']
    normals = opts.get('normals', False)
    base = mesh_from_grid(dec, d, sigma, G, thr=10.0, **opts)
    got = mesh_from_grid(dec, d, sigma, G, thr=10.0, path=str(tmp_path / 'm.bin'), mesh_format=fmt, **opts)       # the extension is not interpreted
    assert len(got) == len(base) == (4 if normals else 3) and got[1].shape[0] > 50
    for a, b in zip(base, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()                            # the tuple, bit for bit
    v, f, colors = got[:3]
    box, qn = _box_and_query(scene, **opts)
    data = open(tmp_path / 'm.bin', 'rb').read()
    assert sorted(os.listdir(tmp_path)) == ['m.bin']
    if fmt == 'ply':
        p = R.parse_ply(data)
        assert data.startswith(R.ply_header(len(v), len(f), normals))                     # the header of the feature's definition, exactly
        pos, nrm, rgb, faces = p['xyz'], p['normal'], p['rgb'], p['faces']
        assert len(data) == len(R.ply_header(len(v), len(f), normals)) + len(v) * (27 if normals else 15) + len(f) * 13
    else:
        g = R.parse_glb(data)
        a = g['arrays']
        assert list(a) == ['POSITION'] + (['NORMAL'] if normals else []) + ['COLOR_0', 'indices'] and g['image'] is None
        pos, nrm, rgb, faces = a['POSITION'], a.get('NORMAL'), a['COLOR_0'][:, :3], a['indices'].reshape(-1, 3)
        assert (a['COLOR_0'][:, 3] == 255).all()
        acc = g['json']['accessors'][0]
        assert acc['min'] == [float(x) for x in pos.min(0)] and acc['max'] == [float(x) for x in pos.max(0)]
    assert np.array_equal(faces, f) and np.array_equal(rgb, colors)
    _held_to_the_tuple(fmt + ' positions', pos, box, v)
    if normals:
        assert np.array_equal(R.bits(nrm), R.bits(R.rotate(R.ROT_X_M90, qn)))
        assert np.abs(nrm.astype(np.float64) - got[3].astype(np.float64)).max() <= 2 * 3 * 2.0 ** -24 * 2
    else:
        assert nrm is None


@pytest.mark.parametrize('normals', [False, True])
def test_textured_glb_holds_the_bake(scene, tmp_path, normals):                            # noqa: F811
    from ln3diff_amd.mesh import atlas_layout, png_bytes, textured_mesh_from_grid
    dec, d, sigma, G = scene['dec'], {'planes_channel_last': scene['pcl']}, scene['sigma'], scene['G']
    opts = dict(simplify_cell=2.0, normals=normals)
    nf = scene['faces'].shape[0]
    T = 4 * atlas_layout(nf, 8192)[0] + 2
    base = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, **opts)
    got = textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, path=str(tmp_path / 'm.glb'), mesh_format='glb', **opts)
    for a, b in zip(base, got):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    v, f = got[:2]
    uv, tex = got[-2:]
    assert len(f) == nf and sorted(os.listdir(tmp_path)) == ['m.glb']                       # no .mtl or .png siblings
    g = R.parse_glb(open(tmp_path / 'm.glb', 'rb').read())
    a = g['arrays']
    assert list(a) == ['POSITION'] + (['NORMAL'] if normals else []) + ['TEXCOORD_0'] and all(x.shape[0] == 3 * nf for x in a.values())
    box, qn = _box_and_query(scene, **opts)
    corner = f.reshape(-1)
    _held_to_the_tuple('textured glb positions', a['POSITION'], box[corner], v[corner])
    if normals:
        assert np.array_equal(R.bits(a['NORMAL']), R.bits(R.rotate(R.ROT_X_M90, qn)[corner]))
    flat = uv.reshape(-1, 2)
    assert np.array_equal(a['TEXCOORD_0'][:, 0], flat[:, 0]) and np.array_equal(a['TEXCOORD_0'][:, 1], np.float32(1) - flat[:, 1])
    assert g['image'] == png_bytes(tex) and g['json']['materials'][0]['pbrMetallicRoughness']['baseColorTexture'] == {'index': 0}
    with pytest.raises(ValueError, match="format 'ply'"):
        textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, texture_size=T, path=str(tmp_path / 'm.ply'), mesh_format='ply', **opts)
    assert sorted(os.listdir(tmp_path)) == ['m.glb']


def test_empty_level_set_and_the_default_format(scene, tmp_path):                          # noqa: F811
    from ln3diff_amd.mesh import mesh_from_grid, textured_mesh_from_grid
    dec, d, sigma, G = scene['dec'], {'planes_channel_last': scene['pcl']}, scene['sigma'], scene['G']
    for normals in (False, True):
        out = mesh_from_grid(dec, d, sigma, G, thr=10.0, min_faces=10 ** 6, normals=normals, path=str(tmp_path / 'e.ply'), mesh_format='ply')
        data = open(tmp_path / 'e.ply', 'rb').read()
        assert [a.shape for a in out[:3]] == [(0, 3)] * 3 and data == R.ply_header(0, 0, normals) and R.parse_ply(data)['nf'] == 0
        mesh_from_grid(dec, d, sigma, G, thr=10.0, min_faces=10 ** 6, normals=normals, path=str(tmp_path / 'e.glb'), mesh_format='glb')
        g = R.parse_glb(open(tmp_path / 'e.glb', 'rb').read())
        assert g['bin'] is None and g['json']['scenes'] == [{}]
    textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, min_faces=10 ** 6, texture_size=16, path=str(tmp_path / 't.glb'), mesh_format='glb')
    assert R.parse_glb(open(tmp_path / 't.glb', 'rb').read())['bin'] is None
    # the default and 'obj': the same files, the same bytes
    for name, kw in (('default', {}), ('obj', dict(mesh_format='obj'))):
        os.makedirs(tmp_path / name)
        mesh_from_grid(dec, d, sigma, G, thr=10.0, normals=True, simplify_cell=2.0, path=str(tmp_path / name / 'm.obj'), **kw)
        textured_mesh_from_grid(dec, d, sigma, G, thr=10.0, simplify_cell=2.0, texture_size=256, path=str(tmp_path / name / 't.obj'), **kw)
    assert sorted(os.listdir(tmp_path / 'default')) == sorted(os.listdir(tmp_path / 'obj')) == ['m.obj', 't.mtl', 't.obj', 't.png']
    for n in os.listdir(tmp_path / 'default'):
        assert open(tmp_path / 'default' / n, 'rb').read() == open(tmp_path / 'obj' / n, 'rb').read(), n


# ---------------------------------------------------------------- pipeline and launcher
def test_render_video_given_triplane_mesh_format(hip_lib, tmp_path):
    from ln3diff_amd.nsr.triplane import draw_render_noise
    from ln3diff_amd.pipeline import render_video_given_triplane
    from ln3diff_amd.synth import synth_input, orbit_cameras
    from test_normals_gpu import _small_ae
    ae, _ = _small_ae()
    cams = orbit_cameras(1).cuda()
    lat = synth_input('z', (2, 12, 32, 32), 7).cuda()
    j, u = draw_render_noise(2, 16 * 16, 64, generator=torch.Generator().manual_seed(1))
    d = {'latent_normalized_2Ddiffusion': lat.clone()}                                     # the level: inside the synthetic sample's own densities
    d.update(ae(latent=d, behaviour='decode_after_vae_no_render'))
    if d.get('planes_channel_last') is not None:
        d['planes_channel_last'] = ae.decoder.triplane_decoder.cast_planes(d['planes_channel_last'])
    thr = float(torch.quantile(ae(latent=d, grid_size=16, behaviour='triplane_decode_grid')['sigma'][0].float().flatten(), 0.8))
    run = lambda **kw: render_video_given_triplane(lat.clone(), ae, cams, triplane_scaling_divider=1.0, jitter=j, u_fine=u, resolution=16,       # noqa: E731
                                                   export_mesh=True, mesh_size=16, mesh_thres=thr, mesh_simplify_cell=2.0, **kw)
    a = run()
    p = run(mesh_format='ply', mesh_path=str(tmp_path / 'm{}.ply'))
    t = run(mesh_format='glb', mesh_texture_size=128, mesh_path=str(tmp_path / 't{}.glb'))
    for k in ('image_raw', 'image_depth', 'weights_samples'):
        assert torch.equal(a[k], p[k]) and torch.equal(a[k], t[k]), k
    for i, (ma, mp, mt) in enumerate(zip(a['mesh'], p['mesh'], t['mesh'])):
        assert len(mp) == 3 and len(mt) == 5 and all(np.array_equal(x, y) for x, y in zip(ma, mp)) and all(np.array_equal(x, y) for x, y in zip(ma, mt))
        ply = R.parse_ply(open(tmp_path / f'm{i}.ply', 'rb').read())
        assert np.array_equal(ply['faces'], ma[1]) and np.array_equal(ply['rgb'], ma[2]) and ply['normal'] is None and len(ma[1]) > 2
        glb = R.parse_glb(open(tmp_path / f't{i}.glb', 'rb').read())
        assert glb['arrays']['POSITION'].shape == (3 * len(ma[1]), 3) and glb['image'][:8] == b'\x89PNG\r\n\x1a\n'
    assert sorted(os.listdir(tmp_path)) == ['m0.ply', 'm1.ply', 't0.glb', 't1.glb']
    with pytest.raises(ValueError, match="format 'ply'"):
        run(mesh_format='ply', mesh_texture_size=128)


def test_entry_point_mesh_format(hip_lib, tmp_path):
    from ln3diff_amd.entry import create_argparser, run
    base = ("--arch_dit_decoder DiT2-B/2 --num_samples 2 --sample_steps 2 --image_size 32 --num_views 1 --mesh_grid 24 --dit_model_arch DiT-B/2 "
            "--trainer_name sgm_legacy --export_mesh true --mesh_thres 4.7 --mesh_simplify_cell 2 ")      # the synthetic decoder's densities lie in [4.1, 5.1]
    go = lambda flags, out: run(create_argparser(True).parse_args((base + flags + f" --logdir {tmp_path / out}").split()))        # noqa: E731
    go("", 'plain')
    go("--mesh_format obj", 'obj')
    go("--mesh_format glb", 'glb')
    go("--mesh_format glb --mesh_texture_size 256", 'tex')
    meta = {k: json.load(open(tmp_path / k / 'args.json')) for k in ('plain', 'obj', 'glb', 'tex')}
    assert 'mesh_format' not in meta['plain'] and 'mesh_format' not in meta['obj'] and meta['glb']['mesh_format'] == meta['tex']['mesh_format'] == 'glb'
    assert {k: v for k, v in meta['glb'].items() if k not in ('mesh_format', 'logdir')} == {k: v for k, v in meta['plain'].items() if k != 'logdir'}
    # the default run writes the files and the bytes it wrote before the flag existed: the same as an explicit obj
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(os.listdir(tmp_path / 'obj'))
    assert [n for n in sorted(os.listdir(tmp_path / 'plain')) if n.startswith('mesh_')] == ['mesh_sample0.obj', 'mesh_sample1.obj']
    for i in range(2):
        assert open(tmp_path / 'plain' / f'mesh_sample{i}.obj', 'rb').read() == open(tmp_path / 'obj' / f'mesh_sample{i}.obj', 'rb').read()
    for out in ('glb', 'tex'):
        assert [n for n in sorted(os.listdir(tmp_path / out)) if n.startswith('mesh_')] == ['mesh_sample0.glb', 'mesh_sample1.glb']
    from test_normals_cpu import parse_obj
    for i in range(2):
        _, _, pf, _ = parse_obj(tmp_path / 'plain' / f'mesh_sample{i}.obj')
        plain, tex = (R.parse_glb(open(tmp_path / out / f'mesh_sample{i}.glb', 'rb').read()) for out in ('glb', 'tex'))
        assert np.array_equal(plain['arrays']['indices'].reshape(-1, 3), pf) and len(pf) > 2
        assert tex['arrays']['TEXCOORD_0'].shape == (3 * len(pf), 2) and tex['image'][:8] == b'\x89PNG\r\n\x1a\n' and plain['image'] is None
    with pytest.raises(SystemExit, match='mesh_texture_size'):
        go("--mesh_format ply --mesh_texture_size 256", 'bad')
    with pytest.raises(SystemExit, match='mesh_format'):
        go("--mesh_format stl", 'bad')
    assert not os.path.exists(tmp_path / 'bad' / 'args.json')                              # refused before sampling
