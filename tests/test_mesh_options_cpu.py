"""The nine mesh options of mesh.MeshPost - mesh_normals, mesh_keep, mesh_min_faces, mesh_simplify_cell, mesh_simplify_placement,
mesh_smooth_iters, mesh_snap_iters, mesh_texture_size, mesh_format - from every public entry of ln3diff_amd.pipeline down to the two mesh
functions, without a GPU and without the library: the real pipeline code runs over a stub decoder (CPU zero tensors) in a real AE, sampling
is stubbed out, and mesh.mesh_from_grid and mesh.textured_mesh_from_grid are replaced by recorders of the keywords they are given.
  - every entry delivers the WHOLE record, with the values given or the defaults, once per sample and in order, to the textured function
    exactly when texture_size is not 0 (the plain one gets every field but texture_size);
  - a misspelt keyword is a TypeError at every entry, whether or not a mesh is exported;
  - without export_mesh a bad value is ignored and neither function is called;
  - the record, its keywords and the launcher's flags are the nine, with their defaults; the launcher accepts and refuses what it did;
  - the real mesh_from_grid hands the record's fields on to extract_isosurface and forward_points."""
import numpy as np
import pytest
import torch

B, V, G, R = 2, 3, 8, 4                      # samples, cameras, mesh grid, render resolution
DEFAULTS = dict(normals=False, keep='all', min_faces=0, simplify_cell=0.0, simplify_placement='mean', smooth_iters=0, snap_iters=0,
                texture_size=0, mesh_format='obj')
ALL = dict(mesh_normals=True, mesh_keep='largest', mesh_min_faces=7, mesh_simplify_cell=2.5, mesh_simplify_placement='quadric',
           mesh_smooth_iters=3, mesh_snap_iters=5, mesh_texture_size=64, mesh_format='glb')          # pairwise distinct: a crossed wire shows
FIELD = dict(zip(ALL, DEFAULTS))             # keyword -> field
MISSPELT = dict(mesh_normals='mesh_normal', mesh_keep='mesh_kep', mesh_min_faces='mesh_min_face', mesh_simplify_cell='mesh_simplify_cel',
                mesh_simplify_placement='mesh_simplify_placment', mesh_smooth_iters='mesh_smooth_iter', mesh_snap_iters='mesh_snap_iter',
                mesh_texture_size='mesh_texture_sizes', mesh_format='mesh_formats')
OPTION_SETS = [{}] + [{k: v} for k, v in ALL.items()] + [ALL]


def _latent():
    return torch.zeros(B, 12, 4, 4)


class _Planes:
    plane_precision = 'fp32'
    neural_rendering_resolution = R

    def set_plane_precision(self, p):
        self.plane_precision = p

    def cast_planes(self, x):
        return x


class _Decoder:
    def __init__(self):
        self.triplane_decoder = _Planes()
        self.points = []

    def vit_decode_backbone(self, ret_dict, img_size):
        return ret_dict

    def vit_decode_postprocess(self, latent, ret_dict):
        return {'planes_channel_last': torch.zeros(B, 3, 4, 4, 2)}

    def triplane_decode(self, latent, c, return_raw_only=False, **kw):
        r = kw.get('neural_rendering_resolution', R)
        z = lambda ch: torch.zeros(c.shape[0], ch, r, r)                                          # noqa: E731
        return {'image_raw': z(3), 'image_depth': z(1), 'weights_samples': z(1), 'image_mask': z(1)}

    def triplane_decode_grid(self, latent, grid_size):
        return {'sigma': torch.zeros(B, grid_size ** 3, 1)}

    def vae_reparameterization(self, h, sample, eps=None, num_frames=None):
        return {'latent_normalized_2Ddiffusion': _latent()}

    def forward_points(self, pcl, pts, with_grad=False):
        self.points.append(with_grad)
        return {'rgb': torch.zeros_like(pts), 'normal': torch.zeros_like(pts)}


class _Encoder:
    num_frames = 1

    def forward_frames(self, img):
        return img


def _ae():
    from ln3diff_amd.nsr.script_util import AE
    ae = AE(None, _Decoder(), R)
    ae.encoder = _Encoder()
    return ae


def _entries():
    """name -> (call(export_mesh, **mesh keywords), whether the entry takes mesh_normals)"""
    from ln3diff_amd import pipeline as P
    ae, cams, cond = _ae(), torch.zeros(V, 25), {'crossattn': torch.zeros(1, 1, 1)}
    common = dict(mesh_size=G, resolution=R, mesh_path='m{}.bin')
    t23d = P.T23DPipeline(None, ae)
    flow = P.FlowMatchingEngine(None, ae, conditioner=lambda img: cond)
    gd = P.GuidedDiffusionEngine(None, ae, None)
    for eng in (t23d, flow, gd):
        eng.sample = lambda *a, **k: _latent()
    return {
        'render_video_given_triplane': (lambda e, **kw: P.render_video_given_triplane(_latent(), ae, cams, export_mesh=e, **common, **kw), True),
        'T23DPipeline.eval_cldm': (lambda e, **kw: t23d.eval_cldm(cond, cams, num_samples=B, export_mesh=e, **common, **kw), True),
        'T23DPipeline.render_video_given_triplane': (lambda e, **kw: t23d.render_video_given_triplane(_latent(), cams, export_mesh=e, **common, **kw), True),
        'FlowMatchingEngine.eval_cldm': (lambda e, **kw: flow.eval_cldm(cond, cams, num_samples=B, export_mesh=e, **common, **kw), True),
        'FlowMatchingEngine.eval_i23d_and_export': (lambda e, **kw: flow.eval_i23d_and_export(None, cams, num_samples=B, export_mesh=e, **common, **kw), False),
        'FlowMatchingEngine.render_video_given_triplane': (lambda e, **kw: flow.render_video_given_triplane(_latent(), cams, export_mesh=e, **common, **kw), True),
        'GuidedDiffusionEngine.eval_cldm': (lambda e, **kw: gd.eval_cldm(cond, cams, export_mesh=e, **common, **kw), True),
        'GuidedDiffusionEngine.eval_ddpm_sample': (lambda e, **kw: gd.eval_ddpm_sample(cams, export_mesh=e, **common, **kw), True),
        'GuidedDiffusionEngine.render_video_given_triplane': (lambda e, **kw: gd.render_video_given_triplane(_latent(), cams, export_mesh=e, **common, **kw), True),
        'reconstruct': (lambda e, **kw: P.reconstruct(ae, torch.zeros(B, 10, 4, 4), cams, export_mesh=e, **common, **kw), True),
    }


ENTRIES = ['render_video_given_triplane', 'T23DPipeline.eval_cldm', 'T23DPipeline.render_video_given_triplane', 'FlowMatchingEngine.eval_cldm',
           'FlowMatchingEngine.eval_i23d_and_export', 'FlowMatchingEngine.render_video_given_triplane', 'GuidedDiffusionEngine.eval_cldm',
           'GuidedDiffusionEngine.eval_ddpm_sample', 'GuidedDiffusionEngine.render_video_given_triplane', 'reconstruct']
NOTHING = {'plain': [], 'textured': []}


@pytest.fixture
def recorder(monkeypatch):
    """{'plain': [...], 'textured': [...]}: the keywords of every call of mesh.mesh_from_grid / mesh.textured_mesh_from_grid"""
    from ln3diff_amd import mesh
    calls = {'plain': [], 'textured': []}
    e3, ef = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)

    def plain(decoder, dec_out, sigma, grid_size, thr=10.0, **kw):
        assert grid_size == G and sigma.numel() == G ** 3
        calls['plain'].append(kw)
        return e3, ef, e3.astype(np.uint8)

    def textured(decoder, dec_out, sigma, grid_size, thr=10.0, **kw):
        assert grid_size == G and sigma.numel() == G ** 3
        calls['textured'].append(kw)
        return e3, ef, e3.astype(np.uint8), np.zeros((0, 3, 2), np.float32), np.zeros((kw['texture_size'],) * 2 + (3,), np.uint8)
    monkeypatch.setattr(mesh, 'mesh_from_grid', plain)
    monkeypatch.setattr(mesh, 'textured_mesh_from_grid', textured)
    return calls


def _strip(kw):
    return {k: v for k, v in kw.items() if k not in ('sample_index', 'path')}


def _out(o):
    return o[1] if isinstance(o, tuple) else o


def test_the_entries_are_all_covered():
    assert list(_entries()) == ENTRIES


@pytest.mark.parametrize('entry', ENTRIES)
def test_options_reach_the_mesh_functions(recorder, entry):
    call, takes_normals = _entries()[entry]
    for given in OPTION_SETS:
        if not takes_normals:
            given = {k: v for k, v in given.items() if k != 'mesh_normals'}
        for calls in recorder.values():
            del calls[:]
        out = _out(call(True, **given))
        want = dict(DEFAULTS, **{FIELD[k]: v for k, v in given.items()})
        used, other = ('textured', 'plain') if want['texture_size'] else ('plain', 'textured')
        if used == 'plain':
            del want['texture_size']                                                               # every field but this one
        assert recorder[other] == [], (entry, given)
        assert [kw['sample_index'] for kw in recorder[used]] == list(range(B)), (entry, given)    # every sample once, in order
        assert [kw['path'] for kw in recorder[used]] == ['m%d.bin' % i for i in range(B)]          # the extension is the caller's
        for kw in recorder[used]:
            assert _strip(kw) == want, (entry, given, kw)
        assert len(out['mesh']) == B and out['image_raw'].shape == (B, V, 3, R, R)
        assert all(len(m) == (5 if used == 'textured' else 3) for m in out['mesh'])
        if used == 'textured':
            assert all(m[4].shape == (64, 64, 3) for m in out['mesh'])


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_misspelt_option_is_a_type_error(recorder, entry):
    call, _ = _entries()[entry]
    for keyword, misspelt in MISSPELT.items():
        for export in (True, False):
            with pytest.raises(TypeError, match=misspelt):
                call(export, **{misspelt: ALL[keyword]})
            assert recorder == NOTHING


@pytest.mark.parametrize('entry', ENTRIES)
def test_options_are_ignored_without_export(recorder, entry):
    call, takes_normals = _entries()[entry]
    for keyword, value in ALL.items():
        if keyword == 'mesh_normals' and not takes_normals:
            continue
        for v in (value, 'bogus'):                                                                 # a good value and a bad one alike
            out = _out(call(False, **{keyword: v}))
            assert 'mesh' not in out and recorder == NOTHING, (entry, keyword, v)


def test_the_record_its_keywords_and_the_launcher_flags():
    from ln3diff_amd import mesh
    from ln3diff_amd.entry import _MESH_FLAGS
    assert mesh.MeshPost._fields == tuple(DEFAULTS) and mesh.MeshPost()._asdict() == DEFAULTS and mesh.MeshPost() == tuple(DEFAULTS.values())
    assert [mesh.MeshPost.keyword(f) for f in mesh.MeshPost._fields] == list(ALL)
    assert _MESH_FLAGS == dict(zip(['export_mesh_normals'] + list(ALL)[1:], DEFAULTS.values())) and list(_MESH_FLAGS)[0] == 'export_mesh_normals'
    for keyword, value in ALL.items():                                                             # every field round-trips alone ...
        assert mesh.MeshPost.from_kwargs({keyword: value}) == mesh.MeshPost(**{FIELD[keyword]: value})
    assert mesh.MeshPost.from_kwargs(ALL) == tuple(ALL.values()) and mesh.MeshPost.from_kwargs({}) == mesh.MeshPost()      # ... and together
    for bad in ('min_faces', 'mesh_size', 'mesh_', 'format', 'mesh_mesh_format'):
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{bad}'"):
            mesh.MeshPost.from_kwargs({bad: 1})


def test_mesh_from_grid_hands_the_record_on(monkeypatch):
    from ln3diff_amd import mesh
    seen = []

    def isosurface(sigma, thr, method, *post, **kw):
        seen.append((post, kw))
        return torch.tensor([[1.0, 2.0, 3.0]]), torch.zeros(0, 3, dtype=torch.int64)
    monkeypatch.setattr(mesh, 'extract_isosurface', isosurface)
    dec = _Decoder()
    d, sigma = dec.vit_decode_postprocess(None, None), torch.zeros(G ** 3)
    out = mesh.mesh_from_record(dec, d, sigma, G, 10.0, 0, None, mesh.MeshPost(True, 'largest', 7, 2.5, 'quadric'))
    assert seen == [(('largest', 7, 2.5), dict(simplify_placement='quadric'))] and dec.points == [True] and len(out) == 4
    out = mesh.mesh_from_record(dec, d, sigma, G, 10.0, 0, None, mesh.MeshPost())
    assert seen[1] == (('all', 0, 0.0), {}) and dec.points == [True, False] and len(out) == 3                # 'mean': the extraction is called as it always was
    with pytest.raises(TypeError, match='texture_size'):                                           # the plain function has no such keyword
        mesh.mesh_from_grid(dec, d, sigma, G, texture_size=0)
    with pytest.raises(TypeError, match='mesh_keep'):
        mesh.mesh_from_grid(dec, d, sigma, G, mesh_keep='largest')
    assert len(seen) == 2


# ---------------------------------------------------------------- the launcher: what validate() accepts and what it refuses, with the flag it names
LAUNCHER_OK = [
    "--export_mesh true --mesh_texture_size 256", "--export_mesh true --mesh_texture_size 4", "--export_mesh true --mesh_texture_size 8192",
    "--mesh_texture_size 0",
    "--export_mesh true --mesh_smooth_iters 10", "--export_mesh true --mesh_smooth_iters 1000", "--mesh_smooth_iters 0",
    "--export_mesh true --mesh_snap_iters 4", "--export_mesh true --mesh_snap_iters 64 --mesh_smooth_iters 10", "--mesh_snap_iters 0",
    "--export_mesh true --mesh_simplify_cell 2 --mesh_simplify_placement quadric", "--export_mesh true --mesh_simplify_cell 2 --mesh_simplify_placement mean",
    "--mesh_simplify_placement mean",
    "--export_mesh true --mesh_format ply", "--export_mesh true --mesh_format glb", "--export_mesh true --mesh_format obj", "--mesh_format obj",
    "--export_mesh true --mesh_format glb --mesh_texture_size 256", "--export_mesh true --mesh_format obj --mesh_texture_size 256",
    "--export_mesh true --mesh_format ply --export_mesh_normals true",
]
LAUNCHER_REFUSED = [
    ("--mesh_texture_size 256", 'export_mesh'),
    ("--export_mesh true --mesh_texture_size 3", 'mesh_texture_size'), ("--export_mesh true --mesh_texture_size 9000", 'mesh_texture_size'),
    ("--export_mesh true --mesh_texture_size -1", 'mesh_texture_size'),
    ("--mesh_smooth_iters 10", 'export_mesh'),
    ("--export_mesh true --mesh_smooth_iters 1001", 'mesh_smooth_iters'), ("--export_mesh true --mesh_smooth_iters -1", 'mesh_smooth_iters'),
    ("--mesh_snap_iters 4", 'export_mesh'),
    ("--export_mesh true --mesh_snap_iters 65", 'mesh_snap_iters'), ("--export_mesh true --mesh_snap_iters -1", 'mesh_snap_iters'),
    ("--mesh_simplify_cell 0 --mesh_simplify_placement quadric", 'export_mesh'),
    ("--export_mesh true --mesh_simplify_placement quadric", 'mesh_simplify_cell'),
    ("--export_mesh true --mesh_simplify_cell 0 --mesh_simplify_placement quadric", 'mesh_simplify_cell'),
    ("--export_mesh true --mesh_simplify_cell 2 --mesh_simplify_placement median", 'mesh_simplify_placement'),
    ("--mesh_format ply", 'export_mesh'), ("--mesh_format glb", 'export_mesh'),
    ("--export_mesh true --mesh_format stl", "mesh_format 'stl'.*obj.*ply.*glb"),
    ("--export_mesh true --mesh_format ply --mesh_texture_size 256", 'mesh_format ply.*mesh_texture_size'),
]


@pytest.mark.parametrize('objaverse', [True, False])
def test_launcher_flags(objaverse):
    from ln3diff_amd.entry import _MESH_FLAGS, create_argparser, validate
    parse = lambda s: create_argparser(objaverse).parse_args(s.split())                           # noqa: E731
    assert {flag: getattr(parse(""), flag) for flag in _MESH_FLAGS} == _MESH_FLAGS                 # unset: the record's defaults
    for ok in LAUNCHER_OK:
        validate(parse(ok))
    for flags, pattern in LAUNCHER_REFUSED:
        with pytest.raises(SystemExit, match=pattern):
            validate(parse(flags))
