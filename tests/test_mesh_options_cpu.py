"""The four mesh post-processing options - mesh_normals, mesh_keep, mesh_min_faces, mesh_simplify_cell - from every public entry of
ln3diff_amd.pipeline down to mesh.mesh_from_grid, without a GPU and without the library: the real pipeline code runs over a stub decoder
(CPU zero tensors) in a real AE, sampling is stubbed out, and mesh.mesh_from_grid is replaced by a recorder of the keywords it is given.
  - every entry delivers exactly normals / keep / min_faces / simplify_cell, with the values given or the defaults, once per sample;
  - a misspelt keyword is a TypeError at every entry, whether or not a mesh is exported;
  - without export_mesh a bad value is ignored and mesh_from_grid is not called;
  - the real mesh_from_grid hands the record's fields on to extract_isosurface and forward_points."""
import numpy as np
import pytest
import torch

B, V, G, R = 2, 3, 8, 4                      # samples, cameras, mesh grid, render resolution
DEFAULTS = dict(normals=False, keep='all', min_faces=0, simplify_cell=0.0)
ALL = dict(mesh_normals=True, mesh_keep='largest', mesh_min_faces=7, mesh_simplify_cell=2.5)        # pairwise distinct: a crossed wire shows
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
    common = dict(mesh_size=G, resolution=R)
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


@pytest.fixture
def recorder(monkeypatch):
    from ln3diff_amd import mesh
    calls = []

    def record(decoder, dec_out, sigma, grid_size, thr=10.0, **kw):
        assert grid_size == G and sigma.numel() == G ** 3
        calls.append(kw)
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint8)
    monkeypatch.setattr(mesh, 'mesh_from_grid', record)
    return calls


def test_the_entries_are_all_covered():
    assert list(_entries()) == ENTRIES


@pytest.mark.parametrize('entry', ENTRIES)
def test_options_reach_mesh_from_grid(recorder, entry):
    call, takes_normals = _entries()[entry]
    for given in OPTION_SETS:
        if not takes_normals:
            given = {k: v for k, v in given.items() if k != 'mesh_normals'}
        del recorder[:]
        out = call(True, **given)
        out = out[1] if isinstance(out, tuple) else out
        assert len(out['mesh']) == B and out['image_raw'].shape == (B, V, 3, R, R)
        want = dict(DEFAULTS, **{k[len('mesh_'):]: v for k, v in given.items()})
        assert [kw['sample_index'] for kw in recorder] == list(range(B)), (entry, given)
        for kw in recorder:
            assert {k: v for k, v in kw.items() if k not in ('sample_index', 'path')} == want, (entry, given, kw)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_misspelt_option_is_a_type_error(recorder, entry):
    call, _ = _entries()[entry]
    for export in (True, False):
        with pytest.raises(TypeError, match='mesh_kep'):
            call(export, mesh_kep='largest')
        assert recorder == []


@pytest.mark.parametrize('entry', ENTRIES)
def test_options_are_ignored_without_export(recorder, entry):
    call, _ = _entries()[entry]
    out = call(False, mesh_keep='bogus')
    out = out[1] if isinstance(out, tuple) else out
    assert 'mesh' not in out and recorder == []


def test_mesh_from_grid_hands_the_record_on(monkeypatch):
    from ln3diff_amd import mesh
    seen = []

    def isosurface(sigma, thr, method, *post):
        seen.append(post)
        return torch.tensor([[1.0, 2.0, 3.0]]), torch.zeros(0, 3, dtype=torch.int64)
    monkeypatch.setattr(mesh, 'extract_isosurface', isosurface)
    dec = _Decoder()
    out = mesh.mesh_from_grid(dec, dec.vit_decode_postprocess(None, None), torch.zeros(G ** 3), G, **mesh.MeshPost(True, 'largest', 7, 2.5)._asdict())
    assert seen == [('largest', 7, 2.5)] and dec.points == [True] and len(out) == 4
    out = mesh.mesh_from_grid(dec, dec.vit_decode_postprocess(None, None), torch.zeros(G ** 3), G, **mesh.MeshPost()._asdict())
    assert seen[1] == ('all', 0, 0.0) and dec.points == [True, False] and len(out) == 3
    assert mesh.MeshPost() == (False, 'all', 0, 0.0) and mesh.MeshPost._fields == ('normals', 'keep', 'min_faces', 'simplify_cell')
    assert mesh.MeshPost.from_kwargs(dict(mesh_min_faces=7)) == mesh.MeshPost(min_faces=7)
    for bad in ('min_faces', 'mesh_size', 'mesh_'):
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{bad}'"):
            mesh.MeshPost.from_kwargs({bad: 1})
