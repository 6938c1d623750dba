"""The mesh smoothing of include/ln3d_meshsmooth.h without a GPU:
  - the numpy reference (tests/mesh_smooth_refs.py) against what the definition promises - which vertices are pinned, that pinned vertices
    keep their bits, that Taubin's passes keep the volume where Laplacian smoothing loses it, that the roughness falls - and seeded faults
    that the equalities of tests/test_mesh_smooth_gpu.py must catch;
  - every entry point validates on fake addresses before it launches (the prototype table against the header: tests/test_abi_types_cpu.py);
  - smooth_mesh between the extraction and the query; the ValueErrors of smooth_mesh and of the ops wrappers.
(mesh_smooth_iters from every public entry of pipeline down, and the launcher flag: tests/test_mesh_options_cpu.py.)"""
import math

import numpy as np
import pytest
import torch

import mesh_smooth_refs as R
from abi_args import BAD_ARG, refuses_null_buffers_and_bad_counts, with_args as _with

P, Q = 0x10000, 0x4000000                    # two fake device addresses, 64 MiB apart


# ---------------------------------------------------------------- the reference's own properties
def test_open_patch_pins_exactly_its_rim():
    xyz, faces, rim = R.patch(6)
    start, nbr, pinned = R.adjacency(faces, len(xyz))
    assert len(faces) == 50 and len(rim) == 20 and np.array_equal(np.nonzero(pinned)[0], rim)
    v0 = (xyz * 30).astype(np.float32)
    v5 = R.smooth(v0, faces, 5)
    moved = (R.bits(v5) != R.bits(v0)).any(1)
    assert not moved[rim].any() and moved[np.setdiff1d(np.arange(36), rim)].all()


def test_closed_meshes_pin_nothing():
    for nv, faces in ((4, R.TETRA_F), (258, R.sphere(3)[1])):
        start, nbr, pinned = R.adjacency(faces, nv)
        assert not pinned.any() and (np.diff(start) >= 3).all()
    v, f = R.sphere(3)
    assert v.shape == (258, 3) and f.shape == (512, 3) and abs(R.volume(v, f) - 4 / 3 * math.pi) < 0.1


def test_adjacency_of_the_hand_made_meshes():
    c = R.cases()
    deg = lambda name: np.diff(R.adjacency(c[name][1], len(c[name][0]))[0])               # noqa: E731
    pin = lambda name: np.nonzero(R.adjacency(c[name][1], len(c[name][0]))[2])[0].tolist()   # noqa: E731
    assert deg('tetra').tolist() == [3] * 4 and pin('tetra') == []
    assert np.array_equal(deg('duplicate_faces'), deg('opposite_windings')) and pin('duplicate_faces') == pin('opposite_windings') == []
    assert pin('two_sided_patch') == [] and np.array_equal(deg('two_sided_patch'), deg('patch6'))        # a second naming unpins, adds no neighbour
    assert deg('three_faces_one_edge').tolist() == [4, 4, 3, 3, 2] and pin('three_faces_one_edge') == [0, 1, 4]
    s, n, p = R.adjacency(c['face_a_a_b'][1], 20)
    assert n[s[18]:s[19]].tolist() == [19] and n[s[19]:s[20]].tolist() == [18] and not p.any()           # (18, 18, 19): one interior edge
    assert 7 in n[s[3]:s[4]] and np.diff(s)[5] == np.diff(R.adjacency(R.sphere(1)[1], 18)[0])[5]          # (5, 5, 5) adds nothing
    assert deg('unreferenced_vertex').tolist() == [3, 3, 0, 3, 3, 0, 0]
    assert deg('fan600')[0] == 600 and set(deg('fan600')[1:]) == {3} and pin('fan600') == list(range(1, 601))
    assert deg('fan600_two_hubs')[[0, 601]].tolist() == [600, 600] and set(deg('fan600_two_hubs')[1:601]) == {4} and pin('fan600_two_hubs') == []
    for name, (v, f) in c.items():                                                        # the two routes to the keys agree
        keys = R.edge_keys(f)
        uniq, cnt = np.unique(keys[keys >= 0], return_counts=True)
        assert {(int(k) >> 32, int(k) & 0xffffffff): int(m) for k, m in zip(uniq, cnt)} == dict(R.edge_count(f)), name
        s, n, _ = R.adjacency(f, len(v))
        assert all((np.diff(n[s[i]:s[i + 1]]) > 0).all() for i in range(len(v))), name    # distinct and ascending


def test_taubin_keeps_the_volume_and_laplacian_does_not():
    """measured with this reference: volume ratio 1.0171 after 10 Taubin iterations at the defaults, 0.4168 after 20 Laplacian passes; mean
    squared umbrella residual 0.002986 -> 0.000985 (root mean square 0.0546 -> 0.0314)"""
    v, f = R.noisy_sphere()
    taubin, laplace = R.smooth(v, f, 10), R.smooth(v, f, 20, R.LAM, 0.0)
    ratio_t, ratio_l = R.volume(taubin, f) / R.volume(v, f), R.volume(laplace, f) / R.volume(v, f)
    before, after = R.roughness(v, f), R.roughness(taubin, f)
    print('[smooth] volume ratio: taubin %.4f laplacian %.4f; roughness %.6f -> %.6f' % (ratio_t, ratio_l, before, after))
    assert 0.97 <= ratio_t <= 1.03 and ratio_l < 0.5
    assert after < before


def test_every_seeded_fault_changes_bits():
    """a fused multiply-add in the last step, float64 accumulation, descending neighbours, neighbours counted once per naming and an in-place
    update are each told from the definition by the equalities of the GPU tests, on the meshes those tests use"""
    c = R.cases()
    for variant in R.VARIANTS:
        hit = [name for name, (v, f) in c.items() if not np.array_equal(R.bits(R.smooth(v, f, 2, variant=variant)), R.bits(R.expected(name, R.LAM, R.MU)[2]))]
        assert {'sphere258', 'fan600_two_hubs', 'patch6'} <= set(hit), (variant, hit)
    v, f = c['duplicate_faces']                                                           # the doubled edges are where 'duplicates' differs in kind
    assert not np.array_equal(np.diff(R.adjacency(f, 18, multiplicity=True)[0]), 2 * np.diff(R.adjacency(f, 18)[0]))
    a, b = R.expected('sphere258', R.LAM, R.MU)[7], R.expected('sphere258', 1.0, -1.0)[7]
    assert not np.array_equal(R.bits(a), R.bits(b)) and np.isfinite(a).all() and np.isfinite(b).all()


# ---------------------------------------------------------------- entry points on fake addresses
# name -> (a valid argument list on fake addresses, indices of its buffers, indices of its int64 counts)
VALID = {
    'ln3d_smooth_edge_keys': ([P, 7, Q, None], (0, 2), (1,)),                                                # faces nf key stream
    'ln3d_smooth_halfedges': ([P, P + 4096, 9, 5, Q, Q + 4096, None], (0, 1, 4, 5), (2, 3)),                 # edge count ne nv dkey pinned stream
    'ln3d_smooth_step': ([P, P + 4096, P + 8192, P + 12288, 5, 18, 0.5, Q, None], (0, 1, 2, 3, 7), (4, 5)),  # in start nbr pinned nv nh factor out stream
}


def test_every_smooth_entry_point_validates_before_it_launches(hip_lib):
    for name, (args, buffers, counts) in VALID.items():
        refuses_null_buffers_and_bad_counts(getattr(hip_lib, name), name, args, buffers, counts)
    step, sargs = hip_lib.ln3d_smooth_step, VALID['ln3d_smooth_step'][0]
    for factor in (float('nan'), float('inf'), -float('inf')):
        assert step(*_with(sargs, i6=factor)) == BAD_ARG, factor
    assert step(*_with(sargs, i7=P)) == BAD_ARG                                            # in and out are one buffer
    for shift in (4, 12 * 5 - 4, -(12 * 5 - 4)):                                           # ... or overlap: nv = 5 rows of 12 bytes
        assert step(*_with(sargs, i7=P + shift)) == BAD_ARG, shift
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG)


class _Field:
    """a decoder that records when it is asked for colours"""
    def __init__(self, log):
        self.log = log

    def forward_points(self, pcl, pts, with_grad=False):
        self.log.append(('forward_points', pts[0].clone()))
        return {'rgb': torch.zeros_like(pts), 'normal': torch.zeros_like(pts)}


def test_smoothing_sits_between_the_extraction_and_the_query(monkeypatch):
    from ln3diff_amd import mesh
    log = []
    G = 8
    raw, smoothed = torch.tensor([[1.0, 2.0, 3.0]]), torch.tensor([[7.0, 0.0, 3.5]])
    faces = torch.zeros(0, 3, dtype=torch.int64)

    def isosurface(sigma, thr, method, *post):
        log.append(('extract_isosurface', post))
        return raw, faces

    def smooth(verts, f, iterations, lam, mu, check=True):
        log.append(('smooth_mesh', verts, f, iterations, lam, mu, check))
        return smoothed, f
    monkeypatch.setattr(mesh, 'extract_isosurface', isosurface)
    monkeypatch.setattr(mesh, 'smooth_mesh', smooth)
    d = {'planes_channel_last': torch.zeros(1, 3, 4, 4, 2)}
    v = mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, smooth_iters=3, smooth_mu=-0.25, simplify_cell=2.0)[0]
    assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'forward_points']
    assert log[0][1] == ('all', 0, 2.0)                                                   # the extraction is called exactly as before
    assert log[1][1] is raw and log[1][2] is faces and log[1][3:] == (3, 0.5, -0.25, False)
    box = (smoothed / (G - 1) * 2 - 1) * 0.45                                             # the query and the result see the SMOOTHED position
    assert torch.equal(log[2][1], box) and np.array_equal(v, (mesh.rotation_matrix_x(-90) @ box.numpy().T).T.astype(np.float32))
    del log[:]
    out = mesh.textured_mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, texture_size=8, smooth_iters=2)
    assert [e[0] for e in log] == ['extract_isosurface', 'smooth_mesh', 'forward_points'] and log[1][3:] == (2, 0.5, -0.53, False) and len(out) == 5
    for bad in (dict(smooth_iters=1001), dict(smooth_iters=1, smooth_lambda=0.0), dict(smooth_iters=1, smooth_mu=0.1)):
        del log[:]
        with pytest.raises(ValueError, match='smooth_'):
            mesh.mesh_from_grid(_Field(log), d, torch.zeros(G ** 3), G, **bad)
        assert log == []                                                                  # refused before anything is extracted


def test_the_default_call_launches_nothing_new(monkeypatch):
    from ln3diff_amd import _lib, mesh

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    v, f = torch.rand(5, 3), torch.tensor([[0, 1, 2]])
    for off in (0, None, 0.0):
        a, b = mesh.smooth_mesh(v, f, off)
        assert a is v and b is f
    a, b = mesh.smooth_mesh(v[:0], f[:0], 3, check=False)                                 # an empty mesh returns empty
    assert a.shape == (0, 3) and b.shape == (0, 3)


def test_smooth_mesh_refuses_bad_arguments(monkeypatch):
    from ln3diff_amd import _lib, mesh, ops

    class NoLibrary:
        def __getattr__(self, name):
            def fail(*a):
                pytest.fail(f"{name} was reached")
            return fail
    monkeypatch.setattr(_lib, 'lib', lambda: NoLibrary())
    v = torch.rand(4, 3)
    f = torch.tensor(R.TETRA_F, dtype=torch.int64)
    nan, inf = v.clone(), v.clone()
    nan[2, 1], inf[0, 0] = float('nan'), float('-inf')
    for bad in (lambda: mesh.smooth_mesh(v.double(), f, 1), lambda: mesh.smooth_mesh(v.reshape(-1), f, 1), lambda: mesh.smooth_mesh(v, f.int(), 1),
                lambda: mesh.smooth_mesh(v, f.int(), 1, check=False), lambda: mesh.smooth_mesh(v, f.reshape(-1), 1, check=False),
                lambda: mesh.smooth_mesh(v, f + 1, 1), lambda: mesh.smooth_mesh(v, f - 1, 1), lambda: mesh.smooth_mesh(v[:3], f, 1),
                lambda: mesh.smooth_mesh(nan, f, 1, check=False), lambda: mesh.smooth_mesh(inf, f, 1, check=False),
                lambda: mesh.smooth_mesh(v, f, -1), lambda: mesh.smooth_mesh(v, f, 1001), lambda: mesh.smooth_mesh(v, f, 2.5),
                lambda: mesh.smooth_mesh(v, f, True), lambda: mesh.smooth_mesh(v, f, 'many'), lambda: mesh.smooth_mesh(v, f, float('nan')),
                lambda: mesh.smooth_mesh(v, f, 1, lam=0.0), lambda: mesh.smooth_mesh(v, f, 1, lam=-0.5), lambda: mesh.smooth_mesh(v, f, 1, lam=1.5),
                lambda: mesh.smooth_mesh(v, f, 1, lam=float('nan')), lambda: mesh.smooth_mesh(v, f, 1, lam=1e-60), lambda: mesh.smooth_mesh(v, f, 1, lam='x'),
                lambda: mesh.smooth_mesh(v, f, 1, mu=0.01), lambda: mesh.smooth_mesh(v, f, 1, mu=-1.01), lambda: mesh.smooth_mesh(v, f, 1, mu=float('nan')),
                lambda: mesh.smooth_mesh(v, f, 1, mu=-float('inf')), lambda: mesh.mesh_adjacency(f + 1, 4), lambda: mesh.mesh_adjacency(f.int(), 4)):
        with pytest.raises(ValueError):
            bad()
    assert mesh._smooth_args(7, 1.0, -1.0) == (7, 1.0, -1.0) and mesh._smooth_args(None) == (0, 0.5, float(np.float32(-0.53)))
    assert mesh._smooth_args(np.int64(3), 0.25, 0)[::2] == (3, 0.0)
    # the wrappers: a host tensor never reaches the library, a buffer of the wrong dtype, length or stride neither
    key, dkey = torch.zeros(12, dtype=torch.int64), torch.zeros(12, dtype=torch.int64)
    edge, count, pinned = torch.zeros(6, dtype=torch.int64), torch.ones(6, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    start, nbr, out = torch.arange(0, 13, 3), torch.zeros(12, dtype=torch.int32), torch.zeros(4, 3)
    for check in (True, False):
        for call in (lambda: ops.smooth_edge_keys(f, 4, key, check=check), lambda: ops.smooth_halfedges(edge, count, 4, dkey, pinned, check=check),
                     lambda: ops.smooth_step(v, start, nbr, pinned, 0.5, out, check=check)):
            with pytest.raises(RuntimeError, match="need device tensors"):
                call()
    with pytest.raises(RuntimeError, match="need device tensors"):
        mesh.smooth_mesh(v, f, 1)
    with pytest.raises(RuntimeError, match="need device tensors"):
        mesh.mesh_adjacency(f, 4)
    for bad in (lambda: ops.smooth_edge_keys(f.int(), 4, key), lambda: ops.smooth_edge_keys(f, 4, key[:11]), lambda: ops.smooth_edge_keys(f, 4, key.int()),
                lambda: ops.smooth_edge_keys(f, 3, key), lambda: ops.smooth_edge_keys(f, 4, torch.zeros(24, dtype=torch.int64)[::2]),
                lambda: ops.smooth_halfedges(edge, count.int(), 4, dkey, pinned), lambda: ops.smooth_halfedges(edge, count, 4, dkey[:11], pinned),
                lambda: ops.smooth_halfedges(edge, count, 5, dkey, pinned), lambda: ops.smooth_halfedges(edge, count, 4, dkey, pinned.long()),
                lambda: ops.smooth_halfedges(edge + 4, count, 4, dkey, pinned), lambda: ops.smooth_halfedges(edge + (4 << 32), count, 4, dkey, pinned),
                lambda: ops.smooth_step(v.double(), start, nbr, pinned, 0.5, out), lambda: ops.smooth_step(v, start[:-1], nbr, pinned, 0.5, out),
                lambda: ops.smooth_step(v, start, nbr.long(), pinned, 0.5, out), lambda: ops.smooth_step(v, start, nbr, pinned[:3], 0.5, out),
                lambda: ops.smooth_step(v, start, nbr, pinned, 0.5, out[:3]), lambda: ops.smooth_step(v, start, nbr, pinned, 0.5, torch.zeros(4, 6)[:, ::2]),
                lambda: ops.smooth_step(v, start, nbr + 4, pinned, 0.5, out), lambda: ops.smooth_step(v, start, nbr - 1, pinned, 0.5, out),
                lambda: ops.smooth_step(v, start + 1, nbr, pinned, 0.5, out), lambda: ops.smooth_step(v, start.flip(0), nbr, pinned, 0.5, out),
                lambda: ops.smooth_step(v, torch.tensor([0, 3, 2, 9, 12]), nbr, pinned, 0.5, out)):
        with pytest.raises(ValueError):
            bad()
