"""Mesh clean-up without a GPU: the numpy reference of tests/mesh_clean_refs.py against scipy and against hand-built expectations and the
recorded figures of the test fields, the C ABI of include/ln3d_meshclean.h (the entry points exist and refuse every missing buffer and bad
size before anything touches the device), the Python argument checks and the launcher's up-front refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_refs as M
from conftest import ROOT

ENTRY_POINTS = ('ln3d_mesh_components', 'ln3d_mesh_component_counts', 'ln3d_mesh_mark', 'ln3d_mesh_gather')


def _all_graphs():
    for name, make in M.GRAPHS.items():
        f, nv = make()
        for seed in M.RENUMBERINGS:
            yield '%s/%s' % (name, seed), M.renumber(f, nv, seed), nv
    for field, method in M.FIELDS:
        pos, f = M.welded(field, method)
        yield '%s/%s' % (field, method), f, len(pos)


def test_reference_agrees_with_scipy():
    pytest.importorskip('scipy')
    n = 0
    for name, f, nv in _all_graphs():
        assert np.array_equal(M.labels(f, nv), M.scipy_labels(f, nv)), name
        n += 1
    assert n == 4 * len(M.GRAPHS) + len(M.FIELDS)


def test_reference_on_hand_built_graphs():
    f, nv = M.strip()
    assert (M.labels(f, nv) == 0).all()
    f, nv = M.interleaved_strips(500, 1000)
    want = np.arange(nv)
    want[:1506] %= 3
    lab = M.labels(f, nv)
    assert np.array_equal(lab, want)
    nvert, nface, best = M.counts(f, lab)
    assert nvert[:3].tolist() == [502] * 3 and nface[:3].tolist() == [500] * 3 and (nvert[3:1506] == 0).all() and (nvert[1506:] == 1).all()
    assert (nface[3:] == 0).all() and best == (500 << 32) | 0x7fffffff            # three-way tie -> root 0
    f, nv = M.fan()
    assert (M.labels(f, nv) == 0).all() and M.counts(f, M.labels(f, nv))[1][0] == 2048
    f, nv = M.two_tetrahedra()
    assert (M.labels(f, nv) == 0).all()                                           # one shared vertex joins the two surfaces
    f, nv = M.single_face()
    lab = M.labels(f, nv)
    assert lab.tolist() == [0, 1, 2, 1, 1, 5]
    nvert, nface, best = M.counts(f, lab)
    assert nvert.tolist() == [1, 3, 1, 0, 0, 1] and nface.tolist() == [0, 1, 0, 0, 0, 0] and best == (1 << 32) | (0x7fffffff - 1)
    f, nv = M.random_triples()
    assert (f[0, 0] == f[0, 1]) and (f[2] == f[2, 0]).all()                        # faces that repeat an index are in the set
    lab = M.labels(f, nv)
    assert (lab[f] == lab[f[:, :1]]).all() and (lab <= np.arange(nv)).all() and (lab[lab] == lab).all()
    # a renumbering permutes the components and nothing else
    for seed in (1, 2, 3):
        g = M.renumber(f, nv, seed)
        assert sorted(np.bincount(M.labels(g, nv), minlength=nv).tolist()) == sorted(np.bincount(lab, minlength=nv).tolist())


@pytest.mark.parametrize('field,method', list(M.FIELDS))
def test_reference_meets_the_recorded_figures(field, method):
    pos, f = M.welded(field, method)
    M.check_figures(field, method, f, len(pos))


@pytest.mark.parametrize('method,big,speck', [('cubes', 248, 8), ('tetra', 768, 24)])
def test_reference_clean_on_the_blob_field(method, big, speck):
    """the two specks have 8 faces each under marching cubes (min_faces = 9 removes them) and 24 under marching tetrahedra (25 does)"""
    pos, f = M.welded('blob', method)
    v1, f1 = M.clean(pos, f, 'largest')
    lab = M.labels(f, len(pos))
    root = M.FIELDS['blob', method]['roots'][1]
    assert len(f1) == big and len(v1) == int((lab == root).sum())
    assert np.array_equal(v1[f1], pos[f[lab[f[:, 0]] == root]])
    for m in (9, speck, speck + 1):
        v2, f2 = M.clean(pos, f, 'all', m)
        assert len(f2) == len(f) - (2 * speck if m > speck else 0)
        assert np.array_equal(v2[f2], pos[f[M.counts(f, lab)[1][lab[f[:, 0]]] >= m]])
    v3, f3 = M.clean(pos, f, 'all', 10 ** 6)
    assert v3.shape == (0, 3) and f3.shape == (0, 3)
    v4, f4 = M.clean(pos, f)
    assert np.array_equal(v4, pos) and np.array_equal(f4, f)


# ---------------------------------------------------------------- C ABI
def test_header_declares_the_entry_points_and_the_library_has_them(hip_lib):
    src = open(os.path.join(ROOT, 'include', 'ln3d_meshclean.h')).read()
    assert tuple(re.findall(r'^int (ln3d_\w+)\(', src, re.M)) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(hip_lib, name), name
    from ln3diff_amd import _lib
    assert _lib.check_symbols() is True
    assert hip_lib.ln3d_abi_version() == 10
    assert 'ln3d_mesh_components' not in open(os.path.join(ROOT, 'include', 'ln3d.h')).read()


P_ = C.c_void_p(0x10000)          # fake, never dereferenced: validation comes before any launch
I64 = C.c_int64
BIG = I64(1 << 31)
# name -> (a valid argument list, the positions of its buffers, {position: bad value} rows); the stream is the last argument
ABI = {
    'ln3d_mesh_components': ((P_, I64(4), I64(8), P_, None), (0, 3),
                             [{1: I64(0)}, {1: I64(-1)}, {1: BIG}, {2: I64(0)}, {2: I64(-5)}, {2: BIG}]),
    'ln3d_mesh_component_counts': ((P_, I64(4), P_, I64(8), P_, P_, P_, None), (0, 2, 4, 5, 6),
                                   [{1: I64(0)}, {1: I64(-1)}, {1: BIG}, {3: I64(0)}, {3: I64(-5)}, {3: BIG}]),
    'ln3d_mesh_mark': ((P_, I64(4), P_, P_, I64(8), I64(0), 0, P_, P_, P_, None), (0, 2, 3, 7, 8, 9),
                       [{1: I64(0)}, {1: I64(-1)}, {1: BIG}, {4: I64(0)}, {4: I64(-5)}, {4: BIG}, {5: I64(-1)}, {5: I64(-(1 << 40))}]),
    'ln3d_mesh_gather': ((P_, P_, P_, P_, P_, P_, I64(8), I64(4), P_, P_, None), (0, 1, 2, 3, 4, 5, 8, 9),
                         [{6: I64(0)}, {6: I64(-5)}, {6: BIG}, {7: I64(0)}, {7: I64(-1)}, {7: BIG}]),
}


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_points_refuse_bad_arguments_before_the_device(hip_lib, name):
    """every missing buffer, nv < 1, nv > 2^31 - 1, nf < 1 (and nf > 2^31 - 1: the counts are int32) and a negative min_faces: -1"""
    ok, buffers, rows = ABI[name]
    fn = getattr(hip_lib, name)
    for i in buffers:
        a = list(ok)
        a[i] = None
        assert fn(*a) == -1, (name, 'null buffer', i)
    for row in rows:
        a = list(ok)
        for i, v in row.items():
            a[i] = v
        assert fn(*a) == -1, (name, {i: v.value for i, v in row.items()})


# ---------------------------------------------------------------- Python argument checks
def test_python_wrappers_refuse_bad_arguments():
    from ln3diff_amd import mesh, ops
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    for kw in (dict(keep='biggest'), dict(min_faces=-1), dict(min_faces=1.5)):
        with pytest.raises(ValueError):
            mesh.clean_mesh(v, f, **kw)
        with pytest.raises(ValueError):
            mesh.extract_isosurface(torch.zeros(3, 3, 3), **kw)
    a, b = mesh.clean_mesh(v, f)                                       # the default launches nothing and hands its arguments back
    assert a is v and b is f
    for bad in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):            # an out-of-range index never reaches a kernel
        for call in (lambda: ops.check_faces(bad, 4), lambda: mesh.clean_mesh(v, bad, 'largest'), lambda: mesh.mesh_components(bad, 4),
                     lambda: ops.mesh_components(bad, 4, None)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        ops.check_faces(f.int(), 4)
    with pytest.raises(ValueError):
        ops.check_faces(f.reshape(-1), 4)
    for vv, ff in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.long)), (v, torch.zeros(0, 3, dtype=torch.long))):   # empty in, empty out
        a, b = mesh.clean_mesh(vv, ff, 'largest')
        assert tuple(a.shape) == (0, 3) and tuple(b.shape) == (0, 3) and b.dtype == torch.int64 and a.dtype == torch.float32


def test_launcher_refuses_the_flags_without_export_mesh():
    from ln3diff_amd.entry import create_argparser, validate
    parse = lambda *flags: create_argparser(True).parse_known_args(list(flags))[0]
    for flags in (('--mesh_keep', 'largest'), ('--mesh_min_faces', '50'), ('--mesh_keep', 'largest', '--mesh_min_faces', '50', '--export_mesh', 'false')):
        with pytest.raises(SystemExit) as e:
            validate(parse(*flags))
        assert '--export_mesh true' in str(e.value)
    for flags in (('--mesh_keep', 'biggest', '--export_mesh', 'true'), ('--mesh_min_faces', '-1', '--export_mesh', 'true')):
        with pytest.raises(SystemExit):
            validate(parse(*flags))
    a = parse('--mesh_keep', 'largest', '--mesh_min_faces', '50', '--export_mesh', 'true')
    assert validate(a) == 'edm' and a.mesh_keep == 'largest' and a.mesh_min_faces == 50
    d = parse()
    assert validate(d) == 'edm' and d.mesh_keep == 'all' and d.mesh_min_faces == 0
