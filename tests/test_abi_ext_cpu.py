"""The additions to the C ABI declared under include/ext/ (mesh simplification, include/ext/ln3d_meshsimplify.h), without a GPU:
  - every prototype of include/ext/*.h maps, by the one rule of tests/test_abi_types_cpu.py, to exactly its row of _lib.EXT_PROTOTYPES, and
    lib() applies that table; the tables do not overlap and check_symbols() covers both;
  - every entry point returns LN3D_ERR_BAD_ARG for each null buffer, each zero, negative or oversize count and each bad cell / origin, and
    LN3D_ERR_UNSUPPORTED for nc = 2^21 + 1, all on fake addresses that are never dereferenced (validation precedes every launch);
  - a host tensor never reaches the library through the new ops wrappers."""
import glob
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_cpu import BAD_ARG, UNSUPPORTED
from test_abi_types_cpu import RESTYPES, _ctype, _source

EXT_HEADERS = sorted(glob.glob(os.path.join(ROOT, 'include', 'ext', '*.h')))
P = 0x10000                                  # a fake device address
BIG = 1 << 31                                # one more than the largest count
NAN, INF = float('nan'), float('inf')


def _declared(lib):
    out = {}
    for path in EXT_HEADERS:
        src = _source(path)
        assert 'struct' not in src, f"{path}: the additions use no struct"
        for ret, name, params in re.findall(r'\b(int|void|const\s+char\s*\*)\s*(ln3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', src):
            assert name not in out, f"{name} declared twice"
            params = params.strip()
            out[name] = (RESTYPES[re.sub(r'\s*\*', '*', ' '.join(ret.split()))],
                         () if params == 'void' else tuple(_ctype(p, lib) for p in params.split(',')))
    return out


def test_ext_table_equals_the_ext_headers():
    from ln3diff_amd import _lib
    declared = _declared(_lib)
    assert EXT_HEADERS and set(declared) == set(_lib.EXT_PROTOTYPES), set(declared) ^ set(_lib.EXT_PROTOTYPES)
    for name, (restype, argtypes) in declared.items():
        assert (_lib.EXT_PROTOTYPES[name][0], tuple(_lib.EXT_PROTOTYPES[name][1])) == (restype, argtypes), name
    assert not set(_lib.EXT_PROTOTYPES) & set(_lib.PROTOTYPES)
    assert sorted(_lib.EXT_PROTOTYPES) == ['ln3d_simplify_faces', 'ln3d_simplify_first', 'ln3d_simplify_keys', 'ln3d_simplify_mean',
                                           'ln3d_simplify_used']


def test_lib_applies_the_ext_table(hip_lib, monkeypatch):
    from ln3diff_amd import _lib
    for name, (restype, argtypes) in _lib.EXT_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert _lib.check_symbols()
    monkeypatch.setitem(_lib.EXT_PROTOTYPES, 'ln3d_no_such_entry_point', _lib._int())
    with pytest.raises(RuntimeError, match='ln3d_no_such_entry_point'):
        _lib.check_symbols()


# name -> (a valid argument list on fake addresses, indices of its buffers, indices of its counts)
VALID = {
    'ln3d_simplify_keys': ([P, 5, 0.0, -1.0, 2.0, 0.5, P, None], (0, 6), (1,)),
    'ln3d_simplify_mean': ([P, P, P, 9, 4, P, None], (0, 1, 2, 5), (3, 4)),
    'ln3d_simplify_faces': ([P, 7, P, 9, 4, P, P, None], (0, 2, 5, 6), (1, 3, 4)),
    'ln3d_simplify_first': ([P, P, 7, P, None], (0, 1, 3), (2,)),
    'ln3d_simplify_used': ([P, P, 7, 4, P, None], (0, 1, 4), (2, 3)),
}
NC_AT = {'ln3d_simplify_mean': 4, 'ln3d_simplify_faces': 4, 'ln3d_simplify_used': 3}          # where nc stands
NV_AT = {'ln3d_simplify_mean': 3, 'ln3d_simplify_faces': 3}                                   # nc <= nv is checked: raise nv with it


def _with(args, **at):
    a = list(args)
    for i, v in at.items():
        a[int(i[1:])] = v
    return a


def test_every_entry_point_validates_before_it_launches(hip_lib):
    from ln3diff_amd import _lib
    assert set(VALID) == set(_lib.EXT_PROTOTYPES)
    for name, (args, buffers, counts) in VALID.items():
        fn = getattr(hip_lib, name)
        for i in buffers:
            assert fn(*_with(args, **{'i%d' % i: None})) == BAD_ARG, (name, 'null buffer', i)
        for i in counts:
            for bad in (0, -1, BIG, 1 << 40):
                assert fn(*_with(args, **{'i%d' % i: bad})) == BAD_ARG, (name, 'count', i, bad)
    keys, kargs = hip_lib.ln3d_simplify_keys, VALID['ln3d_simplify_keys'][0]
    for cell in (0.0, -0.0, -1.0, NAN, INF, -INF):
        assert keys(*_with(kargs, i5=cell)) == BAD_ARG, cell
    for i in (2, 3, 4):
        for o in (NAN, INF, -INF):
            assert keys(*_with(kargs, **{'i%d' % i: o})) == BAD_ARG, (i, o)
    # more clusters than vertices cannot be
    assert hip_lib.ln3d_simplify_mean(*_with(VALID['ln3d_simplify_mean'][0], i3=4, i4=5)) == BAD_ARG
    assert hip_lib.ln3d_simplify_faces(*_with(VALID['ln3d_simplify_faces'][0], i3=4, i4=5)) == BAD_ARG
    # nc = 2^21 + 1: three cluster numbers no longer fit a face key; a null buffer still comes first
    for name, at in NC_AT.items():
        big = {'i%d' % at: (1 << 21) + 1}
        if name in NV_AT:
            big['i%d' % NV_AT[name]] = 1 << 22
        assert getattr(hip_lib, name)(*_with(VALID[name][0], **big)) == UNSUPPORTED, name
        assert getattr(hip_lib, name)(*_with(VALID[name][0], i0=None, **big)) == BAD_ARG, name
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG) and hip_lib.ln3d_strerror(UNSUPPORTED)


class _NoLibrary:
    def __getattr__(self, name):
        def fail(*a):
            pytest.fail(f"{name} was reached with a host tensor")
        return fail


@pytest.mark.parametrize('check', [True, False])
def test_host_tensors_never_reach_the_library(monkeypatch, check):
    """the new wrappers turn tensors into addresses through ops._p only (and their checks refuse a host tensor themselves): with small CPU
    tensors of the right dtypes, shapes and values each call raises before the (fake) library is touched"""
    from ln3diff_amd import _lib, ops
    monkeypatch.setattr(_lib, 'lib', lambda: _NoLibrary())
    v = torch.rand(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)                                          # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                                          # noqa: E731
    calls = [
        lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i64(4)),
        lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(2, 3), check=check),
        lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(2, 3), i64(2), check=check),
        lambda: ops.simplify_first(i64(2), torch.arange(2), i32(2), check=check),
        lambda: ops.simplify_used(faces, i32(2), i32(4), check=check),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="need device tensors"):
            call()
    with pytest.raises(RuntimeError, match="need device tensors"):
        ops.check_index(torch.arange(3), 3, "index")
    # the checks themselves: a value outside its range, a wrong dtype, a wrong shape - ValueError, wherever the tensor lives
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(4), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.tensor([-1, 0]), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(3, dtype=torch.int32), 3, "index")
    with pytest.raises(ValueError):
        ops.check_index(torch.arange(3), 3, "index", (4,))
    with pytest.raises(ValueError):
        ops.simplify_faces(faces, torch.tensor([0, 1, 2, 0]), 2, i64(2, 3), i64(2))             # cluster 2 of 2
    with pytest.raises(ValueError):
        ops.simplify_first(i64(2), torch.tensor([0, 2]), i32(2))                                 # perm 2 of 2
    with pytest.raises(ValueError):
        ops.simplify_used(faces, i32(2), i32(3))                                                 # corner 3 of 3 clusters
    with pytest.raises(ValueError):
        ops.simplify_mean(v, torch.tensor([0, 1, 2, 4]), torch.tensor([0, 2, 4]), torch.zeros(2, 3))      # order 4 of 4
    # a buffer that the kernel would write past its end - another dtype, too short, strided - is refused from its metadata, checked or not
    for bad in (lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i32(4)),
                lambda: ops.simplify_keys(v, (0.0, 0.0, 0.0), 1.0, i64(3)),
                lambda: ops.simplify_keys(v.double(), (0.0, 0.0, 0.0), 1.0, i64(4)),
                lambda: ops.simplify_keys(torch.rand(4, 6)[:, ::2], (0.0, 0.0, 0.0), 1.0, i64(4)),
                lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(1, 3), check=check),
                lambda: ops.simplify_mean(v, torch.arange(4), torch.tensor([0, 2, 4]), torch.zeros(2, 3, dtype=torch.float64), check=check),
                lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(1, 3), i64(2), check=check),
                lambda: ops.simplify_faces(faces, torch.tensor([0, 1, 1, 0]), 2, i64(2, 3), i32(2), check=check),
                lambda: ops.simplify_first(i64(2), torch.arange(2), i64(2), check=check),
                lambda: ops.simplify_first(i64(2), torch.arange(2), i32(1), check=check),
                lambda: ops.simplify_used(faces, i32(1), i32(4), check=check),
                lambda: ops.simplify_used(faces, i32(2), i64(4), check=check)):
        with pytest.raises(ValueError):
            bad()


def test_simplify_mesh_refuses_bad_arguments_before_any_launch(monkeypatch):
    from ln3diff_amd import _lib
    from ln3diff_amd.mesh import simplify_mesh, _simplify_cell
    monkeypatch.setattr(_lib, 'lib', lambda: _NoLibrary())
    v = torch.rand(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int64)
    for cell in (-1.0, NAN, INF, 1e-60, 'two'):
        with pytest.raises(ValueError):
            simplify_mesh(v, faces, cell)
    for cell in (None, 0, 0.0):
        a, b = simplify_mesh(v, faces, cell)
        assert a is v and b is faces and _simplify_cell(cell) == 0.0
    with pytest.raises(ValueError):
        simplify_mesh(v.double(), faces, 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v.reshape(3, 4), faces, 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v, faces.int(), 1.0)
    with pytest.raises(ValueError):
        simplify_mesh(v, faces + 2, 1.0)                                                         # index 5 of 4 vertices
    for origin in ((0.0, 0.0), (0.0, NAN, 0.0), (INF, 0.0, 0.0)):
        with pytest.raises(ValueError):
            simplify_mesh(v, faces, 1.0, origin)
