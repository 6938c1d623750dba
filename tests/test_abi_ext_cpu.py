"""The additions to the C ABI declared under include/ext/ (texture baking, include/ext/ln3d_meshbake.h), without a GPU:
  - every prototype of include/ext/*.h maps, by the one rule of tests/test_abi_types_cpu.py, to exactly its row of _lib.EXT_PROTOTYPES, and
    lib() applies that table; the tables do not overlap, PROTOTYPES keeps its 80 rows and check_symbols() covers both;
  - the additions use no struct and no new LN3D_ERR_* / LN3D_EPI_* constant;
  - both entry points return LN3D_ERR_BAD_ARG for each null buffer, each zero, negative or oversize count and each bad (T, n, c, nf)
    combination, all on fake addresses that are never dereferenced (validation precedes every launch)."""
import glob
import os
import re

import pytest

from conftest import ROOT
from test_abi_cpu import BAD_ARG
from test_abi_types_cpu import RESTYPES, _ctype, _source

EXT_HEADERS = sorted(glob.glob(os.path.join(ROOT, 'include', 'ext', '*.h')))
P = 0x10000                                  # a fake device address
BIG = 1 << 31                                # one more than the largest count


def _declared(lib):
    out = {}
    for path in EXT_HEADERS:
        src = _source(path)
        assert 'struct' not in src, f"{path}: the additions use no struct"
        assert not re.search(r'LN3D_(ERR|EPI)_\w+\s*=|#define\s+LN3D_(ERR|EPI)_', src), f"{path}: the additions define no constant"
        for ret, name, params in re.findall(r'\b(int|void|const\s+char\s*\*)\s*(ln3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', src):
            assert name not in out, f"{name} declared twice"
            params = params.strip()
            out[name] = (RESTYPES[re.sub(r'\s*\*', '*', ' '.join(ret.split()))],
                         () if params == 'void' else tuple(_ctype(p, lib) for p in params.split(',')))
    return out


def test_ext_table_equals_the_ext_headers():
    from ln3diff_amd import _lib
    declared = _declared(_lib)
    assert EXT_HEADERS and list(declared) == list(_lib.EXT_PROTOTYPES), set(declared) ^ set(_lib.EXT_PROTOTYPES)          # row for row
    for name, (restype, argtypes) in declared.items():
        assert (_lib.EXT_PROTOTYPES[name][0], tuple(_lib.EXT_PROTOTYPES[name][1])) == (restype, argtypes), name
    assert not set(_lib.EXT_PROTOTYPES) & set(_lib.PROTOTYPES) and len(_lib.PROTOTYPES) == len(_lib.SYMBOLS) == 80 and _lib.ABI_VERSION == 10
    assert list(_lib.EXT_PROTOTYPES) == ['ln3d_bake_points', 'ln3d_bake_pack']


def test_lib_applies_the_ext_table(hip_lib, monkeypatch):
    from ln3diff_amd import _lib
    for name, (restype, argtypes) in _lib.EXT_PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert _lib.check_symbols()
    monkeypatch.setitem(_lib.EXT_PROTOTYPES, 'ln3d_no_such_entry_point', _lib._int())
    with pytest.raises(RuntimeError, match='ln3d_no_such_entry_point'):
        _lib.check_symbols()


# name -> (a valid argument list on fake addresses, indices of its buffers, indices of its int64 counts)
VALID = {
    'ln3d_bake_points': ([P, 9, P, 7, 11, 2, 5, P, P, None], (0, 2, 7, 8), (1, 3)),             # verts nv faces nf T n c points owner stream
    'ln3d_bake_pack': ([P, P, 121, 0, P, None], (0, 1, 4), (2,)),                               # rgb owner P fill tex stream
}


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
    points, pargs = hip_lib.ln3d_bake_points, VALID['ln3d_bake_points'][0]
    # (T, n, c, nf): T outside [4, 8192]; n < 1; c < 4; n * c > T; nf > 2 n^2 - each with the other values as sane as they can be
    for T, n, c, nf in ((3, 1, 3, 1), (3, 1, 4, 1), (0, 1, 4, 1), (-8, 1, 4, 1), (8193, 1, 4, 1), (16384, 2048, 4, 2), (1 << 30, 1, 4, 1),
                        (11, 0, 5, 1), (11, -2, 5, 1), (11, 2, 3, 7), (11, 2, 0, 7), (11, 2, -5, 7), (11, 2, 6, 7), (11, 3, 4, 7),
                        (8192, 1 << 16, 1 << 16, 7),                                     # n * c overflows an int
                        (11, 2, 5, 9), (4, 1, 4, 3), (64, 1, 64, 3), (8192, 2048, 4, 2 * 2048 * 2048 + 1)):
        assert points(*_with(pargs, i3=nf, i4=T, i5=n, i6=c)) == BAD_ARG, (T, n, c, nf)
    pack, kargs = hip_lib.ln3d_bake_pack, VALID['ln3d_bake_pack'][0]
    for fill in (-1, 256, 1 << 20):
        assert pack(*_with(kargs, i3=fill)) == BAD_ARG, fill
    assert pack(*_with(kargs, i2=8192 * 8192 + 1)) == BAD_ARG
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG)
