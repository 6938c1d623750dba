"""The ctypes binding against the headers, without a GPU.  ln3diff_amd/_lib.py declares every export once (PROTOTYPES: restype and
argtypes) and mirrors six argument structs by hand; nothing at run time reads include/.  Here the headers are parsed and
  - every `int | void | const char* ln3d_*(...)` of every header maps, by the one rule of _lib's docstring, to exactly its PROTOTYPES
    row, the rows of a header stand in its declaration order, and include/ has no subdirectory that this file would not read;
  - a C probe compiled with the build's compiler prints sizeof / offsetof of the six structs and the values of the header's constants,
    which must be the Structure classes' layouts and _lib's constants;
  - ops._p, the one place a tensor becomes an address, refuses a host tensor before the library is reached;
  - a value of the wrong kind is a ctypes.ArgumentError, not a call."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

HEADERS = sorted(glob.glob(os.path.join(ROOT, 'include', '*.h')))
STRUCTS = {'ln3d_gemm_args': 'GemmArgs', 'ln3d_gemm_mx_args': 'MxGemmArgs', 'ln3d_attn_args': 'AttnArgs', 'ln3d_norm_args': 'NormArgs',
           'ln3d_render_args': 'RenderArgs', 'ln3d_normals_args': 'NormalsArgs'}
SCALARS = {'int64_t': C.c_int64, 'int': C.c_int, 'float': C.c_float}
RESTYPES = {'int': C.c_int, 'void': None, 'const char*': C.c_char_p}


def _source(path):
    """a header without its comments"""
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S))


def _ctype(decl, lib):
    """one parameter or field declaration `type name` -> its ctypes type by the rule of _lib's docstring; anything else fails"""
    decl = ' '.join(decl.split())
    if '*' in decl:
        m = re.match(r'const (ln3d_\w+)\s?\*', decl)
        if m:
            assert m.group(1) in STRUCTS, f"pointer to an unknown ln3d type: {decl!r}"
            return C.POINTER(getattr(lib, STRUCTS[m.group(1)]))
        return C.c_void_p
    ctype = decl.rsplit(' ', 1)[0]
    assert ctype in SCALARS, f"parameter type outside the mapping rule: {decl!r}"
    return SCALARS[ctype]


def _declared_prototypes(lib, by_header=None):
    """{name: (restype, argtypes)} of every header; by_header, a dict, gets {header path: [its names in declaration order]}"""
    out = {}
    for path in HEADERS:
        names = [] if by_header is None else by_header.setdefault(path, [])
        for ret, name, params in re.findall(r'\b(int|void|const\s+char\s*\*)\s*(ln3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', _source(path)):
            assert name not in out, f"{name} declared twice"
            names.append(name)
            params = params.strip()
            out[name] = (RESTYPES[re.sub(r'\s*\*', '*', ' '.join(ret.split()))],
                         () if params == 'void' else tuple(_ctype(p, lib) for p in params.split(',')))
    return out


def _declared_structs():
    """{struct name: [(field, declaration it came from)]} of every `typedef struct [tag] { ... } name;`, fields in order"""
    out = {}
    for path in HEADERS:
        for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', _source(path)):
            fields = []
            for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
                first, *more = [d.strip() for d in decl.split(',')]                     # `int M, N, K`: one type, several fields
                assert not any('*' in d or ' ' in d for d in more), f"{name}: cannot read {decl!r}"
                base = first.rsplit(' ', 1)[0]
                fields += [(re.search(r'(\w+)$', d).group(1), d if d is first else base + ' ' + d) for d in [first] + more]
            out[name] = fields
    return out


def _constants():
    text = ''.join(_source(p) for p in HEADERS)
    return sorted(set(re.findall(r'\b(LN3D_EPI_\w+)\s*=', text)) | set(re.findall(r'#define\s+(LN3D_ERR_\w+|LN3D_RENDER_SCRATCH_FLOATS)\b', text)))


def test_prototype_table_equals_the_headers():
    from ln3diff_amd import _lib
    by_header = {}
    declared = _declared_prototypes(_lib, by_header)
    assert set(declared) == set(_lib.PROTOTYPES), set(declared) ^ set(_lib.PROTOTYPES)
    assert not [e.name for e in os.scandir(os.path.join(ROOT, 'include')) if e.is_dir()]      # one folder: HEADERS is every header
    for path, names in by_header.items():                                                  # row for row, in the order the header declares them
        assert [n for n in _lib.PROTOTYPES if n in set(names)] == names, path
    for name, (restype, argtypes) in declared.items():
        assert (_lib.PROTOTYPES[name][0], tuple(_lib.PROTOTYPES[name][1])) == (restype, argtypes), name
    assert list(_lib.SYMBOLS) == list(_lib.PROTOTYPES) and len(_lib.SYMBOLS) == 95
    assert {'ln3d_simplify_faces', 'ln3d_simplify_first', 'ln3d_simplify_keys', 'ln3d_simplify_mean', 'ln3d_simplify_used'} <= set(_lib.PROTOTYPES)


def test_lib_applies_the_table(hip_lib, monkeypatch):
    from ln3diff_amd import _lib
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert _lib.check_symbols() and hip_lib.ln3d_abi_version() == _lib.ABI_VERSION == 10
    assert hip_lib.ln3d_reload_env() is None
    assert isinstance(hip_lib.ln3d_strerror(-1), bytes)
    monkeypatch.setitem(_lib.PROTOTYPES, 'ln3d_no_such_entry_point', _lib._int())
    with pytest.raises(RuntimeError, match='ln3d_no_such_entry_point'):
        _lib.check_symbols()


def test_struct_layouts_and_constants_equal_the_compilers(tmp_path):
    from ln3diff_amd import _lib
    structs, consts = _declared_structs(), _constants()
    assert set(structs) == set(STRUCTS) and len(structs) == 6, set(structs) ^ set(STRUCTS)
    lines = ['#include <stdio.h>', '#include <stddef.h>'] + [f'#include "{os.path.basename(h)}"' for h in HEADERS] + ['int main(void) {']
    for s, fields in structs.items():
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        lines += [f'  printf("{s} {f} %zu\\n", offsetof({s}, {f}));' for f, _ in fields]
    lines += [f'  printf("const {c} %d\\n", (int)({c}));' for c in consts] + ['  return 0;', '}']
    (tmp_path / 'probe.c').write_text('\n'.join(lines) + '\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")                     # the compiler build() uses, on the host side only
    subprocess.check_call([hipcc, '-x', 'c', '-I', os.path.join(ROOT, 'include'), 'probe.c', '-o', 'probe'], cwd=tmp_path)
    rows = [ln.split() for ln in subprocess.check_output([str(tmp_path / 'probe')], text=True).splitlines()]
    measured = {(a, b): int(v) for a, b, v in rows}

    for s, fields in structs.items():
        cls = getattr(_lib, STRUCTS[s])
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], s                       # names, in order
        for (f, ctype), (_, decl) in zip(cls._fields_, fields):
            assert ctype is _ctype(decl, _lib), (s, decl)
            assert getattr(cls, f).offset == measured[s, f], (s, f, getattr(cls, f).offset, measured[s, f])
        assert C.sizeof(cls) == measured[s, 'sizeof'], s
    assert [measured[s, 'sizeof'] for s in ('ln3d_gemm_args', 'ln3d_gemm_mx_args', 'ln3d_attn_args', 'ln3d_norm_args', 'ln3d_render_args')] \
        == [192, 184, 88, 104, 264]

    epi = {c[len('LN3D_'):]: measured['const', c] for c in consts if c.startswith('LN3D_EPI_')}
    assert epi == {k: v for k, v in vars(_lib).items() if k.startswith('EPI_')} and len(epi) == 10
    assert measured['const', 'LN3D_RENDER_SCRATCH_FLOATS'] == _lib.RENDER_SCRATCH_FLOATS
    from test_abi_cpu import BAD_ARG, UNSUPPORTED                              # the codes the ABI tests expect, by value
    err = {c: measured['const', c] for c in consts if c.startswith('LN3D_ERR_')}
    assert err == {'LN3D_ERR_BAD_ARG': BAD_ARG, 'LN3D_ERR_LAUNCH': -2, 'LN3D_ERR_UNSUPPORTED': UNSUPPORTED}


class _NoLibrary:
    def __getattr__(self, name):
        def fail(*a):
            pytest.fail(f"{name} was reached with a host tensor")
        return fail


def test_host_tensors_never_reach_the_library(monkeypatch):
    """every wrapper turns tensors into addresses through ops._p, which refuses a host tensor: with small CPU tensors of the right
    dtypes and shapes each call below raises before the (fake) library is touched, so nothing can launch"""
    from ln3diff_amd import _lib, ops
    monkeypatch.setattr(_lib, 'lib', lambda: _NoLibrary())
    f = lambda *s: torch.zeros(*s)                                                               # noqa: E731
    h = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)                                         # noqa: E731
    i32, i64 = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    calls = [
        lambda: ops.cast_bf16(f(8), h(8)),
        lambda: ops.axpby(f(8), f(8), 1.0, 2.0),
        lambda: ops.tile_rows(f(4), f(8), 4, 2),
        lambda: ops.add_table_rows(f(1, 4), f(2, 4), f(2, 1, 4), 2, 1, 4),
        lambda: ops.timestep_embedding(f(1), h(1, 256), 1),
        lambda: ops.groupnorm_swish(f(1, 4, 32), f(32), f(32), h(1, 4, 32), f(8 * 2 * 2), 1, 4, 32, groups=8),
        lambda: ops.im2col3x3(h(1, 2, 2, 8), h(4, 128), 1, 2, 2, 8, 0, 128),
        lambda: ops.mesh_count(f(2, 2, 2), 2, 0.5, i32),
        lambda: ops.mcubes_emit(f(2, 2, 2), 2, 0.5, i64, f(9), i64),
        lambda: ops.ddim_step(f(8), f(8), f(8), f(8), 3.0, 1.0, 1.0, 1.0, 1.0, 0.0, False),
        lambda: ops.geglu(f(1, 128), h(1, 64), 1, 64),
        lambda: ops.planes_to_nchw(f(1, 3, 2, 2, 32), f(1, 96, 2, 2), 1, 32, 2, 2),
        # the two that had the check before their own validation keep it behind it
        lambda: ops.gemm(h(4, 64), h(8, 64), None, ops.EPI_F32, f(4, 8)),
        lambda: ops.attention(h(1, 1, 64, 64), h(1, 1, 64, 64), h(1, 1, 64, 64), h(1, 64, 64), 1, 1, 64, 64, 64, 64, 64),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="need device tensors"):
            call()
    with pytest.raises(RuntimeError, match="need device tensors"):
        ops.check_faces(torch.zeros(1, 3, dtype=torch.int64), 1)
    assert ops._p(None) is None


def test_wrong_kinds_of_argument_are_marshalling_errors(hip_lib):
    from ln3diff_amd._lib import GemmArgs
    with pytest.raises(C.ArgumentError):
        hip_lib.ln3d_cast_f32_bf16(1.5, None, 1, None)                          # a float for a pointer
    with pytest.raises(C.ArgumentError):
        hip_lib.ln3d_attention_bf16(C.byref(GemmArgs()), None)                  # another struct's arguments
    with pytest.raises(C.ArgumentError):
        hip_lib.ln3d_attention_bf16(GemmArgs(), None)                           # the same, passed as ops passes its structs
    with pytest.raises(C.ArgumentError):
        hip_lib.ln3d_timestep_embedding(None, None, "1", 256, None)             # a str for an int
    with pytest.raises(C.ArgumentError):
        hip_lib.ln3d_tile_rows(None, None, 4.0, 1, None)                        # a float for an int64_t
