"""Opt-in fp16 tri-plane texels (include/ln3d_planes16.h, Triplane.set_plane_precision('fp16')) without a GPU: the new entry points exist
and validate their arguments before they touch the device (fake, never dereferenced addresses, as tests/test_abi_cpu.py), the ABI
number is unchanged, the precision switch and the launchers' --plane_precision are checked on the CPU, and the ops refuse a texel type
that no kernel reads."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from test_abi_cpu import BAD_ARG, RENDER_ROWS, QUERY_OK, QUERY_ROWS, _render_args

N = None
P = C.c_void_p(0x10000)
I64, F = C.c_int64, C.c_float
NULL_CALLS = {
    'ln3d_planes_to_channel_last_f16': (N, N, 1, 32, 8, 8, N),
    'ln3d_planes_f32_to_f16': (N, N, I64(64), N),
    'ln3d_render_triplane_f16': (N, N),
    'ln3d_query_points_f16': (N, 8, 8, N, I64(1), N, N, N, N, F(0.9), N, N, N, N),
}


def test_the_header_s_entry_points_exist_and_reject_missing_buffers(hip_lib):
    from ln3diff_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ln3d_planes16.h')).read()
    declared = set(re.findall(r'^int (ln3d_[a-z0-9_]+)\(', hdr, re.M))
    assert declared == set(NULL_CALLS), declared ^ set(NULL_CALLS)
    assert _lib.check_symbols()
    for name, args in NULL_CALLS.items():
        assert getattr(hip_lib, name)(*args) == BAD_ARG, name
    assert hip_lib.ln3d_abi_version() == 10


def test_sizes_and_scales_are_validated_before_any_launch(hip_lib):
    """the rows tests/test_abi_cpu.py walks over ln3d_render_triplane and ln3d_query_points (the planes_ok cases among them: H, W <= 0,
    32-bit tap offsets, box_warp <= 0 or not finite), with the same codes"""
    for kw, code in RENDER_ROWS:
        assert hip_lib.ln3d_render_triplane_f16(C.byref(_render_args(**kw)), None) == code, (kw, code)
    for k in ('planes', 'plane_index', 'jitter', 'u_fine', 'rgb', 'depth', 'wsum', 'ray_limits', 'scalars', 'dec_w0', 'dec_b0', 'dec_w1', 'dec_b1'):
        assert hip_lib.ln3d_render_triplane_f16(C.byref(_render_args(**{k: None})), None) == BAD_ARG, k
    # 32-bit tap BYTE offsets inside one tri-plane: 3 * H * W * 32 * 2 bytes in binary16 - the first size past 2^31 - 1 is refused
    assert 3344 * 3345 > 0x7fffffff // (3 * 32 * 2) >= 3344 * 3344
    assert hip_lib.ln3d_render_triplane_f16(C.byref(_render_args(H=3344, W=3345)), None) == BAD_ARG
    for row in QUERY_ROWS + [{0: N}, {3: N}, {1: 3344, 2: 3345}]:
        a = list(QUERY_OK)
        for i, v in row.items():
            a[i] = v
        assert hip_lib.ln3d_query_points_f16(*a) == BAD_ARG, row
    ok = (P, P, 1, 32, 8, 8, N)
    for i, bad in [(0, N), (1, N), (2, 0), (2, -1), (3, 16), (3, 0), (4, 0), (4, -1), (5, 0), (5, -8), (2, 1 << 15)]:
        a = list(ok)
        a[i] = bad
        assert hip_lib.ln3d_planes_to_channel_last_f16(*a) == BAD_ARG, (i, bad)
    a = list(ok)
    a[4], a[5] = 1 << 16, 1 << 16                                       # H * W is an int
    assert hip_lib.ln3d_planes_to_channel_last_f16(*a) == BAD_ARG
    a[4], a[5] = 1, 0x7fffffff - 30                                     # so is H * W + 31, the grid's rounding
    assert hip_lib.ln3d_planes_to_channel_last_f16(*a) == BAD_ARG
    for a in [(N, P, I64(4), N), (P, N, I64(4), N), (P, P, I64(0), N), (P, P, I64(-1), N)]:
        assert hip_lib.ln3d_planes_f32_to_f16(*a) == BAD_ARG, a


def test_set_plane_precision_is_checked_on_cpu():
    from ln3diff_amd.nsr.triplane import Triplane
    tp = Triplane(img_resolution=16)
    assert tp.plane_precision == 'fp32'
    for bad in ('bf16', 'fp8', 'half', None):
        with pytest.raises(ValueError, match='expected one of'):
            tp.set_plane_precision(bad)
    assert tp.plane_precision == 'fp32'
    assert tp.set_plane_precision('fp16') is tp and tp.plane_precision == 'fp16'
    assert Triplane(img_resolution=16).plane_precision == 'fp32'               # per instance
    x32, x16 = torch.zeros(1, 3, 2, 2, 32), torch.zeros(1, 3, 2, 2, 32, dtype=torch.float16)
    assert tp.cast_planes(x16) is x16                                             # f16 planes pass under either setting
    assert tp.set_plane_precision('fp32').plane_precision == 'fp32'
    assert tp.cast_planes(x32) is x32 and tp.cast_planes(x16) is x16
    with pytest.raises(TypeError):
        Triplane.to_channel_last(torch.zeros(1, 96, 2, 2))                        # an instance method: the precision is the instance's


def _args(*flags, objaverse=True):
    from ln3diff_amd.entry import create_argparser
    return create_argparser(objaverse).parse_args(list(flags))


def test_plane_precision_flag():
    from ln3diff_amd.entry import validate
    for objaverse in (True, False):
        assert _args(objaverse=objaverse).plane_precision == 'fp32'
        assert _args('--plane_precision', 'fp16', objaverse=objaverse).plane_precision == 'fp16'
    assert validate(_args('--plane_precision', 'fp16')) == 'edm'
    assert validate(_args('--plane_precision', 'fp32')) == 'edm'
    assert validate(_args('--plane_precision', 'fp16', '--create_dit', 'true', '--roll_out', 'true', '--dit_model_arch', 'DiT-B/2', objaverse=False)) == 'gd'
    for bad in ('bf16', 'fp8'):
        with pytest.raises(SystemExit, match='expected one of'):
            validate(_args('--plane_precision', bad))


def test_ops_refuse_texel_types_no_kernel_reads(hip_lib):
    """the dispatch is on planes.dtype and happens before anything is launched: CPU tensors are enough"""
    from ln3diff_amd import ops
    z = torch.zeros(4)
    dec = (z, z, z, z)
    for dt in (torch.bfloat16, torch.float64, torch.int16):
        planes = torch.zeros(1, 3, 8, 8, 32, dtype=dt)
        with pytest.raises(TypeError, match='float32 or torch.float16'):
            ops.render_triplane(planes, 8, 8, z.int(), z, 4, dec, z, z, z, z, z, z, z)
        with pytest.raises(TypeError, match='float32 or torch.float16'):
            ops.query_points(planes[0], 8, 8, torch.zeros(4, 3), dec, 0.9, z, z, z)
    with pytest.raises(TypeError):
        ops.planes_to_channel_last_f16(torch.zeros(1, 96, 8, 8), torch.zeros(1, 3, 8, 8, 32), 1, 32, 8, 8)      # an f32 destination
    with pytest.raises(TypeError):
        ops.planes_f32_to_f16(torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.float16))
