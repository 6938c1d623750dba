"""MX-FP8 path of the T23D DiT without a GPU (include/ln3d_mx.h): every entry point rejects missing buffers before it touches the
device, the reference quantizer the GPU tests compare against is pinned on known cases, and --dit_precision is parsed and refused where
the path does not exist.

quantize_mx_ref() is THE reference quantizer of the format (OCP MX v1.0 MXFP8, the rule documented in include/ln3d_mx.h), written once
on torch's float8_e4m3fn / float8_e8m0fnu dtypes; tests/test_mxfp8_gpu.py imports it."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

N = None
I64 = C.c_int64


# ------------------------------------------------------------------------------------------------------------ reference quantizer
def quantize_mx_ref(x):
    """x [R, K] (any float dtype, K % 32 == 0) -> (q uint8 [R, K] e4m3fn bits, s uint8 [R, K / 32] E8M0 bits).
    e = floor(log2(amax)) - 8 clamped to [-127, 127] (all-zero block: -127); element = RNE(x / 2^e) saturated to +-448.
    Non-finite values: amax is taken over the finite elements of a block (none, or only zeros: e = -127), a NaN or +-Inf element is
    the E4M3 NaN code with its sign (0x7F / 0xFF), the finite elements of the block are quantized as if it were not there."""
    x = x.float()
    R, K = x.shape
    xb = x.reshape(R, K // 32, 32)
    fin = torch.isfinite(xb)
    xf = torch.where(fin, xb, torch.zeros_like(xb))
    amax = xf.abs().amax(-1)
    _, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1 (exact)
    e = torch.where(amax > 0, ex - 1 - 8, torch.full_like(ex, -127)).clamp(-127, 127)
    scale = torch.ldexp(torch.ones_like(amax), e.float())          # 2^e (2^-127 is an f32 subnormal: exact)
    s = (e + 127).to(torch.uint8)
    assert torch.equal(s.view(torch.float8_e8m0fnu).float(), scale)   # the byte IS the E8M0 encoding of the scale
    v = torch.ldexp(xf, -e.float()[..., None]).clamp(-448.0, 448.0)
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    nan_code = torch.where(torch.signbit(xb), torch.full_like(q, 0xFF), torch.full_like(q, 0x7F))
    return torch.where(fin, q, nan_code).reshape(R, K), s


def dequantize_mx(q, s):
    """(q, s) uint8 -> f32 [R, K]"""
    R, K = q.shape
    v = q.view(torch.float8_e4m3fn).float().reshape(R, K // 32, 32)
    sc = s.view(torch.float8_e8m0fnu).float() if s.min() > 0 else torch.ldexp(torch.ones(s.shape), s.float() - 127)
    return (v * sc[..., None]).reshape(R, K)


def e4m3_step(v):
    """spacing of e4m3 values at |v| (elementwise; subnormal spacing 2^-9 below 2^-6)"""
    _, ex = torch.frexp(v.abs().float())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float32), (ex - 1 - 3).clamp(min=-9).float())


def test_reference_quantizer_known_cases():
    # exact powers of two: amax 2^k -> e = k - 8, the element 2^8 = 256 (e4m3 0x78), 2^(j-8) for the others
    x = torch.zeros(1, 32)
    x[0, :6] = torch.tensor([4.0, 2.0, 1.0, 0.5, -0.25, 0.0])
    q, s = quantize_mx_ref(x)
    assert int(s[0, 0]) == 2 - 8 + 127
    assert q[0, :6].tolist() == [0x78, 0x70, 0x68, 0x60, 0xD8, 0x00]
    assert torch.equal(dequantize_mx(q, s), x)
    # saturation: 1.99 * 2^8 / 2^0 = 509 > 448 -> 448 (0x7E), never the NaN code 0x7F
    x = torch.full((1, 32), 1.0)
    x[0, 0] = 509.0
    x[0, 1] = -470.0
    q, s = quantize_mx_ref(x)
    assert int(s[0, 0]) == 127 and q[0, 0] == 0x7E and q[0, 1] == 0xFE and q[0, 2] == 0x38
    # all-zero block: the smallest scale (byte 0), zero elements
    q, s = quantize_mx_ref(torch.zeros(2, 64))
    assert int(s.max()) == 0 and int(q.max()) == 0
    # scale clamped at 2^-127: a block whose elements land in the e4m3 subnormal range (below 2^-6, steps of 2^-9)
    x = torch.zeros(1, 32)
    x[0, 0] = 2.0 ** -130                                      # floor(log2) - 8 = -138 -> clamped to -127: element 2^-3 (normal)
    x[0, 1] = 2.0 ** -136                                      # 2^-9 after scaling: the smallest subnormal (0x01)
    x[0, 2] = 3 * 2.0 ** -137                                  # 1.5 * 2^-9 -> ties to even: 2^-8 (0x02)
    x[0, 3] = 2.0 ** -138                                      # 0.5 * 2^-9 -> ties to even: 0
    q, s = quantize_mx_ref(x)
    assert int(s[0, 0]) == 0
    assert q[0, :4].tolist() == [0x20, 0x01, 0x02, 0x00]
    # a normal-range block with subnormal elements: amax 1 -> e = -8, element 2^-16 -> 2^-8 = 2 x 2^-9 (0x02)
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1] = 1.0, 2.0 ** -16
    q, s = quantize_mx_ref(x)
    assert int(s[0, 0]) == 119 and q[0, 1] == 0x02
    # round to nearest even in the normal range: 1 + 1/16 is halfway between 1 and 1.125 -> 1; 1 + 3/16 -> 1.25
    x = torch.zeros(1, 32)
    x[0, 0], x[0, 1], x[0, 2] = 256.0, 1.0625 * 2 ** -8 * 256, 1.1875 * 2 ** -8 * 256
    q, s = quantize_mx_ref(x)
    assert q[0, 1] == 0x38 and q[0, 2] == 0x3A
    # non-finite values (the rule of include/ln3d_mx.h).  A lone NaN / -Inf: its NaN code with the sign, no finite element -> byte 0
    x = torch.zeros(2, 32)
    x[0, 3], x[1, 31] = float('nan'), float('-inf')
    q, s = quantize_mx_ref(x)
    assert s.reshape(-1).tolist() == [0, 0] and q[0, 3] == 0x7F and q[1, 31] == 0xFF
    assert int(q[0].sum()) == 0x7F and int(q[1].sum()) == 0xFF             # the zeros around them stay zero
    x[0, 3] = -x[0, 3]                                                     # the sign of a NaN is kept
    assert quantize_mx_ref(x)[0][0, 3] == 0xFF
    # a block of NaN only next to an ordinary one: every element 0x7F, byte 0; the neighbour block is what it was
    x = torch.full((1, 64), float('nan'))
    x[0, 32:] = 1.0
    q, s = quantize_mx_ref(x)
    assert s[0].tolist() == [0, 119] and bool((q[0, :32] == 0x7F).all()) and bool((q[0, 32:] == 0x78).all())
    # Inf next to finite values: their codes and the scale are those of the block without the Inf
    x = torch.zeros(1, 32)
    x[0, :6] = torch.tensor([4.0, 2.0, 1.0, 0.5, -0.25, 0.0])
    q0, s0 = quantize_mx_ref(x)
    x[0, 5], x[0, 9], x[0, 10] = float('inf'), float('-inf'), float('nan')
    q, s = quantize_mx_ref(x)
    assert torch.equal(s, s0) and q[0, :5].tolist() == q0[0, :5].tolist() == [0x78, 0x70, 0x68, 0x60, 0xD8]
    assert q[0, 5] == 0x7F and q[0, 9] == 0xFF and q[0, 10] == 0x7F and int(q[0, 11:].max()) == 0 and int(q[0, 6:9].max()) == 0
    xb = x.bfloat16()                                                      # bf16 input: the same classes (the NaN written as bits:
    xb.view(torch.int16)[0, 10] = 0x7FC0                                   # torch's f32 -> bf16 cast of a NaN does not keep its sign)
    assert torch.equal(quantize_mx_ref(xb)[0], q)


# ------------------------------------------------------------------------------------------------------------ C ABI
def _norm_args_null():
    from ln3diff_amd import _lib
    return C.byref(_lib.NormArgs())                                 # x / y NULL


def _gemm_args_null():
    from ln3diff_amd import _lib
    return C.byref(_lib.MxGemmArgs())


NULL_CALLS = {
    'ln3d_quantize_mx': lambda: (N, 0, I64(32), 1, 32, N, I64(32), N, I64(1), N),
    'ln3d_gemm_mxfp8': lambda: (_gemm_args_null(), N),
    'ln3d_norm_modulate_mx': lambda: (_norm_args_null(), N, N),
}


def test_every_mx_entry_point_rejects_missing_buffers(hip_lib):
    hdr = open(os.path.join(ROOT, 'include', 'ln3d_mx.h')).read()
    declared = set(re.findall(r'^int (ln3d_[a-z0-9_]+)\(', hdr, re.M))
    assert declared == set(NULL_CALLS), declared ^ set(NULL_CALLS)
    for name, args in NULL_CALLS.items():
        assert getattr(hip_lib, name)(*args()) == -1, name                      # LN3D_ERR_BAD_ARG
    assert hip_lib.ln3d_gemm_mxfp8(N, N) == -1 and hip_lib.ln3d_norm_modulate_mx(N, N, N) == -1


def test_mx_shape_rules_are_validated(hip_lib):
    """K % 32 for the quantizer, K % 128 for the GEMM: refused up front (pointers are never dereferenced on the host)."""
    from ln3diff_amd import _lib
    fake = C.c_void_p(1 << 20)
    assert hip_lib.ln3d_quantize_mx(fake, 0, I64(48), 1, 48, fake, I64(48), fake, I64(2), N) == -1
    a = _lib.MxGemmArgs()
    a.Xq = a.Xs = a.Wq = a.Ws = a.out0 = fake
    a.M, a.N, a.K, a.ldx, a.ldw, a.ldxs, a.ldws, a.ldo, a.epilogue = 32, 32, 96, 96, 96, 4, 4, 32, 0
    assert hip_lib.ln3d_gemm_mxfp8(C.byref(a), N) == -1                         # K = 96
    a.K, a.ldx, a.ldw, a.epilogue = 128, 128, 128, 2
    assert hip_lib.ln3d_gemm_mxfp8(C.byref(a), N) == -1                         # GELU_ERF without out_scale
    a.out1 = a.out2 = fake
    a.M, a.N, a.epilogue, a.tokens, a.tok_pad, a.heads, a.head_dim, a.transpose_mask = 16, 192, 6, 8, 8, 8, 8, 0b100
    assert hip_lib.ln3d_gemm_mxfp8(C.byref(a), N) == -1                         # HEADS: a transposed output whose rows end inside a 16-token group


# ------------------------------------------------------------------------------------------------------------ --dit_precision
def _args(*flags):
    from ln3diff_amd.entry import create_argparser
    return create_argparser(True).parse_known_args(list(flags))[0]


def test_dit_precision_flag():
    from ln3diff_amd.entry import validate
    assert _args().dit_precision == 'bf16'
    for arch in ('DiT-B/2', 'DiT-L/2', 'DiT-XL/2'):
        assert validate(_args('--dit_model_arch', arch, '--dit_precision', 'mxfp8')) == 'edm'
    for flags, msg in [(('--dit_precision', 'fp8'), 'expected one of'),
                       (('--dit_precision', 'mxfp8', '--i23d', 'true', '--trainer_name', 'flow_matching'), 'I23D'),
                       (('--dit_precision', 'mxfp8', '--dit_model_arch', 'DiT-PixelArt-L/2', '--trainer_name', 'flow_matching'), 'PixArt'),
                       (('--dit_precision', 'mxfp8', '--create_dit', 'false', '--trainer_name', 'adm'), 'U-Net')]:
        with pytest.raises(SystemExit) as e:
            validate(_args(*flags))
        assert msg in str(e.value), (flags, str(e.value))


def test_set_matmul_precision_is_checked_on_cpu():
    from ln3diff_amd.dit.dit_trilatent import DiT_TriLatent
    from ln3diff_amd.dit.dit_models_xformers import TextCondDiTBlock
    m = DiT_TriLatent(input_size=8, patch_size=2, in_channels=4, hidden_size=128, depth=1, num_heads=2, num_classes=0, learn_sigma=False,
                      context_dim=768, roll_out=True, vit_blk=TextCondDiTBlock)
    assert m.matmul_precision == 'bf16'
    with pytest.raises(ValueError):
        m.set_matmul_precision('fp8')
    m._packed = {'sentinel': 1}
    assert m.set_matmul_precision('mxfp8').matmul_precision == 'mxfp8' and m._packed is None     # the pack is dropped
    m._packed = {'sentinel': 1}
    m.set_matmul_precision('mxfp8')
    assert m._packed == {'sentinel': 1}                                         # no change, no repack
