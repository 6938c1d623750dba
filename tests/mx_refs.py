"""Float64 helpers for the MX-FP8 kernels of include/ln3d_mx.h (tests/test_mx_refs_cpu.py pins each of them without a GPU):

  e4m3_table / e4m3_rne_expected   the E4M3 code space from its bit fields and round-to-nearest-even onto it, written without torch's
                                   float8 cast: the independent oracle of the quantizer (quantize_mx_ref of tests/test_mxfp8_cpu.py is
                                   written ON that cast);
  mx_exact_operand / assert_fp32_exact
                                   MXFP8 operands of small integers and power-of-two block scales, and the condition under which every
                                   partial sum of their product is exact in fp32, so that a GEMM result is determined bit for bit
                                   whatever the summation order;
  check_mx_output / gelu64         an MXFP8 output against the reference quantizer applied to the float64 values it approximates.

The float64 norm (kr.norm_modulate), bf16 rounding (kr.bf16_rne), head-split map (kr.heads_split_ref) and the erf polynomial's documented
error (kr.GELU_ERF_ABS) are those of tests/kernel_refs.py."""
import torch

import kernel_refs as kr
from test_mxfp8_cpu import dequantize_mx, e4m3_step, quantize_mx_ref

E4M3_MAX = 448.0
NAN_CODES = (0x7F, 0xFF)


# ---------------------------------------------------------------- the E4M3 code space
def e4m3_table():
    """The 256 values of OCP FP8 E4M3 (float64), from the bit fields: sign s, exponent E (4 bits, bias 7), mantissa m (3 bits);
    E = 0: (-1)^s m 2^-9; otherwise (-1)^s (8 + m) 2^(E - 10); E = 15, m = 7 (0x7F / 0xFF) is NaN, there are no infinities."""
    c = torch.arange(256)
    s, E, m = c >> 7, (c >> 3) & 15, (c & 7).double()
    mag = torch.where(E == 0, m * 2.0 ** -9, (8.0 + m) * torch.exp2(E.double() - 10.0))
    v = torch.where(s == 1, -mag, mag)
    v[0x7F] = v[0xFF] = float("nan")
    return v


def e4m3_rne_expected(v):
    """v (finite, any shape) -> uint8 E4M3 codes: the nearest code value, a tie to the code with an even mantissa (= the even code),
    |v| >= 448 to +-448 (0x7E / 0xFE, never the NaN code), the sign of v kept on a zero result."""
    v = v.double()
    assert bool(torch.isfinite(v).all())
    pos = e4m3_table()[:0x7F]                                        # 0 .. 448, ascending with the code
    a = v.abs().clamp(max=E4M3_MAX)
    hi = torch.searchsorted(pos, a.reshape(-1).contiguous()).reshape(a.shape).clamp(max=0x7E)      # first code with pos >= a
    lo = (hi - 1).clamp(min=0)
    d_lo, d_hi = a - pos[lo], pos[hi] - a                            # exact where it decides: a has 24 bits, the codes 4, in one binade
    even = torch.where(lo % 2 == 0, lo, hi)
    code = torch.where(d_hi < d_lo, hi, torch.where(d_lo < d_hi, lo, even))
    return (code | (torch.signbit(v).long() << 7)).to(torch.uint8)


def e4m3_probes():
    """Every point at which rounding to E4M3 can go wrong, as f32 magnitudes (ascending): the 127 non-negative code values, the 126
    midpoints between neighbours and the f32 values next to each midpoint on both sides, and values beyond 448 (below 512, so that a
    block led by 448 keeps its scale): the next f32, the would-be midpoint 464, the would-be code 480, the last f32 below 512."""
    pos = e4m3_table()[:0x7F].float()
    mid = (pos[:-1] + pos[1:]) / 2                                   # exact: 5 significant bits
    inf = torch.tensor(float("inf"))
    beyond = torch.tensor([448.0, 464.0, 480.0, 512.0])
    p = torch.cat([pos, mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), torch.nextafter(beyond[:1], inf), beyond[1:3],
                   torch.nextafter(beyond[3:], -inf)])
    return p.sort().values


# ---------------------------------------------------------------- exact GEMM operands
def assert_fp32_exact(K, vmax, emin, emax, bias=0, gate_exp=0, res=0):
    """Refuses a case unless every partial sum of sum_k x_k w_k is exact in fp32 in ANY order: the products are multiples of
    g = 2^(2 emin) and every partial sum is at most S = K vmax^2 2^(2 emax), so all are exact when S / g < 2^24.  With an epilogue
    res + gate * (sum + bias), integer |bias| <= bias and |res| <= res (multiples of g: emin <= 0) and gate = +-2^j, |j| <= gate_exp:
    every intermediate is a multiple of g 2^-gate_exp and at most (S + bias) 2^gate_exp + res.  -> (bound, grid)"""
    assert vmax <= 16, "integers above 16 are not all E4M3 values"
    assert emin <= 0 or (bias == 0 and res == 0)
    bound = (K * vmax * vmax * 2.0 ** (2 * emax) + bias) * 2.0 ** gate_exp + res
    g = 2.0 ** (2 * emin - gate_exp)
    assert bound / g < 2.0 ** 24, f"K {K}, |v| <= {vmax}, scales 2^{emin}..2^{emax}: sums up to {bound:g} on a grid of {g:g} are not exact in fp32"
    return bound, g


def mx_exact_operand(R, K, gen, vmax=8, emin=-2, emax=2):
    """-> (q uint8 [R, K], s uint8 [R, K / 32], deq float64 [R, K]): integer elements in [-vmax, vmax] (exact in E4M3 up to 16), one
    power-of-two scale 2^emin .. 2^emax per 32-block.  The codes come from e4m3_rne_expected, not from torch's cast."""
    assert K % 32 == 0 and vmax <= 16
    v = torch.randint(-vmax, vmax + 1, (R, K), generator=gen).double()
    e = torch.randint(emin, emax + 1, (R, K // 32), generator=gen)
    q = e4m3_rne_expected(v)
    assert torch.equal(e4m3_table()[q.long()], v)
    return q, (e + 127).to(torch.uint8), v * torch.exp2(e.double()).repeat_interleave(32, 1)


# ---------------------------------------------------------------- MXFP8 outputs against the reference quantizer
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2 ** 0.5))


def check_mx_output(q, s, v64, what, near_rel):
    """an MXFP8 output against the reference quantizer applied to the fp64 values it approximates: scales equal except blocks whose
    amax lies within `near_rel` (relative) of a power of two, where the kernel's own value may fall on the other side; elements of the
    other blocks within one e4m3 step of the reference quantizer's (+ the documented 1.3e-4 absolute error of the erf-GELU polynomial,
    common.h gelu_erf2, for the GELU epilogue).  Saturation at 448 is part of the format: both sides saturate alike."""
    q, s = q.cpu(), s.cpu()
    q_ref, s_ref = quantize_mx_ref(v64.float())
    R, K = v64.shape
    amax = v64.abs().reshape(R, K // 32, 32).amax(-1)
    m, _ = torch.frexp(amax)
    near = ((m - 0.5).abs() / 0.5 < near_rel) | ((1.0 - m).abs() < near_rel)
    diff = s != s_ref
    print(what, 'blocks', diff.numel(), 'scale differs', int(diff.sum()), 'of which near a power of two', int((diff & near).sum()))
    assert int((diff & ~near).sum()) == 0, (what, int((diff & ~near).sum()))
    got, ref = dequantize_mx(q, s).double(), dequantize_mx(q_ref, s_ref).double()
    same = (~diff).repeat_interleave(32, 1)
    sc = torch.ldexp(torch.ones(R, K // 32, dtype=torch.float64), s.double() - 127).repeat_interleave(32, 1)
    tol = e4m3_step((torch.maximum(got.abs(), ref.abs()) / sc).float()).double() * sc + (kr.GELU_ERF_ABS if what == 'gelu' else 0.0)
    err = torch.where(same, (got - ref).abs(), torch.zeros_like(got))
    print(what, 'elements off the reference quantizer by > 0 / > 1 step:', int(((err > 0) & same).sum()), int((err > tol).sum()))
    assert bool((err <= tol).all()), (what, float((err - tol).max()))
    return int(diff.sum()), int((diff & near).sum())
