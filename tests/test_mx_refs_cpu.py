"""The float64 helpers of tests/mx_refs.py are right and can fail: the E4M3 table decodes like torch's float8_e4m3fn, the rounding
oracle agrees with the reference quantizer and knows its ties, exact operands decode to what they claim, the exactness condition refuses
what it must, and the output checker rejects a wrong scale and a wrong element.  No GPU needed."""
import pytest
import torch

import mx_refs as mr
from test_mxfp8_cpu import dequantize_mx, quantize_mx_ref


def test_e4m3_table_is_torchs_decode():
    t = mr.e4m3_table()
    dec = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    ok = torch.ones(256, dtype=torch.bool)
    ok[list(mr.NAN_CODES)] = False
    assert int(ok.sum()) == 254 and torch.equal(t[ok], dec[ok])
    assert bool(torch.isnan(t[~ok]).all()) and bool(torch.isnan(dec[~ok]).all())
    assert float(t[0x7E]) == 448.0 and float(t[0x01]) == 2.0 ** -9 and float(t[0x08]) == 2.0 ** -6 and float(t[0x38]) == 1.0
    assert bool((t[1:0x7F] > t[0:0x7E]).all())                           # ascending with the code: "even code" = even mantissa


def test_rne_expected_known_ties_and_saturation():
    v = torch.tensor([1.0625, 1.1875, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, 448.0, 464.0, 1e9, -1e9, 0.0, -0.0, 2.0 ** -11])
    assert mr.e4m3_rne_expected(v).tolist() == [0x38, 0x3A, 0xB8, 0x00, 0x02, 0x7E, 0x7E, 0x7E, 0xFE, 0x00, 0x80, 0x00]
    up = torch.nextafter(torch.tensor([1.0625, 2.0 ** -10]), torch.tensor(9.0))
    assert mr.e4m3_rne_expected(up).tolist() == [0x39, 0x01]
    with pytest.raises(AssertionError):
        mr.e4m3_rne_expected(torch.tensor([float("nan")]))


def test_rne_expected_agrees_with_the_reference_quantizer():
    """on random finite data (every magnitude from e4m3 subnormals to saturation) and on every probe, with the block's scale pinned"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 32 * 31, generator=g) * torch.exp2(torch.randint(-14, 9, (64, 32 * 31), generator=g).float())
    p = mr.e4m3_probes()
    probes = torch.cat([p, -p])
    assert probes.numel() == 2 * (127 + 3 * 126 + 4)
    for vals in (x.reshape(-1).clamp(-500, 500), probes):
        n = (vals.numel() + 30) // 31
        pad = torch.zeros(n * 31)
        pad[:vals.numel()] = vals
        blk = torch.cat([torch.full((n, 1), 448.0), pad.reshape(n, 31)], 1)      # e = 0: the element IS RNE(x)
        assert int((blk != 0).sum()) >= vals.numel() - 2
        q, s = quantize_mx_ref(blk)
        assert bool((s == 127).all())
        assert torch.equal(q, mr.e4m3_rne_expected(blk))


def test_probes_cover_every_code_and_both_sides_of_every_tie():
    p = mr.e4m3_probes()
    codes = mr.e4m3_rne_expected(p)
    assert sorted(set(codes.tolist())) == list(range(0x7F))
    assert bool((p[1:] >= p[:-1]).all()) and float(p[-1]) < 512.0 and float(p[-1]) > 511.9
    t = mr.e4m3_table()
    exact = t[codes.long()] == p.double()
    assert int(exact.sum()) == 127                                          # the code values; everything else rounds


def test_exact_operand_and_the_exactness_condition():
    g = torch.Generator().manual_seed(1)
    q, s, d = mr.mx_exact_operand(5, 256, g, vmax=8, emin=-2, emax=2)
    assert q.dtype == s.dtype == torch.uint8 and d.dtype == torch.float64 and s.shape == (5, 8)
    assert torch.equal(dequantize_mx(q, s).double(), d)                     # torch's decode agrees with the table
    assert int(s.min()) >= 125 and int(s.max()) <= 129 and float((d / torch.exp2(s.double() - 127).repeat_interleave(32, 1)).abs().max()) <= 8
    assert len(set(s.reshape(-1).tolist())) > 1 and len(set(q.reshape(-1).tolist())) > 8
    mr.assert_fp32_exact(896, 8, -2, 2)                                     # the largest K at these ranges
    with pytest.raises(AssertionError):
        mr.assert_fp32_exact(1024, 8, -2, 2)
    mr.assert_fp32_exact(4096, 8, -1, 0)                                    # a smaller range buys a longer K
    with pytest.raises(AssertionError):
        mr.assert_fp32_exact(384, 8, -2, 2, bias=64, gate_exp=1, res=500)   # a gate of 2^+-1 costs a factor of 4
    mr.assert_fp32_exact(384, 8, -1, 1, bias=64, gate_exp=2, res=500)
    with pytest.raises(AssertionError):
        mr.assert_fp32_exact(128, 17, 0, 0)
    # the condition is the right one: at its edge a sum of K vmax^2 2^(2 emax) on a grid of 2^(2 emin) still fits 24 bits, one step on not
    bound, grid = mr.assert_fp32_exact(896, 8, -2, 2)
    top = torch.tensor(bound - grid, dtype=torch.float64)
    assert float(top.float().double()) == float(top) and float((top * 2 + grid).float().double()) != float(top * 2 + grid)


def test_check_mx_output_accepts_the_quantizer_and_rejects_errors():
    g = torch.Generator().manual_seed(2)
    v = torch.randn(16, 128, generator=g, dtype=torch.float64) * 3
    q, s = quantize_mx_ref(v.float())
    assert mr.check_mx_output(q, s, v, 'norm', 1e-6) == (0, 0)
    bad = s.clone()
    bad[3, 1] += 1
    with pytest.raises(AssertionError):
        mr.check_mx_output(q, bad, v, 'norm', 1e-6)                         # a scale off by one, amax nowhere near a power of two
    bad = q.clone()
    bad[5, 7] = (bad[5, 7] & 0x80) | ((bad[5, 7] & 0x7F) + 2 if (bad[5, 7] & 0x7F) < 0x70 else (bad[5, 7] & 0x7F) - 2)
    with pytest.raises(AssertionError):
        mr.check_mx_output(bad, s, v, 'norm', 1e-6)                         # an element two codes off
    assert abs(float(mr.gelu64(torch.tensor(1.0, dtype=torch.float64))) - 0.8413447460685429) < 1e-15
