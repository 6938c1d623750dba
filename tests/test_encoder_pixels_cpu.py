"""The per-pixel, per-stage criterion of tests/encoder_pixel_refs.py checked without a GPU: the health of its yardstick for every
(case, stage) test_encoder_pixels_gpu.py runs, the launches every case states against ln3diff_amd.convstack and csrc/kernel_plan.h,
the oracle's self-consistency (forward IS the chained run_stage), and that the criterion REJECTS the wiring defects of a multi-view
encoder - the ones the whole-tensor rel-L2 < 1.5e-2 gate of tests/test_encoder_gpu.py is printed beside.

Measured (worst rho; whole-tensor rel-L2 of the defective stage against y16, and whether the old 1.5e-2 gate would have seen it):
    attn1 per frame instead of joint (rel64)                 rho 35     rel-L2 4.7e-2  seen
    frames of two objects interleaved (rel64)                rho 13     rel-L2 1.9e-2  seen, barely
    Downsample padded (1,0,1,0)                              rho 840 / 970     rel-L2 1.4     seen
    Downsample from the odd origin                           rho 710 / 1060    rel-L2 1.4     seen
    one frame of twelve from the odd origin (down0_ds)       rho 910    rel-L2 4.0e-1  seen; found in that frame and in no other
    padded input channels of conv_in alias real channels     rho 700 / 1490    rel-L2 0.8 / 1.8   seen
    attn2's projection swapped with attn1's (dh48-rect)      rho 260    rel-L2 2.8e-1  seen
    the last frame dropped from the joint keys               rho 6.5    rel-L2 9.8e-3  NOT seen
    the last frame dropped, one object of two                rho 6.5    rel-L2 7.3e-3  NOT seen
    scale Dp ** -0.5 for dh ** -0.5, heads 48 -> 64          rho 3.6    rel-L2 3.5e-3  NOT seen
    scale Dp ** -0.5 for dh ** -0.5, heads 16 -> 64          rho 12     rel-L2 1.1e-2  NOT seen
    GroupNorm eps 1e-5 for 1e-6                              rho 0.6 .. 1.3   rel-L2 6e-4 .. 1e-3   NOT seen, and by the criterion at
                                                             CAP = 1.0 not reliably either: recorded as such, not rejected
The figures are asserted as inequalities below and printed by every test."""
import pytest
import torch
import torch.nn.functional as F

import encoder_pixel_refs as R
from conftest import rel_l2
from ln3diff_amd import convstack
from ln3diff_amd.dit.dit_models_xformers import attn_out_dim
from oracle import decoder as odec
from oracle import dit as odit
from oracle import encoder as oenc
from oracle import unet as ounet

CAP = 1.0              # the GPU test's caps are at or below this; a defect rejected at 1.0 is rejected at any tighter cap
OLD_GATE = 1.5e-2      # tests/test_encoder_gpu.py: every stage rel-L2 < 1.5e-2 against the reference goldens


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("cid", [i for i in R.CASE_IDS if not R.CASES[i]['raises']])
def test_yardstick_of_every_stage_of_every_case(cid):
    """measured: medians 1.3e-3 .. 3.7e-3, worst pixel 6.1e-3 - no case needed another scale or seed"""
    for name in R.stage_names(cid):
        _, y64, y16 = R.stage_pair(cid, name)
        med, mx = R.pixel_yardstick(y16, y64)
        print(f'{cid} {name}: d / |y64| per pixel: median {med:.2e} max {mx:.2e}')
        assert R.YARD_MEDIAN[0] <= med <= R.YARD_MEDIAN[1] and mx <= R.YARD_MAX, (cid, name, med, mx)


# ------------------------------------------------------------------------------------------------ the stated launches
def _product_route(dh, L):
    """ConvStack.self_attend's own condition: the MFMA kernels, or 'small'"""
    return 'mfma' if convstack.mfma_head(dh) and L >= convstack.MFMA_MIN_TOKENS and L % 32 == 0 else 'small'


def test_every_case_states_the_launch_the_product_and_the_plan_give(tmp_path):
    assert ounet.MFMA_MIN_TOKENS == convstack.MFMA_MIN_TOKENS
    cpu = torch.device('cpu')
    for c in R.CASES.values():
        cfg = R.case_cfg(c['id'])
        dh, heads, Fr = cfg['d_head'], cfg['n_heads'], cfg['num_frames']
        shapes = dict((n, (H, W)) for n, H, W in R.stage_shapes(c['id']))
        # ---- the attention: token counts from the walk, the route from ConvStack.self_attend's condition and the oracle's assumption
        if 'mid_attn_1' in shapes:
            H, W = shapes['mid_attn_1']
            assert c['attn1'][0] == Fr * H * W and c['attn2'][0] == H * W, c['id']
            for L, route in (c['attn1'], c['attn2']):
                assert ounet.attn_route(dh, L) == route, (c['id'], dh, L, route)
                assert (route == 'small') == (_product_route(dh, L) == 'small'), (c['id'], dh, L)
            if c['raises']:                                     # too many tokens for ln3d_attention_small at a head size the MFMA route refuses
                assert not convstack.mfma_head(dh) and c['attn1'][0] > 1024
            for (L, route), seqs in ((c['attn1'], c['objects']), (c['attn2'], c['N'])):
                assert route == 'small' or seqs * heads < R.CUS, c['id']          # never a head for every CU
        else:
            assert c['attn1'] is None and c['attn2'] is None, c['id']
        # ---- the shortcuts and the padded projections of the product's own packing
        m = R.build_enc(c['cfg'])
        if c['stage'] is None:
            skips = {}
            for b in [b for d in m.down for b in d.block] + [m.mid.block_1, m.mid.block_2]:
                if hasattr(b, 'nin_shortcut'):
                    q = convstack.pack_resblock(b.norm1, b.conv1, b.norm2, b.conv2, cpu, shortcut=b.nin_shortcut)
                    skips[b.in_channels] = 'centre' if 'kpad' in q['skip'] else 'gemm'
            assert skips == c['skips'], (c['id'], skips)
            assert m.steps() == oenc.stages(cfg)
        if 'mid_attn_1' in shapes:
            blk = m.mid.attn_1.transformer_blocks[0]
            plain, padded = convstack.pack_out_proj(blk.attn1.to_out[0].weight, blk.attn1.to_out[0].bias, heads, dh, cpu)
            if not convstack.mfma_head(dh):
                assert padded is None and c['attn1'][1] == c['attn2'][1] == 'small'
            else:                                               # a copy of its own exactly where the heads are stored wider than they are
                assert (padded is not plain) == (attn_out_dim(dh) != dh) and padded['cin'] == heads * attn_out_dim(dh)
        # ---- the GEMMs: stated to leave the 128x128 register-staged tile, or not
        ring = any(rows >= R.GEMM_RING_ROWS and n >= 128 for rows, n in R.gemms(c['id']))
        assert ring == c['ring_gemm'], (c['id'], R.gemms(c['id']))
        cin_pad = (cfg['in_channels'] + 7) // 8 * 8
        assert convstack.pack_conv3(m.conv_in, cpu, cin_pad=cin_pad)['cin'] == cin_pad
    # ---- every stated attention launch and the widest GEMM beside it against the plan of csrc/kernel_plan.h
    launches = R.enc_launches()
    planned = R.plan([ln for _, _, ln in launches], tmp_path)
    for (who, route, ln), (kernel, ring) in zip(launches, planned):
        if route != 'small':
            assert ln[3] < R.CUS and kernel != 'kres' and R.ROUTE_OF_KERNEL[kernel] == route, (who, ln, kernel, route)
        assert ring == R.CASES[who.split('/')[0]]['ring_gemm'], (who, ln)
    # ---- the cases reach what they are there for
    a1 = {c['attn1'][1] for c in R.CASES.values() if c['attn1'] and not c['raises']}
    a2 = {c['attn2'][1] for c in R.CASES.values() if c['attn2'] and not c['raises']}
    assert a1 == set(R.ROUTES) and a2 == {'small', 'stream'}
    assert any(c['attn1'][1] != c['attn2'][1] for c in R.CASES.values() if c['attn1'])      # one block, two attention kernels
    wide = {R.case_cfg(c['id'])['d_head'] for c in R.CASES.values() if c['attn1'] and c['attn1'][1] != 'small'}
    assert {d for d in wide if attn_out_dim(d) != d} == {16, 48} and {64, 80, 128} <= wide  # padded copies and plain projections
    assert {v for c in R.CASES.values() for v in c['skips'].values()} == {'gemm', 'centre'}
    assert {(R.case_cfg(i)['in_channels'] + 7) // 8 * 8 - R.case_cfg(i)['in_channels'] for i in R.CASE_IDS
            if 'conv_in' in R.stage_names(i)} == {0, 5, 6}
    assert {c['objects'] for c in R.CASES.values()} >= {1, 2, 3} and {R.case_cfg(i)['num_frames'] for i in R.CASE_IDS} >= {1, 2, 5, 6, 8, 9}
    assert any(c['H'] != c['W'] for c in R.CASES.values() if c['stage'] is None)
    assert any(c['ring_gemm'] for c in R.CASES.values()) and not any(c['ring_gemm'] for c in R.CASES.values() if c['stage'] and not c['raises'])


# ------------------------------------------------------------------------------------------------ oracle self-consistency
@pytest.mark.parametrize("cid", R.WALKED)
def test_forward_is_the_chained_stages_bit_for_bit(cid):
    """oracle.encoder.forward == run_stage chained by hand, in fp32, float64 and under rounding; the taps are those tensors; pooled is
    the mean over each object's frames"""
    cfg, x = R.case_cfg(cid), R.case_input(cid)
    for dt, rounded in ((torch.float32, False), (torch.float64, False), (torch.float64, True)):
        sd = {k: v.to(dt) for k, v in R.cfg_sd(R.CASES[cid]['cfg']).items()}

        def both():
            taps = {}
            y = oenc.forward(sd, cfg, x.to(dt), taps)
            h = x.to(dt)
            for name in oenc.stages(cfg):
                assert torch.equal(taps[name][0], h)
                h = oenc.run_stage(sd, cfg, name, h)
                assert torch.equal(taps[name][1], h)
            return y, h
        with torch.no_grad():
            if rounded:
                with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
                    y, chained = both()
            else:
                y, chained = both()
            assert y.dtype == dt and torch.equal(y, chained)
            if not rounded:
                Fr = cfg['num_frames']
                p = oenc.pooled(sd, cfg, x.to(dt))
                assert torch.equal(p, y.reshape(-1, Fr, *y.shape[1:]).mean(1))
    assert torch.equal(R.net_taps(cid)['conv_out'][1], R.run(cid, None, x, whole=True))


def test_frames_1_is_the_unet_transformer_bit_for_bit():
    """spatial_transformer(frames=1) is the function the U-Net oracle always was (its fp32 results stay bit-identical); with frames = F
    the joint attention couples the frames of an object and nothing else"""
    cid = 'f2-8x16'
    cfg, sd = R.case_cfg(cid), R.cfg_sd('f2')
    x = R.case_input(cid)
    p = dict(heads=cfg['n_heads'], depth=1)
    with torch.no_grad():
        a = ounet.spatial_transformer(sd, 'mid.attn_1', x, None, p)
        b = ounet.spatial_transformer(sd, 'mid.attn_1', x, None, p, frames=1)
        j = ounet.spatial_transformer(sd, 'mid.attn_1', x, None, p, frames=2)
        x2 = x.clone()
        x2[0] += 0.5
        j2 = ounet.spatial_transformer(sd, 'mid.attn_1', x2, None, p, frames=2)
    assert torch.equal(a, b) and not torch.equal(a, j)
    assert not torch.equal(j[1], j2[1]) and torch.equal(j[2:], j2[2:])


# ------------------------------------------------------------------------------------------------ injected defects
def _judge(what, y_bad, y16, y64):
    rho, _ = R.pixel_rho(y_bad, y16, y64)
    where, w = R.worst_pixel(rho)
    e = rel_l2(y_bad, y16)
    print(f'{what}: worst pixel (frame, pixel) = {where} rho = {w:.3g}, pixels over the cap {int((rho > CAP).sum())} of {rho.numel()}; '
          f'whole-tensor rel-L2 {e:.2e} (the old {OLD_GATE:g} gate would have seen it: {e >= OLD_GATE})')
    assert torch.isfinite(rho).all()
    return rho[:, 0], e                    # [N, pixels]


def test_defect_attn1_per_frame_instead_of_joint(monkeypatch):
    cid, name = 'rel64', 'mid_attn_1'
    x_in, y64, y16 = R.stage_pair(cid, name)
    tr = oenc.transformer
    monkeypatch.setattr(oenc, 'transformer', lambda sd, cfg, x, frames=None: tr(sd, cfg, x, frames=1))
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, _ = _judge('attn1 per frame', bad, y16, y64)
    assert float(rho.min()) > CAP


def test_defect_frames_of_two_objects_interleaved():
    """row order (frame, object) instead of (object, frame): attn1 groups frames of different objects; everything per frame is unmoved"""
    cid, name = 'rel64', 'mid_attn_1'
    x_in, y64, y16 = R.stage_pair(cid, name)
    B, Fr = R.CASES[cid]['objects'], R.case_cfg(cid)['num_frames']
    sw = lambda t, a, b: t.reshape(a, b, *t.shape[1:]).transpose(0, 1).reshape(t.shape)
    bad = sw(R.run(cid, name, sw(x_in, B, Fr)), Fr, B)
    rho, _ = _judge('frames of two objects interleaved', bad, y16, y64)
    assert float((rho > CAP).float().mean()) > 0.99
    ok = R.run(cid, 'mid_block_1', sw(R.stage_pair(cid, 'mid_block_1')[0], B, Fr))    # a per-frame stage does not see the order
    assert torch.equal(sw(ok, Fr, B), R.stage_pair(cid, 'mid_block_1')[2])


@pytest.mark.parametrize("cid", ['ds-8x24-c32', 'ds-16x16-c256'])
def test_defect_downsample_padded_on_the_other_side(monkeypatch, cid):
    name = R.CASES[cid]['stage']
    x_in, y64, y16 = R.stage_pair(cid, name)
    monkeypatch.setattr(oenc, 'downsample', lambda sd, pre, x: ounet._conv(sd, pre + '.conv', F.pad(x, (1, 0, 1, 0)), stride=2, padding=0))
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, _ = _judge(f'{cid}: Downsample padded (1,0,1,0)', bad, y16, y64)
    assert float(rho.min()) > CAP


@pytest.mark.parametrize("cid", ['ds-8x24-c32', 'ds-16x16-c256'])
def test_defect_downsample_from_the_odd_origin(monkeypatch, cid):
    """windows at (2 oy + 1, 2 ox + 1) instead of (2 oy, 2 ox)"""
    name = R.CASES[cid]['stage']
    x_in, y64, y16 = R.stage_pair(cid, name)
    monkeypatch.setattr(oenc, 'downsample', lambda sd, pre, x: ounet._conv(sd, pre + '.conv', F.pad(x[..., 1:, 1:], (0, 2, 0, 2)), stride=2,
                                                                          padding=0))
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, _ = _judge(f'{cid}: Downsample from the odd origin', bad, y16, y64)
    assert float(rho.min()) > CAP


def test_defect_one_frame_downsampled_wrongly_is_found_where_it_is(monkeypatch):
    """ONE frame of twelve through a Downsample from the odd origin: every pixel of that frame is over the cap and no other frame moves"""
    cid, name = 'rel64', 'down0_ds'
    x_in, y64, y16 = R.stage_pair(cid, name)
    good = oenc.downsample

    def one_frame(sd, pre, x):
        y = good(sd, pre, x).clone()
        y[7] = ounet._conv(sd, pre + '.conv', F.pad(x[7:8, :, 1:, 1:], (0, 2, 0, 2)), stride=2, padding=0)[0]
        return y
    monkeypatch.setattr(oenc, 'downsample', one_frame)
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, _ = _judge('one frame of twelve from the odd origin', bad, y16, y64)
    assert float(rho[7].min()) > CAP and float(rho[[i for i in range(12) if i != 7]].max()) == 0.0


@pytest.mark.parametrize("cid", ['cin3', 'cin10'])
def test_defect_padded_input_channels_not_zero(cid):
    """the channels conv_in's input is padded with (3 -> 8, 10 -> 16) alias the first channels, in the activation and the packed weight"""
    x_in, y64, y16 = R.stage_pair(cid, 'conv_in')
    cfg = R.case_cfg(cid)
    cin = cfg['in_channels']
    pad = (cin + 7) // 8 * 8 - cin
    sd = dict(R.cfg_sd(R.CASES[cid]['cfg']))
    alias = torch.arange(pad) % cin
    sd['conv_in.weight'] = torch.cat([sd['conv_in.weight'], sd['conv_in.weight'][:, alias]], dim=1)
    bad = R.run(cid, 'conv_in', torch.cat([x_in, x_in[:, alias]], dim=1), sd=sd)
    rho, _ = _judge(f'{cid}: padded input channels alias channels 0..{pad - 1}', bad, y16, y64)
    assert float((rho > CAP).float().mean()) > 0.99
    # zeros in the activation alone are what the kernel writes: exact, whatever the weight holds there
    zero = R.run(cid, 'conv_in', F.pad(x_in, (0, 0, 0, 0, 0, pad)), sd=sd)
    assert rel_l2(zero, y16) < 1e-13


def test_defect_attn2_projection_swapped_with_attn1s():
    cid, name = 'dh48-rect', 'mid_attn_1'
    x_in, y64, y16 = R.stage_pair(cid, name)
    sd = dict(R.cfg_sd(R.CASES[cid]['cfg']))
    for leaf in ('weight', 'bias'):
        a, b = (f'mid.attn_1.transformer_blocks.0.attn{i}.to_out.0.{leaf}' for i in (1, 2))
        sd[a], sd[b] = sd[b], sd[a]
    rho, _ = _judge('o1 / o2 swapped', R.run(cid, name, x_in, sd=sd), y16, y64)
    assert float((rho > CAP).float().mean()) > 0.99


def _drop_last_frame(monkeypatch, cid, objects):
    """attn1's keys and values without the last frame's tokens, for the given objects"""
    c, cfg = R.CASES[cid], R.case_cfg(cid)
    HW = c['attn2'][0]
    ca = ounet.cross_attention

    def dropped(sd, pre, x, context, heads):
        y = ca(sd, pre, x, context, heads)
        if pre.endswith('.attn1'):
            assert x.shape[1] == cfg['num_frames'] * HW
            short = ca(sd, pre, x, x[:, :-HW], heads)      # a context: the small kernel's rounding, far below what a missing frame does
            y = y.clone()
            y[objects] = short[objects]
        return y
    monkeypatch.setattr(ounet, 'cross_attention', dropped)


@pytest.mark.parametrize("objects", [[0, 1], [1]])
def test_defect_last_frame_dropped_from_the_joint_keys(monkeypatch, objects):
    """measured: whole-tensor rel-L2 5.2e-3 (both objects) / 3.7e-3 (one): inside the old gate; per pixel rho up to 5.3"""
    cid, name = 'rel64', 'mid_attn_1'
    x_in, y64, y16 = R.stage_pair(cid, name)
    _drop_last_frame(monkeypatch, cid, objects)
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, e = _judge(f'last frame dropped from the joint keys of objects {objects}', bad, y16, y64)
    Fr = R.case_cfg(cid)['num_frames']
    hit = rho.reshape(2, Fr, -1)[objects]
    assert float((hit > CAP).float().mean()) > 0.5 and e < OLD_GATE
    if objects == [1]:
        assert float(rho.reshape(2, Fr, -1)[0].max()) == 0.0


@pytest.mark.parametrize("cid", ['dh48-rect', 'dh16'])
def test_defect_scale_of_the_padded_head_size(monkeypatch, cid):
    """Dp ** -0.5 instead of dh ** -0.5 on heads zero-padded 48 -> 64 and 16 -> 64 (measured: rho 1.9 at 48, where the scale is off by
    13 %, with a whole-tensor rel-L2 of 1.5e-3)"""
    name = 'mid_attn_1'
    x_in, y64, y16 = R.stage_pair(cid, name)
    kern = odit._sdpa_kernel
    monkeypatch.setattr(odit, '_sdpa_kernel', lambda q, k, v, one_tile, causal=False, dh_true=None: kern(q, k, v, one_tile, causal, None))
    bad = R.run(cid, name, x_in)
    monkeypatch.undo()
    rho, e = _judge(f'{cid}: scale Dp ** -0.5', bad, y16, y64)
    assert float(rho.max()) > CAP and e < OLD_GATE


def test_defect_groupnorm_eps_is_not_reliably_seen_at_cap_1(monkeypatch):
    """GroupNorm eps 1e-5 for 1e-6 in the ResnetBlocks.  The change itself is a few 1e-6 relative, but it moves bf16 operands across
    rounding boundaries, and each flip is worth a bf16 ulp: measured worst rho 0.65 (rel64 down1), 0.61 (rel64 mid_block_1), 1.30
    (dh48-rect down0, 52 of 36 864 pixels over 1.0), whole-tensor rel-L2 6e-4 .. 1e-3 - the size of what two correct implementations
    differ by (test_fp32_working_precision_is_the_size_of_what_a_stage_may_differ_by).  The criterion does not reliably see it and this
    test records that - as the LN eps and the tanh-GELU were recorded for the conditioner towers - instead of dropping the defect from
    the list."""
    worst, over = 0.0, 0.0
    for cid, name in (('rel64', 'down1'), ('rel64', 'mid_block_1'), ('dh48-rect', 'down0')):
        x_in, y64, y16 = R.stage_pair(cid, name)
        monkeypatch.setattr(odec, '_gn', lambda x, sd, p: F.group_norm(x, 32, sd[p + 'weight'], sd[p + 'bias'], eps=1e-5))
        bad = R.run(cid, name, x_in)
        monkeypatch.undo()
        rho, e = _judge(f'{cid}/{name}: GroupNorm eps 1e-5', bad, y16, y64)
        assert 0.1 < float(rho.max()) and e < OLD_GATE
        worst, over = max(worst, float(rho.max())), max(over, float((rho > CAP).float().mean()))
    assert worst < 3.0 and over < 0.01     # not reliably seen at 1.0: under 1 % of the pixels of any stage are over it


def test_no_defect_is_rho_zero():
    """without a defect the same computation gives rho = 0 everywhere"""
    for cid, name in (('rel64', 'mid_attn_1'), ('dh48-rect', 'mid_attn_1'), ('ds-8x24-c32', 'down0_ds'), ('cin10', 'conv_in'),
                      ('rel64', 'down0_ds'), ('dh16', 'mid_attn_1')):
        x_in, y64, y16 = R.stage_pair(cid, name)
        assert float(R.pixel_rho(R.run(cid, name, x_in), y16, y64)[0].max()) == 0.0


# ------------------------------------------------------------------------------------------------ why per stage, and what a cap can be
def test_fp32_working_precision_is_the_size_of_what_a_stage_may_differ_by():
    """The restatement at fp32 working precision against itself at float64 - two correct bf16 implementations.  End to end they
    decorrelate past any cap <= 1.0; one stage on the same input stays inside it, and its worst pixel is what a HIP stage may be
    expected to show.  Measured (rel64 / ch32-128 / dh48-rect): end to end median rho 0.69 / 0.64 / 0.72, worst 1.35 / 1.53 / 1.34; one
    stage: convs alone 6e-5 .. 1e-4, ResnetBlock stages 0.001 .. 0.96 (down0: 0.49 / 0.75 / 0.96) with a median of 3e-5, mid_attn_1
    0.72 / 0.78 / 0.75 with a median of 0.45."""
    for cid in R.WALKED:
        cfg, sd = R.case_cfg(cid), R.cfg_sd(R.CASES[cid]['cfg'])
        worst = {}
        pairs = {name: R.stage_pair(cid, name) for name in R.stage_names(cid)}     # outside the rounding context: y64 is unrounded
        with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            for name, (x_in, y64, y16) in pairs.items():
                y32 = oenc.run_stage(sd, cfg, name, x_in)
                assert y32.dtype == torch.float32
                worst[name] = float(R.pixel_rho(y32.double(), y16, y64)[0].max())
            e32 = oenc.forward(sd, cfg, R.case_input(cid))
        y64 = R.run(cid, None, R.case_input(cid), rounded=False, whole=True)
        rho, _ = R.pixel_rho(e32.double(), R.net_taps(cid)['conv_out'][1], y64)
        print(f'{cid}: end to end median rho {float(rho.median()):.2f} worst {float(rho.max()):.2f}; one stage: ' +
              ', '.join(f'{n} {w:.2g}' for n, w in worst.items()))
        assert float(rho.max()) > CAP > max(worst.values())
        assert max(worst[n] for n in worst if n == 'conv_in' or n.endswith('_ds')) < 1e-3
