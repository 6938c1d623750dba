"""The per-pixel, per-block criterion of tests/unet_pixel_refs.py checked without a GPU: the health of its yardstick for every
(case, block) test_unet_pixels_gpu.py runs, the launch every case states against ln3diff_amd.convstack and csrc/kernel_plan.h, the
oracle's self-consistency (unet_forward IS the chained run_block; num_heads_upsample moves exactly the output blocks' heads), and -
the point of it - that the criterion REJECTS the defects a whole-tensor rel-L2 < 2e-2 gate cannot see, where they are and nowhere else.

Why per block and not end to end (test_end_to_end_decorrelation_is_why_blocks_are_judged_one_by_one; measured here): the SAME
restatement run at float64 and at fp32 working precision - two correct bf16 implementations - differs end to end by
    st         median rho 0.80, worst 5.41
    attn-roll  median rho 0.71, worst 1.89
    attn-96    median rho 0.70, worst 3.88
of what operand rounding does to a pixel, so no cap at or below 1.0 can hold end to end; one block on the same input differs by a
worst rho, over the blocks of a network, of 0.71 / 0.46 / 0.56 (the transformer blocks the most)."""
import pytest
import torch
import torch.nn.functional as F

import unet_pixel_refs as R
from conftest import rel_l2
from ln3diff_amd import convstack
from ln3diff_amd.dit.dit_models_xformers import attn_head_pad
from oracle import dit as odit
from oracle import unet as ounet

CAP = 1.0              # the GPU test's caps are at or below this; a defect rejected at 1.0 is rejected at any tighter cap
NET_BLOCKS = [(n, b) for n in R.WALKED for b in R.block_names(n)]
RUN_CASES = [i for i in R.CASE_IDS if not R.CASES[i]['raises']]


# ------------------------------------------------------------------------------------------------ yardstick
def _healthy(who, y16, y64):
    med, mx = R.pixel_yardstick(y16, y64)
    print(f'{who}: d / |y64| per pixel: median {med:.2e} max {mx:.2e}')
    assert R.YARD_MEDIAN[0] <= med <= R.YARD_MEDIAN[1] and mx <= R.YARD_MAX, (who, med, mx)


@pytest.mark.parametrize("net", R.WALKED)
def test_yardstick_of_every_block_of_the_networks(net):
    """measured: medians 1.8e-3 .. 4.2e-3, worst pixel 1.9e-2 (the 4-channel head)"""
    for name in R.block_names(net):
        _, _, y64, y16 = R.block_pair(net, name)
        _healthy(f'{net} {name}', y16, y64)


@pytest.mark.parametrize("cid", RUN_CASES)
def test_yardstick_of_every_single_block(cid):
    """measured: the AttentionBlocks 1.4e-4 .. 3.0e-4 (the residual dominates under the synthetic weights), the others 4e-4 .. 2.8e-3"""
    y64, y16 = R.single_pair(cid)
    _healthy(cid, y16, y64)


# ------------------------------------------------------------------------------------------------ the stated launches
def _walk(net):
    """[(block, layer kind, params, H, W at the layer's input)] of a network"""
    c = R.NETS[net]
    H, W = c['image_size'], c['image_size'] * (3 if c['roll_out'] else 1)
    out = []
    for name, layers in ounet.blocks(c):
        for kind, p in layers:
            out.append((name, kind, p, H, W))
            if kind == 'down':
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            elif kind == 'up':
                H, W = 2 * H, 2 * W
    return out


def _product_route(dh, L):
    """ConvStack.self_attend's own condition: the MFMA kernels, or 'small'"""
    return 'mfma' if convstack.mfma_head(dh) and L >= convstack.MFMA_MIN_TOKENS and L % 32 == 0 else 'small'


def test_every_case_states_the_launch_the_product_and_the_plan_give(tmp_path):
    assert ounet.MFMA_MIN_TOKENS == convstack.MFMA_MIN_TOKENS
    for dh in (8, 12, 32, 40, 48, 64, 72, 80, 96, 128, 136, 160):
        assert ounet.head_pad(dh) == attn_head_pad(dh)
        for L in (64, 255, 256, 288, 289, 1024):
            assert (ounet.attn_route(dh, L) == 'small') == (_product_route(dh, L) == 'small'), (dh, L)
            assert ounet.attn_route(dh, L, self_attention=False) == 'small'
    # ---- what the walked networks contain is what NET_LAUNCH says
    for net in R.WALKED:
        st, walk = R.NET_LAUNCH[net], _walk(net)
        B = len(R.TIMESTEPS)
        attn = {(p['ch'] // p['heads'], H * W) for _, k, p, H, W in walk if k in ('attention', 'transformer')}
        assert attn == set(st['self_attn']), (net, attn)
        m = R.build_net(net)
        skips = {}
        for blk in [*m.input_blocks, m.middle_block, *m.output_blocks]:
            for layer in blk:
                if layer.__class__.__name__ == 'ResBlock' and not isinstance(layer.skip_connection, torch.nn.Identity):
                    q = convstack.pack_resblock(layer.in_layers[0], layer.in_layers[2], layer.out_layers[0], layer.out_layers[3], torch.device('cpu'),
                                                shortcut=layer.skip_connection)
                    skips[layer.channels] = 'centre' if 'kpad' in q['skip'] else 'gemm'
        assert skips == st['skips'], (net, skips)
        rows = max(B * H * W * (4 if k == 'up' else 1) for _, k, p, H, W in walk)
        assert rows == st['rows'] and st['ring_gemm'] == (rows >= R.GEMM_RING_ROWS), (net, rows)
        assert all(B * p['heads'] < R.CUS for _, k, p, _, _ in walk if k in ('attention', 'transformer'))
    # ---- every stated self-attention launch against ConvStack.self_attend's condition, the oracle's assumption and the plan
    launches = R.mfma_launches()
    planned = R.plan([ln for _, _, ln in launches], tmp_path)
    for (who, route, ln), (kernel, ring) in zip(launches, planned):
        assert ln[3] < R.CUS, who                                     # B * heads: never a head for every CU
        if route != 'small':
            assert kernel != 'kres' and R.ROUTE_OF_KERNEL[kernel] == route, (who, ln, kernel, route)
    for c in R.CASES.values():
        for dh, L, route, is_self in c['attn']:
            assert ounet.attn_route(dh, L, is_self) == route, (c['id'], dh, L, route)
            assert (route == 'small') == (not is_self or _product_route(dh, L) == 'small'), (c['id'], dh, L)
            assert L == (c['H'] * c['W'] if is_self else c['Lc']), c['id']
        assert c['ring_gemm'] is False, c['id']                       # no single case leaves the 128x128 tile; attn-roll does (2304 rows)
    for net in R.WALKED:
        for (dh, L), route in R.NET_LAUNCH[net]['self_attn'].items():
            assert ounet.attn_route(dh, L) == route and (route == 'small') == (_product_route(dh, L) == 'small'), (net, dh, L)
    ring = {who: r for (who, _, _), (_, r) in zip(launches, planned)}
    assert ring['attn-roll'] is True and ring['st'] is False and ring['attn-96'] is False
    assert not any(ring[c['id']] for c in R.CASES.values() if c['id'] in ring)
    # ---- the cases reach what they are there for
    routes = {r for c in R.CASES.values() for _, _, r, s in c['attn'] if s}
    assert routes == {'stream', 'ring64', 'ring80', 'ring128', 'small'}
    assert {c['Lc'] for c in R.CASES.values() if c['Lc']} == {1, 64, 65, 77}
    # the one case that must raise: too many tokens for ln3d_attention_small at a head size the MFMA route refuses
    c = R.CASES['ab-320h2-33x32']
    assert c['raises'] and not convstack.mfma_head(160) and c['H'] * c['W'] > 1024


# ------------------------------------------------------------------------------------------------ oracle self-consistency
@pytest.mark.parametrize("net", R.WALKED)
def test_forward_is_the_chained_blocks_bit_for_bit(net):
    """unet_forward == run_block chained by hand with the skip stack, in fp32, float64 and under rounding; the taps are those tensors"""
    cfg = R.NETS[net]
    x, t, ctx = R.net_inputs(net)
    for dt, rounded in ((torch.float32, False), (torch.float64, False), (torch.float64, True)):
        sd = {k: v.to(dt) for k, v in R.net_sd(net).items()}
        xx, cc = x.to(dt), None if ctx is None else ctx.to(dt)

        def both():
            taps = {}
            y = ounet.unet_forward(sd, cfg, xx, t.to(dt), cc, taps)
            emb = ounet.time_embed(sd, cfg, t.to(dt))
            h, hs = ounet.roll(xx) if cfg['roll_out'] else xx, []
            for name, _ in ounet.blocks(cfg):
                if name.startswith('output_blocks'):
                    h = torch.cat([h, hs.pop()], dim=1)
                assert torch.equal(taps[name][0], h)
                h = ounet.run_block(sd, cfg, name, h, emb, cc)
                assert torch.equal(taps[name][1], h)
                if name.startswith('input_blocks'):
                    hs.append(h)
            assert not hs and torch.equal(taps['time_embed'][1], emb)
            return y, ounet.unroll(h) if cfg['roll_out'] else h
        with torch.no_grad():
            if rounded:
                with odit.operand_rounding(torch.bfloat16, kernel_arith=True):
                    y, chained = both()
            else:
                y, chained = both()
        assert y.dtype == dt and torch.equal(y, chained)
    y64, y16, _ = R.net_oracles(net)
    with torch.no_grad():
        y32 = ounet.unet_forward(R.net_sd(net), cfg, x, t, ctx)
    assert y32.dtype == torch.float32 and rel_l2(y32, y64) < 1e-5 and 1e-4 < rel_l2(y16, y64) < 5e-2


def test_layout_honours_num_heads_upsample_in_the_output_blocks_only():
    cfg = R.NETS['attn-96']
    assert cfg['num_heads_upsample'] == 1 and cfg['num_heads'] == 2
    with_, without = ounet.layout(cfg), ounet.layout(dict(cfg, num_heads_upsample=-1))
    assert with_[0] == without[0] and with_[1] == without[1]
    n = 0
    for a, b in zip(with_[2], without[2]):
        assert len(a) == len(b)
        for (ka, pa), (kb, pb) in zip(a, b):
            assert ka == kb
            if ka == 'attention':
                assert pa == dict(pb, heads=1) and pb['heads'] == 2
                n += 1
            else:
                assert pa == pb
    assert n == 4
    # the product's constructor agrees (its AttentionBlocks carry the head count), for this network and for num_head_channels / legacy=False
    for net in ('attn-96', 'nhc32', 'attn-roll'):
        m = R.build_net(net)
        mods = [*m.input_blocks, m.middle_block, *m.output_blocks]
        lay = ounet.layout(R.NETS[net])
        for blk, layers in zip(mods, [*lay[0], *lay[1:2], *lay[2]]):
            for layer, (kind, p) in zip(blk, layers):
                if kind == 'attention':
                    assert layer.num_heads == p['heads'], (net, p)
    # a SpatialTransformer network takes (num_heads, dim_head) everywhere, as the reference constructor does
    st = ounet.layout(dict(R.NETS['st'], num_heads_upsample=1))
    assert st == ounet.layout(R.NETS['st'])


# ------------------------------------------------------------------------------------------------ injected defects
def _judge(what, y_bad, y16, y64):
    rho, _ = R.pixel_rho(y_bad, y16, y64)
    where, w = R.worst_pixel(rho)
    e = rel_l2(y_bad, y16)
    print(f'{what}: worst pixel (sample, pixel) = {where} rho = {w:.2f}, pixels over the cap {int((rho > CAP).sum())} of {rho.numel()}; '
          f'whole-tensor rel-L2 {e:.2e} (passes a 2e-2 gate: {e < 2e-2})')
    assert torch.isfinite(rho).all()
    return rho[:, 0]                       # [B, pixels]


def test_defect_replicate_padding_on_one_conv(monkeypatch):
    """the stem conv of attn-96 with replicate instead of zero padding: every border pixel over the cap, every interior pixel untouched"""
    net, name = 'attn-96', 'input_blocks.0'
    x_in, emb, y64, y16 = R.block_pair(net, name)
    conv = ounet._conv

    def replicate(sd, pre, x, stride=1, padding=1):
        if pre == 'input_blocks.0.0':
            return conv(sd, pre, F.pad(x, (1, 1, 1, 1), mode='replicate'), stride, 0)
        return conv(sd, pre, x, stride, padding)
    monkeypatch.setattr(ounet, '_conv', replicate)
    bad = R.run_net_block(net, name, x_in, emb)
    monkeypatch.undo()
    rho = _judge('replicate padding', bad, y16, y64).reshape(3, 16, 16)
    border = torch.ones(16, 16, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert bool((rho[:, border] > CAP).all()) and float(rho[:, ~border].max()) == 0.0


def test_defect_another_samples_embedding_row():
    """sample b given sample b + 1's embedding row in one ResBlock + transformer block: every pixel of every sample over the cap"""
    net, name = 'st', 'input_blocks.1'
    x_in, emb, y64, y16 = R.block_pair(net, name)
    rho = _judge('embedding row of the next sample', R.run_net_block(net, name, x_in, emb.roll(-1, 0)), y16, y64)
    assert float(rho.min()) > CAP


def test_defect_legacy_qkv_rows_not_reordered():
    """AttentionBlock with 4 heads whose qkv rows are read as [q | k | v][head][ch] without the re-ordering from the legacy
    [head][q | k | v][ch]: every pixel over the cap (measured: worst rho 457)"""
    cid = 'ab-128h4-16x16'
    y64, y16 = R.single_pair(cid)
    sd = dict(R.single_sd(cid))
    nh, C = 4, 128
    for leaf in ('weight', 'bias'):
        w = sd[f'blk.0.qkv.{leaf}']
        sd[f'blk.0.qkv.{leaf}'] = w.reshape(3, nh, C // nh, -1).transpose(0, 1).reshape(w.shape)
    rho = _judge('legacy head order ignored', R.run_single(cid, sd=sd), y16, y64)
    assert float((rho > CAP).float().mean()) > 0.99


def test_defect_num_heads_upsample_ignored():
    """the output blocks' AttentionBlocks run with num_heads instead of num_heads_upsample: over the cap in every output block, and the
    input and middle blocks are untouched"""
    net = 'attn-96'
    cfg = dict(R.NETS[net], num_heads_upsample=-1)
    sd, ctx = R.to64(R.net_sd(net)), None
    for name in R.block_names(net)[1:]:
        x_in, emb, y64, y16 = R.block_pair(net, name)
        with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            bad = ounet.run_block(sd, cfg, name, x_in.double(), emb.double(), ctx)
        rho = _judge(f'num_heads_upsample ignored, {name}', bad, y16, y64)
        if name.startswith('output_blocks'):
            assert float((rho > CAP).float().mean()) > 0.99, name
        else:
            assert float(rho.max()) == 0.0, name


def test_defect_nearest_upsample_source_off_by_one(monkeypatch):
    """the nearest-2x source column (x + 1) // 2 instead of x // 2"""
    cid = 'up-5x7'
    y64, y16 = R.single_pair(cid)
    up = ounet.upsample2x
    monkeypatch.setattr(ounet, 'upsample2x', lambda h: torch.cat([up(h)[..., 1:], up(h)[..., -1:]], dim=-1))
    bad = R.run_single(cid)
    monkeypatch.undo()
    rho = _judge('nearest-2x source off by one', bad, y16, y64).reshape(2, 10, 14)
    # output columns 12 and 13 read source column 6 either way (7 is clamped), so the last output column sees no change
    assert bool((rho[..., :-1] > CAP).all()) and float(rho[..., -1].max()) == 0.0


def test_defect_strided_conv_from_the_odd_origin(monkeypatch):
    """the stride-2 conv centred on (2 oy + 1, 2 ox + 1) - the ldm Downsample's pad (0, 1, 0, 1) - instead of (2 oy, 2 ox)"""
    cid = 'down-8x8'
    y64, y16 = R.single_pair(cid)
    conv = ounet._conv
    monkeypatch.setattr(ounet, '_conv', lambda sd, pre, x, stride=1, padding=1: conv(sd, pre, F.pad(x, (0, 1, 0, 1)), stride, 0) if stride == 2
                        else conv(sd, pre, x, stride, padding))
    bad = R.run_single(cid)
    monkeypatch.undo()
    rho = _judge('stride-2 conv from the odd origin', bad, y16, y64)
    assert float(rho.min()) > CAP


def test_defect_skip_concat_halves_swapped():
    """cat([skip, h]) instead of cat([h, skip]) in front of an output block (96 + 64 channels)"""
    net, name = 'attn-96', 'output_blocks.1'
    x_in, emb, y64, y16 = R.block_pair(net, name)
    assert x_in.shape[1] == 160
    rho = _judge('skip concat swapped', R.run_net_block(net, name, torch.cat([x_in[:, 96:], x_in[:, :96]], dim=1), emb), y16, y64)
    assert float(rho.min()) > CAP


def test_defect_last_context_key_dropped():
    """the 65th of 65 context keys dropped (a key behind a 64-key lane round)"""
    cid = 'st-128h4-d2-lc65'
    y64, y16 = R.single_pair(cid)
    ctx = R.single_inputs(cid)[2]
    rho = _judge('last of 65 context keys dropped', R.run_single(cid, ctx=ctx[:, :64]), y16, y64)
    assert float((rho > CAP).float().mean()) > 0.99


def test_defect_centre_tap_shortcut_in_a_corner_tap(monkeypatch):
    """the 1x1 shortcut that runs as the centre tap of a 3x3 (input width 160) with its weight in tap (0, 0)"""
    cid = 'res-n1-160to96'
    y64, y16 = R.single_pair(cid)
    conv = ounet._conv
    monkeypatch.setattr(ounet, '_conv', lambda sd, pre, x, stride=1, padding=1: conv(sd, pre, F.pad(x, (1, 0, 1, 0))[..., :-1, :-1], stride, padding)
                        if pre.endswith('skip_connection') else conv(sd, pre, x, stride, padding))
    bad = R.run_single(cid)
    monkeypatch.undo()
    rho = _judge('centre-tap shortcut in a corner tap', bad, y16, y64)
    assert float(rho.min()) > CAP


def test_no_defect_is_rho_zero():
    """without a defect the same computation gives rho = 0 everywhere"""
    for cid in ('up-5x7', 'res-n1-160to96', 'st-128h4-d2-lc65'):
        y64, y16 = R.single_pair(cid)
        assert float(R.pixel_rho(R.run_single(cid), y16, y64)[0].max()) == 0.0


# ------------------------------------------------------------------------------------------------ why per block
def test_end_to_end_decorrelation_is_why_blocks_are_judged_one_by_one():
    """The restatement at fp32 working precision against itself at float64: end to end the two decorrelate past any cap <= 1.0 (the
    figures of the module docstring), one block on the same input stays far inside it."""
    for net in R.WALKED:
        cfg = R.NETS[net]
        x, t, ctx = R.net_inputs(net)
        y64, y16, taps = R.net_oracles(net)
        with torch.no_grad(), odit.operand_rounding(torch.bfloat16, kernel_arith=True):
            y16_32 = ounet.unet_forward(R.net_sd(net), cfg, x, t, ctx)
            assert y16_32.dtype == torch.float32
            rho, _ = R.pixel_rho(y16_32.double(), y16, y64)
            worst_block = 0.0
            for name in R.block_names(net)[1:]:
                x_in, emb, b64, b16 = R.block_pair(net, name)
                b32 = ounet.run_block(R.net_sd(net), cfg, name, x_in, emb, ctx)
                worst_block = max(worst_block, float(R.pixel_rho(b32.double(), b16, b64)[0].max()))
        print(f'{net}: end to end median rho {float(rho.median()):.2f} worst {float(rho.max()):.2f}; one block, worst over the blocks {worst_block:.2f}')
        assert float(rho.max()) > CAP > worst_block
