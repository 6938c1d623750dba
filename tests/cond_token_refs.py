"""Per-token criterion for the four conditioner towers (CPU only: torch and the oracle, no HIP) - the analogue of dit_token_refs.py,
whose criterion it reuses unchanged (token_rho / worst_token / yardstick: a [B, T, D] output is one group per (b, t) there).

The towers: the CLIP-L text tower (FrozenCLIPEmbedder), the OpenCLIP visual tower (FrozenOpenCLIPImageEmbedder), DINOv2 with
registers (FrozenDinov2ImageEmbedder) and the 9-channel multi-view Pluecker DINOv2 (FrozenDinov2ImageEmbedderMVPlucker through
MV23DConditioner), all on the shared pre-LN block dit_models_xformers.vit_block_hip.  All are width 128, depth 2, 2 heads (one
DINOv2 case: width 256, 2 heads = Dh 128) with the synthetic weights of seed 0 (synth_state_dict for CLIP, synth_vit_state_dict for
DINOv2: LayerScale gammas 1 + 0.1 N).  The TOKENS of a case are everything its forward returns, as named parts of shape
[B, groups, D]:
    text      'last'   [B, T, D]
    openclip  'tokens' [B, Lp, D] (the patch tokens) and 'pooled' [B, 1, E] (one group per sample, judged on its own)
    dino      'tokens' [B, 1 + Lp, D] (output_cls=True: cls, then the patch tokens)
    mv        'tokens' [B, n_cond_frames * Lp, D] (every (b, view, l))
For every part, y64 is the float64 oracle (oracle/clip_text.py, oracle/vit_image.py on a float64 state dict) and y16 the same under
operand_rounding(bf16, kernel_arith=True); a tower passes when max rho <= CAP over every group of every part.

Every case states the launch it expects - the attention kernel and whether the block GEMMs leave the 128x128 tile - and
tests/test_cond_tokens_cpu.py checks those statements against csrc/kernel_plan.h, so that a retuned threshold cannot silently move a
case onto another path.  No case has a key count that is a multiple of 256 (the streaming attention kernel: no released tower
config has one), asserted below.
"""
import functools

import torch

from dit_token_refs import YARD_MAX, YARD_MEDIAN, to64, token_rho, worst_token, yardstick      # noqa: F401  (the criterion, not forked)
from ln3diff_amd.synth import orbit_cameras, synth_input, synth_state_dict, synth_vit_state_dict
from oracle import clip_text as oclip
from oracle import dit as odit
from oracle import vit_image as ovit

D, DEPTH, HEADS, PATCH = 128, 2, 2, 14
TEXT_VOCAB, TEXT_MLP, CLIP_MLP, CLIP_EMBED = 1000, 256, 256, 64
GEMM_RING_ROWS = 1536          # csrc/kernel_plan.h: a GEMM leaves the 128x128 register-staged tile at M >= 1536 and N >= 128


# ------------------------------------------------------------------------------------------------ cases
def _text_ids(kind, B, T):
    g = torch.Generator().manual_seed(77 * T + B)
    if kind == 'eos999':                                   # EOS at 1 / 40 / 76, the EOS id repeated as padding behind it
        ids = torch.randint(1, 999, (B, T), generator=g)
        for b, pos in enumerate((1, 40, 76)):
            ids[b, pos:] = 999
        return ids, torch.tensor([1, 40, 76])
    ids = torch.randint(3, 900, (B, T), generator=g)
    if kind == 'legacy':                                   # eos_token_id == 2: the FIRST occurrence of the largest id
        ids[0, 20] = ids[0, 50] = 950                      # twice in one row
        ids[1, 76] = 950
        ids[2, 0] = 950
        return ids, torch.tensor([20, 76, 0])
    return ids, ids.argmax(-1)


def _text(cid, T, B, kind='plain', max_pos=77, why=''):
    ids, pos = _text_ids(kind, B, T)
    return dict(id=cid, tower='text', B=B, T=T, seqs=B, heads=HEADS, width=D, why=why,
                kw=dict(always_return_pooled=True, vocab_size=TEXT_VOCAB, hidden_size=D, intermediate_size=TEXT_MLP, num_hidden_layers=DEPTH,
                        num_attention_heads=HEADS, eos_token_id=999 if kind == 'eos999' else 2, max_position_embeddings=max_pos),
                ids=ids, eos_pos=pos)


def _image(cid, tower, S, B, why='', R=4, width=D, version='openai', n_cond_frames=0, views=0):
    Lp = (S // PATCH) ** 2
    c = dict(id=cid, tower=tower, B=B, S=S, Lp=Lp, heads=HEADS, width=width, why=why)
    if tower == 'openclip':
        c.update(T=1 + Lp, seqs=B, act='quick_gelu' if version == 'openai' else 'gelu', img=synth_input('img', (B, 3, S, S), 3),
                 kw=dict(output_tokens=True, version=version, arch='custom', width=width, mlp_width=CLIP_MLP, layers=DEPTH, heads=HEADS,
                         image_size=S, embed_dim=CLIP_EMBED))
    elif tower == 'dino':
        c.update(T=1 + R + Lp, seqs=B, R=R, img=synth_input('img', (B, 3, S, S), 4),
                 kw=dict(output_cls=True, width=width, layers=DEPTH, heads=HEADS, image_size=S, num_register_tokens=R))
    else:                                                  # images at size, clamped to [-1, 1]: they go through preprocess
        V = n_cond_frames
        cams = torch.stack([orbit_cameras(views, elevation_deg=15.0 + 10.0 * b) for b in range(B)])
        c.update(T=1 + R + Lp, seqs=B * V, R=R, V=V, img=synth_input('mvimg', (B, views, 3, S, S), 7).clamp(-1, 1), cams=cams,
                 kw=dict(arch='vitb', n_cond_frames=V, width=width, layers=DEPTH, heads=HEADS, image_size=S, num_register_tokens=R))
    return c


def _cases():
    cs = [
        _text('text-eos999', 77, 3, 'eos999', why='tail of the 2nd key block; EOS pooling per sample'),
        _text('text-legacy', 77, 3, 'legacy', why='legacy argmax pooling: first occurrence of the largest id'),
        _text('text-T64', 64, 2, why='exactly one key block'),
        _text('text-T65', 65, 2, why='one key past a 64-key block: two key blocks'),
        _text('text-T33', 33, 2, why='a query tile partly past the end'),
        _text('text-T128', 128, 2, max_pos=128, why="the kernel's key limit, no tail mask"),
        _text('text-B20', 77, 20, why='M = 1540: block GEMMs on ring tiles, tiles straddle prompts'),
        _image('openclip-S56', 'openclip', 56, 2, 'T 17'),
        _image('openclip-S112', 'openclip', 112, 3, 'T 65: one token past a 64-key tile'),
        _image('openclip-S224', 'openclip', 224, 2, 'T 257: the production sequence'),
        _image('openclip-S224-B6', 'openclip', 224, 6, 'M = 1542: ring tiles'),
        _image('openclip-erf', 'openclip', 56, 2, 'erf-GELU epilogue (version != openai)', version='laion2b'),
        _image('dino-S56', 'dino', 56, 2, 'T 21'),
        _image('dino-S112', 'dino', 112, 3, 'T 69'),
        _image('dino-S224', 'dino', 224, 2, 'T 261'),
        _image('dino-S224-B6', 'dino', 224, 6, 'M = 1566: ring tiles'),
        _image('dino-R0', 'dino', 112, 2, 'T 65: reg=None path of vit_assemble', R=0),
        _image('dino-Dh128', 'dino', 56, 2, 'Dh 128: ring128', width=256),
        _image('mv-S56', 'mv', 56, 2, '9 channels, kpad 1792, view selection', n_cond_frames=2, views=3),
        _image('mv-S224-B1', 'mv', 224, 1, 'M = 1044: production token count below 1536', n_cond_frames=4, views=5),
        _image('mv-S224-B2', 'mv', 224, 2, 'M = 2088: above 1536', n_cond_frames=4, views=5),
    ]
    for c in cs:
        c['M'] = c['seqs'] * c['T']
        Dh = c['width'] // c['heads']
        # ---- the launch this case is expected to be (checked against csrc/kernel_plan.h by tests/test_cond_tokens_cpu.py)
        c['attn'] = 'short' if c['tower'] == 'text' else ('ring128' if Dh == 128 else ('ring64_occ4' if c['T'] > 128 else 'ring64_occ2'))
        c['ring_gemm'] = c['M'] >= GEMM_RING_ROWS                           # N >= 128 for every block GEMM (width >= 128)
        assert c['tower'] == 'text' or c['T'] % 256 != 0, "the streaming attention kernel is out of scope"
        c['ntok'] = {'text': c['M'], 'openclip': c['B'] * c.get('Lp', 0), 'dino': c['B'] * (1 + c.get('Lp', 0)),
                     'mv': c['seqs'] * c.get('Lp', 0)}[c['tower']]
    return {c['id']: c for c in cs}


CASES = _cases()
CASE_IDS = list(CASES)
TOWER_IDS = {t: [i for i in CASE_IDS if CASES[i]['tower'] == t] for t in ('text', 'openclip', 'dino', 'mv')}


def case(cid):
    return CASES[cid]


# ------------------------------------------------------------------------------------------------ towers and weights
def build_tower(c, **over):
    """the product module of a case (a parameter container until it runs: built on the CPU too, for its state-dict manifest)"""
    from ln3diff_amd.sgm.encoders import FrozenCLIPEmbedder
    from ln3diff_amd.sgm import image_encoders as ie
    cls = {'text': FrozenCLIPEmbedder, 'openclip': ie.FrozenOpenCLIPImageEmbedder, 'dino': ie.FrozenDinov2ImageEmbedder,
           'mv': ie.FrozenDinov2ImageEmbedderMVPlucker}[c['tower']]
    return cls(**dict(c['kw'], **over))


_PREFIX = {'text': 'transformer.', 'openclip': 'model.', 'dino': 'model.', 'mv': 'model.'}


@functools.lru_cache(maxsize=None)
def _synth_sd(tower, kw_items):
    c = dict(tower=tower, kw=dict(kw_items))
    pre = _PREFIX[tower]
    shapes = {k[len(pre):]: tuple(v.shape) for k, v in build_tower(c).state_dict().items()}
    empty = {k: torch.zeros(s) for k, s in shapes.items() if 0 in s}       # register_tokens [1, 0, D] of a tower without registers
    sd = (synth_state_dict if tower in ('text', 'openclip') else synth_vit_state_dict)({k: s for k, s in shapes.items() if k not in empty}, 0)
    return {**sd, **empty}


def synth_sd(c):
    """the synthetic fp32 state dict of a case's tower under the ORACLE's key names (seed 0, the goldens' recipe); shared, never modified"""
    return _synth_sd(c['tower'], tuple(sorted(c['kw'].items())))


def load_tower(c, **over):
    """the case's tower with its synthetic weights; `over` replaces constructor arguments (the weights depend on names and shapes only)"""
    c = dict(c, kw=dict(c['kw'], **over))
    m = build_tower(c)
    m.load_state_dict({_PREFIX[c['tower']] + k: v for k, v in synth_sd(c).items()}, strict=True)
    return m


def inputs(c):
    """what the oracle is called with (and, moved to the device, the tower)"""
    if c['tower'] == 'text':
        return {'ids': c['ids']}
    if c['tower'] == 'mv':
        return {'img': c['img'], 'c': c['cams']}
    return {'img': c['img']}


# ------------------------------------------------------------------------------------------------ tokens
def parts(c, out):
    """what a tower's forward (or its oracle, brought to the same order by oracle_forward) returns -> {part: [B, groups, D]}"""
    if c['tower'] == 'text':
        return {'last': out[0]}
    if c['tower'] == 'openclip':
        tokens, pooled = out
        return {'tokens': tokens, 'pooled': pooled.reshape(pooled.shape[0], 1, -1)}
    if c['tower'] == 'dino':
        cls, tokens = out
        return {'tokens': torch.cat([cls[:, None], tokens], 1)}
    return {'tokens': out.reshape(out.shape[0], -1, out.shape[-1])}


def oracle_forward(c, sd, inp):
    """the oracle of the case's tower on (sd, inputs) in their dtype, in the order the product forward returns"""
    with torch.no_grad():
        if c['tower'] == 'text':
            return oclip.clip_text_forward(sd, inp['ids'], c['heads'], c['kw']['eos_token_id'])
        if c['tower'] == 'openclip':
            pooled, tokens, _ = ovit.openclip_visual_forward(sd, inp['img'], c['heads'], act=c['act'])
            return tokens, pooled
        if c['tower'] == 'dino':
            return ovit.dinov2_forward(sd, inp['img'], c['heads'])
        return ovit.dinov2_mv_plucker_forward(sd, inp, c['heads'], n_cond_frames=c['V'], size=c['S'])


def rounded_oracle(cid, sd=None, inp=None, kernel_arith=True):
    """y16 parts of a case, computed afresh (the planted-error tests call it with oracle functions, weights or inputs replaced)"""
    c = case(cid)
    with odit.operand_rounding(torch.bfloat16, kernel_arith=kernel_arith):
        return parts(c, oracle_forward(c, to64(synth_sd(c) if sd is None else sd), to64(inputs(c) if inp is None else inp)))


@functools.lru_cache(maxsize=None)
def oracle_pair(cid):
    """(y64, y16) of a case, each {part: float64 [B, groups, D]}: one computation per process"""
    c = case(cid)
    y64 = parts(c, oracle_forward(c, to64(synth_sd(c)), to64(inputs(c))))
    y16 = rounded_oracle(cid)
    assert all(v.dtype == torch.float64 for v in (*y64.values(), *y16.values()))
    return y64, y16


def judge(cid, y):
    """y: parts of a forward -> {part: (rho [B, 1, groups], d)}; every returned number is in exactly one group"""
    y64, y16 = oracle_pair(cid)
    assert set(y) == set(y64), (set(y), set(y64))
    return {k: token_rho(y[k], y16[k], y64[k], None) for k in y64}
