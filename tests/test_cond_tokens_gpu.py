"""Every token of the four conditioner towers against the float64 oracle (tests/cond_token_refs.py), and the towers' exact invariants.

The whole-tensor gates of test_clip_gpu.py / test_vit_gpu.py (rel-L2 < 2e-2 against an fp32 golden, every tok_stride-th patch token)
cannot see one token wrong by a few percent, a LayerScale ignored, positional rows shifted by a patch or a quick-GELU constant off by
6 % (tests/test_cond_tokens_cpu.py plants each); here every group a tower's forward returns is held to

    rho_t = ||y_hip - y16||_t / max(||y16 - y64||_t, 0.1 median)  <=  CAP

with y64 the float64 oracle and y16 the float64 oracle with the kernels' arithmetic (oracle.dit.operand_rounding(bf16,
kernel_arith=True)), at the shapes where the launch changes: one / two key blocks of the causal kernel, a token past a 64-key tile,
the production sequences, the block GEMMs on both sides of the 128x128 tile (M = 1536), registers on and off, both activations,
Dh 64 and 128.  The invariants below them are exact (torch.equal): what a tower must not depend on.
"""
import pytest
import torch

import cond_token_refs as R
from ln3diff_amd.synth import synth_input
from oracle import clip_text as oclip

pytestmark = pytest.mark.gpu

# CAP: the project's rule (test_dit_tokens_gpu.py) - twice the worst measured rho, rounded up to one digit, never above 1.0.
# measured: worst rho of every case (over its parts) on gfx950 (MI355X), tile choice left to the library
MEASURED = {
    'text-eos999': 0.482, 'text-legacy': 0.682, 'text-T64': 0.600, 'text-T65': 0.338, 'text-T33': 0.890, 'text-T128': 0.647, 'text-B20': 0.823,
    'openclip-S56': 0.376, 'openclip-S112': 0.856, 'openclip-S224': 0.657, 'openclip-S224-B6': 0.821, 'openclip-erf': 0.618,
    'dino-S56': 0.218, 'dino-S112': 0.666, 'dino-S224': 0.532, 'dino-S224-B6': 0.603, 'dino-R0': 0.211, 'dino-Dh128': 0.330,
    'mv-S56': 0.565, 'mv-S224-B1': 0.573, 'mv-S224-B2': 0.607,
}
# Twice the worst (0.890, text-T33) is 1.8, so the ceiling decides: CAP = 1.0, one cap for all towers.  The OpenCLIP cases' worst is
# their pooled vector (one group per sample: 0.38 .. 0.86; their patch tokens 0.33 .. 0.49).  No case needed a rounding point beyond
# what operand_rounding(kernel_arith=True) names: the single-pass causal softmax of the short-sequence kernel was added to it with
# these tests, the quick-GELU stays exact (oracle.dit.quick_gelu).  No invariant failed and no kernel was found wrong; the one change
# to shipped code is that FrozenCLIPEmbedder.forward refuses a head size other than 64, more than 128 tokens or more tokens than
# position rows before any launch (it used to assert Dh in (64, 128) and fail inside the third kernel, or read past the table).
CAP = 1.0
assert set(MEASURED) == set(R.CASE_IDS) and CAP <= 1.0


# ------------------------------------------------------------------------------------------------ running a tower
def _run(cs, m=None, **inp):
    """forward of the case's tower on the device with `inp` replacing the case's inputs -> what forward returns, on the CPU"""
    m = R.load_tower(cs) if m is None else m
    x = {k: v.cuda() for k, v in dict(R.inputs(cs), **inp).items()}
    if cs['tower'] == 'text':
        out = m(x['ids'])
    elif cs['tower'] == 'mv':
        from ln3diff_amd.sgm.image_encoders import MV23DConditioner
        out = MV23DConditioner(m)(x)
        assert set(out) == {'concat'}
        out = out['concat']
    else:
        m.preprocess = lambda img: img                       # the case's image is the tower's input (as test_vit_gpu.py does)
        out = m(x['img'])
    return out.cpu() if torch.is_tensor(out) else tuple(o.cpu() for o in out)


def _check(cid, out):
    c = R.case(cid)
    res = R.judge(cid, R.parts(c, out))
    want = {'tokens': c['ntok'], 'last': c['ntok'], 'pooled': c['B']}
    worst_all = 0.0
    for part, (rho, d) in res.items():
        assert rho.numel() == want[part], (cid, part, rho.numel(), want[part])                  # every token, none left out
        where, worst = R.worst_token(rho)
        print(f"{cid} [{part}]: worst token (sample, group) = ({where[0]}, {where[2]}), rho = {worst:.3f}; median rho {float(rho.median()):.3f}; "
              f"d median {float(d.median()):.3e} (measured: worst of the case {MEASURED[cid]})")
        assert torch.isfinite(rho).all(), (cid, part)
        worst_all = max(worst_all, worst)
    assert worst_all <= CAP, (cid, worst_all)


@pytest.mark.parametrize("cid", R.TOWER_IDS['text'])
def test_text_tower_every_token(hip_lib, cid):
    c = R.case(cid)
    last, pooled = _run(c)
    assert last.dtype == torch.float32 and tuple(last.shape) == (c['B'], c['T'], c['width'])
    _check(cid, (last, pooled))
    # pooling, both EOS rules: bit-identical to the final-LN state at the sample's own position
    pos = oclip.eos_positions(c['ids'], c['kw']['eos_token_id'])
    assert torch.equal(pos, c['eos_pos'])
    assert torch.equal(pooled, last[torch.arange(c['B']), pos]), cid


@pytest.mark.parametrize("cid", R.TOWER_IDS['openclip'])
def test_openclip_tower_every_token(hip_lib, cid):
    c = R.case(cid)
    tokens, pooled = _run(c)
    assert tuple(tokens.shape) == (c['B'], c['Lp'], c['width']) and tuple(pooled.shape) == (c['B'], R.CLIP_EMBED)
    _check(cid, (tokens, pooled))


@pytest.mark.parametrize("cid", R.TOWER_IDS['dino'])
def test_dinov2_tower_every_token(hip_lib, cid):
    c = R.case(cid)
    m = R.load_tower(c)
    assert (m._spec()['reg'] is None) == (c['R'] == 0)                                           # the reg=None path of vit_assemble
    cls, tokens = _run(c, m)
    assert tuple(cls.shape) == (c['B'], c['width']) and tuple(tokens.shape) == (c['B'], c['Lp'], c['width'])
    _check(cid, (cls, tokens))


@pytest.mark.parametrize("cid", R.TOWER_IDS['mv'])
def test_mv_plucker_tower_every_token(hip_lib, cid):
    c = R.case(cid)
    m = R.load_tower(c)
    assert m.state_dict()['model.patch_embed.proj.weight'].shape[1] == 9 and c['img'].shape[1] > c['V']
    tok = _run(c, m)
    assert tuple(tok.shape) == (c['B'], c['V'], c['Lp'], c['width'])
    _check(cid, tok)


# ------------------------------------------------------------------------------------------------ exact invariants
def _other_ids(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 900, tuple(c['ids'].shape), generator=g)


def test_text_tower_is_causal(hip_lib):
    """Replacing every id behind position j leaves last[:, :j + 1] bit-identical: a masked probability is exactly 0 and a GEMM row
    depends on its own row only.  j on both sides of the 32-query tile and the 64-key block."""
    c = R.case('text-eos999')
    m = R.load_tower(c)
    last, _ = _run(c, m)
    other = _other_ids(c, 5)
    for j in (0, 31, 32, 63, 64):
        ids = c['ids'].clone()
        ids[:, j + 1:] = other[:, j + 1:]
        assert not torch.equal(ids, c['ids'])
        last2, _ = _run(c, m, ids=ids)
        assert torch.equal(last2[:, :j + 1], last[:, :j + 1]), j
        assert not torch.equal(last2[:, j + 1:], last[:, j + 1:]), j


def _sample(out, b):
    """sample b of everything a forward returned"""
    return [o[b] for o in ((out,) if torch.is_tensor(out) else out)]


@pytest.mark.parametrize("cid", ['text-eos999', 'text-B20', 'openclip-S56', 'openclip-S224-B6', 'dino-S56', 'dino-S224-B6', 'mv-S56', 'mv-S224-B2'])
def test_sample_does_not_depend_on_its_batch_neighbours(hip_lib, cid):
    """With B fixed, replacing samples 1 .. B-1 leaves sample 0's output bit-identical - for every tower once below and once above
    M = 1536, where the GEMM tiles straddle sample boundaries."""
    c = R.case(cid)
    assert c['ring_gemm'] == (cid in ('text-B20', 'openclip-S224-B6', 'dino-S224-B6', 'mv-S224-B2')) and c['B'] > 1
    m = R.load_tower(c)
    a = _run(c, m)
    if c['tower'] == 'text':
        ids = c['ids'].clone()
        ids[1:] = _other_ids(c, 9)[1:]
        new = dict(ids=ids)
    else:
        img = c['img'].clone()
        img[1:] = synth_input('other', tuple(img.shape), 11)[1:].clamp(-1, 1)
        new = dict(img=img)
        if c['tower'] == 'mv':
            cams = c['cams'].clone()
            cams[1:] = c['cams'][:-1].flip(1)
            new['c'] = cams
    b = _run(c, m, **new)
    for x, y in zip(_sample(a, 0), _sample(b, 0)):
        assert torch.equal(x, y), cid
    assert not any(torch.equal(x, y) for x, y in zip(_sample(a, -1), _sample(b, -1)))             # the replaced samples did change


def test_mv_unused_views_do_not_matter(hip_lib):
    """views at index >= n_cond_frames, and their cameras, do not change the output"""
    c = R.case('mv-S56')
    m = R.load_tower(c)
    a = _run(c, m)
    img, cams = c['img'].clone(), c['cams'].clone()
    img[:, c['V']:] = synth_input('other', tuple(img.shape), 13)[:, c['V']:].clamp(-1, 1)
    cams[:, c['V']:] = cams[:, :1]
    assert torch.equal(_run(c, m, img=img, c=cams), a)
    img[:, 0] = img[:, c['V']]                                                                   # ... and a used one does
    assert not torch.equal(_run(c, m, img=img, c=cams), a)


def test_openclip_pooled_is_the_same_in_every_output_form(hip_lib):
    c = R.case('openclip-S56')
    _, pooled = _run(c)
    z = _run(c, R.load_tower(c, output_tokens=False))
    assert torch.is_tensor(z) and torch.equal(z, pooled)
    z = _run(c, R.load_tower(c, output_tokens=False, unsqueeze_dim=True))
    assert tuple(z.shape) == (c['B'], 1, R.CLIP_EMBED) and torch.equal(z[:, 0], pooled)
    _, z = _run(c, R.load_tower(c, unsqueeze_dim=True))
    assert torch.equal(z[:, 0], pooled)


def test_text_tower_refuses_what_the_causal_kernel_does_not_serve(hip_lib):
    """A Dh-128 text tower (width 256, 2 heads) constructs, but the causal kernel is Dh 64 only: forward raises before any launch
    and names the limit.  The same for more tokens than the kernel's 128 keys or than the position table has rows."""
    c = R.case('text-T128')
    ids = c['ids']
    with pytest.raises(ValueError, match='got head size 128'):
        R.load_tower(c, hidden_size=256)(ids.cuda())
    with pytest.raises(ValueError, match='and 129 tokens'):
        R.load_tower(c, max_position_embeddings=256)(torch.cat([ids, ids[:, :1]], 1).cuda())
    with pytest.raises(ValueError, match='has 77 rows.*and 78 tokens'):
        R.load_tower(c, max_position_embeddings=77)(ids[:, :78].cuda())
