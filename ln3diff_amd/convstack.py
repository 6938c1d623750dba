"""The LDM-style conv stack shared by the Objaverse VAE decoder (vit/vit_triplane.py), the multi-view VAE encoder (vit/mv_encoder.py)
and the U-Net denoiser (guided_diffusion/unet.py): weight packing and the launch sequence of each building block, on channel-last
activations ([N*H*W, C] f32 stream, bf16 GEMM operands, fp32 accumulation / norms / softmax).  The models keep their module trees,
their walk over them and their forward order; the pieces are here, once:

  conv 3x3        ln3d_im2col3x3 (nearest-2x upsample fused) / ln3d_im2col3x3_strided (stride 2, padding 1) / ln3d_im2col3x3_pad01
                  (pad (0,1,0,1), stride 2, padding 0) -> ln3d_gemm_bf16 (+ bias / + residual epilogue)
  GroupNorm(32)   ln3d_groupnorm_swish (stats + apply, widths dividing 256) or ln3d_groupnorm_any (any width; the ResBlock's `h + emb`
                  row or its scale / shift modulation folded in); one of the two per runner
  ResnetBlock     GN + swish -> conv -> [emb Linear] -> GN + swish -> conv with the residual epilogue onto x (a 1x1 GEMM of x first when
                  the width changes)
  self-attention  fused q|k|v GEMM, then ln3d_attention_bf16 (MFMA; heads zero-padded to 64 / 80 / 128, the output projection padded to
                  match) for >= MFMA_MIN_TOKENS tokens, ln3d_attention_small below
  transformer     GroupNorm -> proj_in GEMM -> per block: LayerNorm (ln3d_norm_modulate) -> self-attention -> to_out (residual epilogue);
                  LayerNorm -> the model's second attention -> to_out; LayerNorm -> GEGLU (GEMM + ln3d_geglu) -> GEMM; proj_out onto h
"""
import types

import torch

from . import ops
from .dit.dit_models_xformers import Workspace, bf16, f32, pad_head_columns, self_attention_hip

MFMA_MIN_TOKENS = 256           # self-attention over at least this many tokens goes to the MFMA attention kernels


def mfma_head(dh):
    """Head sizes the MFMA route takes: a multiple of 8 (the head-split GEMM epilogue) up to the attention kernels' 128."""
    return dh % 8 == 0 and dh <= 128


# ----------------------------------------------------------------------------- packing
def pack_conv3(conv, dev, cin_pad=None):
    w = conv.weight.detach().float().cpu()                    # [Cout, Cin, 3, 3] -> [Cout, (ky, kx, c)] with c padded to cin_pad
    co, ci = w.shape[0], w.shape[1]
    cp = cin_pad or ci
    kpad = (9 * cp + 63) // 64 * 64
    m = torch.zeros(co, 9, cp)
    m[:, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, 9, ci)
    full = torch.zeros(co, kpad)
    full[:, :9 * cp] = m.reshape(co, 9 * cp)
    return {'w': bf16(full, dev), 'b': f32(conv.bias, dev), 'kpad': kpad, 'cin': cp, 'cout': co}


def pack_lin(w, b, dev):
    w2 = w.detach().reshape(w.shape[0], -1)
    return {'w': bf16(w2, dev), 'b': None if b is None else f32(b, dev), 'cout': w2.shape[0], 'cin': w2.shape[1]}


def pack_gn(norm, dev, eps=None):
    """eps: for containers that carry none."""
    return (f32(norm.weight, dev), f32(norm.bias, dev), float(norm.eps if eps is None else eps))


def pack_ln(norm, dev):
    return (f32(norm.weight - 1.0, dev), f32(norm.bias, dev), float(norm.eps))           # y = LN(x) (1 + (w - 1)) + b


def pack_lin_any(w, b, dev):
    """pack_lin for any input width (a multiple of 8).  ln3d_gemm_bf16 steps K by 64: a linear / 1x1 whose input width is no multiple of
    64 is packed as the centre tap of a 3x3 (K = 9 cin, padded; it carries 'kpad') and runs on the im2col of its input - ConvStack.lin."""
    q = pack_lin(w, b, dev)
    if q['cin'] % 64:
        w3 = torch.zeros(q['cout'], q['cin'], 3, 3)
        w3[:, :, 1, 1] = w.detach().float().cpu().reshape(q['cout'], q['cin'])
        q = pack_conv3(types.SimpleNamespace(weight=w3, bias=b), dev)
    return q


def pack_resblock(n1, c1, n2, c2, dev, shortcut=None, eps=None):
    q = {'n1': pack_gn(n1, dev, eps), 'c1': pack_conv3(c1, dev), 'n2': pack_gn(n2, dev, eps), 'c2': pack_conv3(c2, dev)}
    if shortcut is not None:
        q['skip'] = pack_lin_any(shortcut.weight, shortcut.bias, dev)
    return q


def pack_out_proj(w, b, heads, dh, dev):
    """An attention's output projection as (plain, padded): the padded copy has zero columns where the MFMA route's output has its zero-
    padded head dims (None for head sizes that route never takes)."""
    plain, w2 = pack_lin_any(w, b, dev), w.detach().reshape(w.shape[0], -1)
    if not mfma_head(dh):
        return plain, None
    wp = pad_head_columns(w2, heads, dh)
    return plain, plain if wp is w2 else pack_lin_any(wp, b, dev)   # 64 / 72 / 80 / 128: nothing to pad, one copy serves both routes


def pack_transformer_block(b, heads, dh, cross, dev):
    """cross: attn2 attends to a context (q2 / kv2); otherwise to the block's own tokens (qkv2)."""
    qkv = lambda at: pack_lin(torch.cat([at.to_q.weight, at.to_k.weight, at.to_v.weight], 0), None, dev)
    q = {'n1': pack_ln(b.norm1, dev), 'n2': pack_ln(b.norm2, dev), 'n3': pack_ln(b.norm3, dev), 'qkv1': qkv(b.attn1),
         'ff1': pack_lin(b.ff.net[0].proj.weight, b.ff.net[0].proj.bias, dev), 'ff2': pack_lin(b.ff.net[2].weight, b.ff.net[2].bias, dev)}
    q['o1'], q['o1p'] = pack_out_proj(b.attn1.to_out[0].weight, b.attn1.to_out[0].bias, heads, dh, dev)
    if cross:
        q['q2'] = pack_lin(b.attn2.to_q.weight, None, dev)
        q['kv2'] = pack_lin(torch.cat([b.attn2.to_k.weight, b.attn2.to_v.weight], 0), None, dev)
        q['o2'] = pack_lin(b.attn2.to_out[0].weight, b.attn2.to_out[0].bias, dev)
    else:
        q['qkv2'] = qkv(b.attn2)
        q['o2'], q['o2p'] = pack_out_proj(b.attn2.to_out[0].weight, b.attn2.to_out[0].bias, heads, dh, dev)
    return q


def pack_transformer(m, cross, dev):
    """SpatialTransformer / SpatialTransformer3D: norm, proj_in, transformer_blocks, proj_out."""
    return {'n': pack_gn(m.norm, dev), 'pin': pack_lin(m.proj_in.weight, m.proj_in.bias, dev),
            'pout': pack_lin(m.proj_out.weight, m.proj_out.bias, dev), 'heads': m.n_heads, 'dh': m.d_head,
            'blocks': [pack_transformer_block(b, m.n_heads, m.d_head, cross, dev) for b in m.transformer_blocks]}


def empty_alloc(dev):
    """The allocator of the models that keep no scratch between forwards: a new tensor per request, whatever its name."""
    return lambda name, shape, dtype: torch.empty(shape, device=dev, dtype=dtype)


# ----------------------------------------------------------------------------- the runner
class ConvStack:
    """Launches the blocks above.  alloc(name, shape, dtype) provides every scratch and result tensor: a Workspace.get keeps one tensor
    per (name, shape) and reuses it, so the names below are chosen for their live ranges; empty_alloc ignores them.  gn_any: GroupNorm by
    ln3d_groupnorm_any instead of ln3d_groupnorm_swish.  h, x: f32 [N*H*W, C]; a_bf: bf16."""

    def __init__(self, dev, alloc, ws=None, gn_any=False, who='conv stack'):
        self.alloc, self.gn_any, self.who = alloc, gn_any, who    # who: the model's name in error messages
        self.ws = Workspace(dev) if ws is None else ws    # zero-initialised padded q / k / V^T of the MFMA attention route

    def bf(self, h, name='bf'):
        y = self.alloc(name, h.shape, torch.bfloat16)
        ops.cast_bf16(h, y)
        return y

    def gn(self, h, nw, N, HW, C, swish, add_row=None, mod=None):
        y = self.alloc('gn', (N * HW, C), torch.bfloat16)
        if self.gn_any:
            ops.groupnorm_any(h, nw[0], nw[1], y, N, HW, C, 32, nw[2], swish, add_row=add_row,
                              mod_scale=None if mod is None else mod[0], mod_shift=None if mod is None else mod[1])
        else:
            assert add_row is None and mod is None, "ln3d_groupnorm_swish takes no embedding row / modulation"
            st = self.alloc('gn_stats', (N * 64 * (1 + (HW + 255) // 256),), torch.float32)     # sums + per-chunk partials (ln3d.h)
            ops.groupnorm_swish(h, nw[0], nw[1], y, st, N, HW, C, 32, nw[2], swish)
        return y

    def conv3(self, a_bf, N, H, W, pc, out, up=1, stride=1, pad01=False, epi=ops.EPI_F32):
        """pad01: the ldm Downsample (pad (0,1,0,1), stride 2, padding 0).  -> (Ho, Wo)"""
        if pad01:
            Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        elif stride == 1:
            Ho, Wo = H * up, W * up
        else:
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        col = self.alloc('col', (N * Ho * Wo, pc['kpad']), torch.bfloat16)
        if pad01:
            ops.im2col3x3_pad01(a_bf, col, N, H, W, pc['cin'], pc['kpad'])
        elif stride == 1:
            ops.im2col3x3(a_bf, col, N, H, W, pc['cin'], up, pc['kpad'])
        else:
            ops.im2col3x3_strided(a_bf, col, N, H, W, pc['cin'], stride, pc['kpad'])
        ops.gemm(col, pc['w'], pc['b'], epi, out)
        return Ho, Wo

    def kcols(self, a_bf, pl):
        """the GEMM operand of a linear packed by pack_lin_any: a_bf itself, or (input width no multiple of 64) its rows as one-pixel
        images through im2col - the centre tap, the other eight taps and the tail zero"""
        if 'kpad' not in pl:
            return a_bf
        col = self.alloc('col', (a_bf.shape[0], pl['kpad']), torch.bfloat16)
        ops.im2col3x3(a_bf, col, a_bf.shape[0], 1, 1, pl['cin'], 1, pl['kpad'])
        return col

    def lin(self, a_bf, pl, epi, out):
        """out = (EPI_GATE_RES: out +=) a_bf @ w^T + b for pl = pack_lin_any(w, b)"""
        ops.gemm(self.kcols(a_bf, pl), pl['w'], pl['b'], epi, out)

    def res(self, x, q, N, H, W, emb_silu=None, in_place=True):
        """One ResnetBlock.  in_place: the residual lands on x when no shortcut GEMM makes a new tensor (False: x is needed again)."""
        cin, cout, HW = q['c1']['cin'], q['c1']['cout'], H * W
        a = self.gn(x, q['n1'], N, HW, cin, True)
        t = self.alloc('res_t', (N * HW, cout), torch.float32)
        self.conv3(a, N, H, W, q['c1'], t)
        if 'emb' in q:
            e = self.alloc('res_emb', (N, q['emb']['cout']), torch.float32)
            ops.gemm(emb_silu, q['emb']['w'], q['emb']['b'], ops.EPI_F32, e)
            if q['ss']:                                   # GN(h) * (1 + scale) + shift, then SiLU (unet.py:267-271)
                a2 = self.gn(t, q['n2'], N, HW, cout, True, mod=(e[:, :cout].contiguous(), e[:, cout:].contiguous()))
            else:                                         # SiLU(GN(h + emb)) (unet.py:272-273)
                a2 = self.gn(t, q['n2'], N, HW, cout, True, add_row=e)
        else:
            a2 = self.gn(t, q['n2'], N, HW, cout, True)
        if 'skip' in q:
            xb = self.bf(x, 'res_xb')
            s = self.alloc(f'res_x{cout}_{HW}', (N * HW, cout), torch.float32)
            if 'kpad' in q['skip']:
                self.conv3(xb, N, H, W, q['skip'], s)
            else:
                ops.gemm(xb, q['skip']['w'], q['skip']['b'], ops.EPI_F32, s)
        else:
            s = x if in_place else x.clone()
        self.conv3(a2, N, H, W, q['c2'], s, epi=ops.EPI_GATE_RES)
        return s

    def self_attend(self, a_bf, q_qkv, B, L, heads, dh, tag):
        """Self-attention of B sequences of L tokens (rows of a_bf in sequence order) -> (bf16 [B*L, heads * head width], padded).
        padded: the MFMA route ran and the head width is attn_out_dim(dh): multiply by the padded output projection."""
        inner = heads * dh
        a_bf = self.kcols(a_bf, q_qkv)
        if mfma_head(dh) and L >= MFMA_MIN_TOKENS and L % 32 == 0:
            # the fused q|k|v GEMM splits heads in its epilogue (q / k [B, H, L, Dp], V^T [B, H, Dp, L], head size zero-padded: exact, the
            # pad contributes 0 to q.k and meets zero columns of the padded projection); the scratch is keyed by dh because two head
            # sizes that pad to the same Dp must not see each other's columns
            return self_attention_hip(self.ws, '%s%d_' % (tag, dh), a_bf, B, L, inner, heads, q_qkv['w'], q_qkv['b']), True
        if L > 1024:
            raise ValueError(f"{self.who}: {L} tokens per sequence need the MFMA attention kernels (a multiple of 32, head size "
                             f"a multiple of 8 up to 128); got head size {dh}")
        y = self.alloc('qkv', (B * L, 3 * inner), torch.bfloat16)
        ops.gemm(a_bf, q_qkv['w'], q_qkv['b'], ops.EPI_BF16, y)
        o = self.alloc('attn_o', (B * L, inner), torch.bfloat16)
        ops.attention_small(y, y[:, inner:], y[:, 2 * inner:], o, B, heads, L, L, dh, 3 * inner, 3 * inner, 3 * inner, dh ** -0.5)
        return o, False

    def geglu_ff(self, a_bf, b, rows, tok):
        """tok += ff2(GEGLU(ff1(a_bf)))"""
        wide = b['ff1']['cout']
        g = self.alloc('ff_g', (rows, wide), torch.float32)
        ops.gemm(a_bf, b['ff1']['w'], b['ff1']['b'], ops.EPI_F32, g)
        gg = self.alloc('ff_gg', (rows, wide // 2), torch.bfloat16)
        ops.geglu(g, gg, rows, wide // 2)
        ops.gemm(gg, b['ff2']['w'], b['ff2']['b'], ops.EPI_GATE_RES, tok)

    def transformer(self, h, q, N, H, W, second, frames=1, in_place=True):
        """attn1 attends over the `frames` consecutive images of an object jointly: rows are (object, frame, pixel), so
        `(b f) l c -> b (f l) c` is a view.  second(a_bf, b) -> (attention output, packed output projection) is the model's attn2."""
        HW, C = H * W, h.shape[1]
        heads, dh = q['heads'], q['dh']
        inner, rows = heads * dh, N * HW
        a = self.gn(h, q['n'], N, HW, C, False)
        tok = self.alloc('tok', (rows, inner), torch.float32)
        ops.gemm(a, q['pin']['w'], q['pin']['b'], ops.EPI_F32, tok)
        for b in q['blocks']:
            def ln(nw):
                y = self.alloc('ln', (rows, inner), torch.bfloat16)
                ops.norm_modulate(tok, y, rows, inner, kind=0, eps=nw[2], shift=nw[1], scale=nw[0], mod_rows=rows, mod_ld=0)
                return y
            o, padded = self.self_attend(ln(b['n1']), b['qkv1'], N // frames, frames * HW, heads, dh, 'j%d_' % frames)
            proj = b['o1p' if padded else 'o1']
            ops.gemm(o, proj['w'], proj['b'], ops.EPI_GATE_RES, tok)
            o, proj = second(ln(b['n2']), b)
            ops.gemm(o, proj['w'], proj['b'], ops.EPI_GATE_RES, tok)
            self.geglu_ff(ln(b['n3']), b, rows, tok)
        s = h if in_place else h.clone()
        ops.gemm(self.bf(tok), q['pout']['w'], q['pout']['b'], ops.EPI_GATE_RES, s)
        return s
