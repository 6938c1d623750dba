"""CPU oracle (TEST INFRASTRUCTURE ONLY) - fp32 torch restatement of the reference's
DiT denoisers on the text/image->3D sampling path.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
The product path (ln3diff_amd/) never does: it runs the HIP kernels or fails loudly.

Pinned against the reference's own Python (run in the build container through
tests/golden/ref_shims.py) by tests/golden/make_golden.py; the committed vectors are
tests/golden/*.npz.  Third-party arithmetic the reference delegates to packages that
are absent from /root/reference (xformers 0.0.26 attention / FusedMLP, timm 0.6
PatchEmbed / Mlp) is restated from its published semantics - "parity unpinned"
against those packages themselves.

All functions take `sd`, a state-dict with the reference's parameter names, so the
same weights drive the reference module, this oracle and the HIP product modules.

Reference citations (relative to the reference checkout):
  timestep_embedding   dit/dit_models_xformers.py:101-127
  pos embed            dit/dit_models_xformers.py:961-1021, dit/dit_trilatent.py:51-66
  modulate             dit/dit_models_xformers.py:48-53
  self attention       vit/vision_transformer.py:108-124 (MemEffAttention)
  cross attention      ldm/modules/attention.py:278-307
  RMSNorm              dit/norm.py:27-40
  TextCondDiTBlock     dit/dit_models_xformers.py:306-323
  ImageCond..PixelArt  dit/dit_models_xformers.py:506-539
  FinalLayer/T2IFinal  dit/dit_models_xformers.py:655-678 / :61-84
  DiT_TriLatent.fwd    dit/dit_trilatent.py:74-143
  DiT_I23D_PixelArt    dit/dit_i23d.py:229-291, forward_with_cfg :155-168
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

DIT_CONFIGS = {
    # arch: (hidden, depth, heads)   reference dit/dit_trilatent.py:272-293
    "DiT-B/2": (768, 12, 12),
    "DiT-L/2": (1024, 24, 16),
    "DiT-XL/2": (1152, 28, 16),
    "DiT-B/1": (768, 12, 12),        # patch size 1 (pass patch=1 to t23d_forward)
}


# ------------------------------------------------------------------ embeddings
def timestep_embedding(t, dim=256, max_period=10000.0):
    # The frequency table and the argument t * freq are fp32 BY DEFINITION (the reference builds them in fp32, and so does the HIP
    # kernel): at t ~ 1000 an argument carries an absolute fp32 error of ~1e-4, which a float64 table would not reproduce - so in
    # float64 mode too the fp32 argument is what enters cos / sin.
    half = dim // 2
    t = _fp(t)
    freqs = torch.exp(-math.log(max_period) *
                      torch.arange(half, dtype=torch.float32) / half)
    args = (t[:, None].float() * freqs[None]).to(t.dtype)
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def _sincos_1d(embed_dim, pos):
    omega = np.arange(embed_dim // 2, dtype=np.float64)
    omega /= embed_dim / 2.
    omega = 1. / 10000 ** omega
    out = np.einsum('m,d->md', pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_pos_embed_2d(embed_dim, grid_hw):
    """get_2d_sincos_pos_embed with a (h, w) tuple: first half of the channels encodes
    grid[0] (the w-index, 'w goes first'), second half grid[1] (the h-index)."""
    gh, gw = grid_hw
    grid_h = np.arange(gh, dtype=np.float32)
    grid_w = np.arange(gw, dtype=np.float32)
    grid = np.stack(np.meshgrid(grid_w, grid_h), axis=0).reshape(2, 1, gh, gw)
    emb_h = _sincos_1d(embed_dim // 2, grid[0])
    emb_w = _sincos_1d(embed_dim // 2, grid[1])
    return np.concatenate([emb_h, emb_w], axis=1)


def trilatent_pos_embed(D, plane_n=3, tokens_per_plane=256):
    """init_PE_3D_aware: grid (plane_n, p*p)."""
    pe = sincos_pos_embed_2d(D, (plane_n, tokens_per_plane))
    return torch.from_numpy(pe).float().reshape(1, plane_n * tokens_per_plane, D)


# ----------------------------------------------------------------- primitives
# Operand-rounding emulation (test infrastructure for the precision argument of DESIGN.md): with OPERAND_ROUND[0] = torch.bfloat16
# every GEMM operand (activations, weights, attention q/k/v and probabilities) is rounded to bf16 and the product accumulated
# in fp32 - the arithmetic of the HIP path's MFMA kernels.  The HIP forward must agree with THIS restatement an order of
# magnitude more tightly than with the fp32 one; what is left is accumulation order and rounding-boundary flips.
#
# Working precision: every function on the denoiser forward paths keeps the dtype of `sd` and the inputs, so a state dict and inputs
# cast to torch.float64 run in float64 end to end, with and without operand rounding (the rounding then is float64 -> bf16 -> float64:
# the bf16-operand restatement without any fp32 noise of its own; "fp32 accumulation" becomes float64 accumulation).  fp32 in, the
# arithmetic is what it always was.  tests/dit_token_refs.py builds its per-token yardstick on this.
OPERAND_ROUND = [None]


def _fp(x):
    """the working-precision view of an input: fp32 / float64 stay, anything else (integer timesteps, half inputs) becomes fp32"""
    return x if x.dtype in (torch.float32, torch.float64) else x.float()


KERNEL_ARITH = [False]
UNFUSED_NORMS = [frozenset()]


class operand_rounding:
    """with operand_rounding(torch.bfloat16): every GEMM / attention operand is rounded to that dtype (see above).

    kernel_arith=True (opt-in; the per-token tests of tests/dit_token_refs.py) additionally restates WHERE the attention kernels
    round inside the softmax - rounding points the plain mode leaves out or places elsewhere, each of which moves a token by a
    quarter of what all operand rounding together does - and the one function the kernels do not evaluate to fp32 accuracy:
      * the erf-GELU of the MLP's fc1 epilogue is gelu_erf2 of csrc/common.h: erf(x / sqrt 2) = u P(u^2), u = x clamped to
        +-3.9985, P a degree-7 polynomial; within 1.3e-4 ABSOLUTE of the exact GELU, which for |gelu(x)| < 0.03 is more than the bf16
        rounding of the value (gelu_erf_kernel below; measured: with the exact erf instead, a block's output is 0.05 of its operand
        rounding away from the HIP block, with the polynomial 0.001);
      * q is stored in bf16 by the QKV / query projection and the scale is applied afterwards: to the fp32 scores (the ring kernel
        attn_kernel, the cross-attention epilogue of the query projection), or - the streaming kernel, Dh 64 with a multiple of 256
        keys - to q itself, q * scale * log2(e) ROUNDED TO bf16 ONCE MORE (attention.hip read_q);
      * the un-normalised probabilities are rounded as P = exp2(s - m) with the kernel's RUNNING reference m, not the row maximum:
        m is the row maximum of the first key tile (64 keys, streaming kernel 32) and is raised to max(m, tile maximum) for the 32
        queries of a wave when a tile of any of them outgrows it by more than 2^8 (the deferred re-base); bf16 rounding is not
        invariant under the factor 2^(m - max), so this decides which way each probability rounds.  The cross-attention that runs
        inside the query projection (LN3D_EPI_CROSS_ATTN, <= 96 keys) has all keys in one tile: m is the row maximum;
      * the causal attention of the CLIP text tower (sdpa(causal=True): attn_short_kernel, Dh 64, <= 128 keys) is a single pass over all
        keys like that epilogue: q stored bf16, the scale on the fp32 scores, m the row maximum over the UNMASKED keys, the row sum over
        the unrounded P, a masked P exactly 0 (tests/cond_token_refs.py);
      * a cross-attention k-norm runs as a pass of its own over the bf16 keys the K projection wrote (_cross_kv): k is rounded in
        front of the norm as well as behind it;
      * the U-Net's self-attention (oracle/unet.py attend) hands the MFMA kernels heads zero-padded to 64 / 80 / 128 with the scale of
        the TRUE head size (dit_models_xformers.self_attention_hip: scale=Dh ** -0.5, head_dim_pad=Dp): _sdpa_kernel(dh_true=...) takes
        the padded width for the kernel choice (32 / 40 / 48 -> 64 over a multiple of 256 keys is the streaming kernel) and the true
        one for the scale; below 256 tokens, at head sizes the MFMA route refuses and against a context it is attn_small_kernel
        (csrc/unet_ops.hip:120-153): q / k / v in bf16, the scale on the fp32 scores (:136), the probabilities NOT rounded (:142,
        :150), the output rounded to bf16 (:151).
    Not restated: the K-resident kernel (a head for every CU: none of the shapes these tests use), whose row sum is taken over the
    ROUNDED probabilities.

    unfused_norms (opt-in, a set of names): a qk-norm that does not run inside its projection's epilogue (the head-row GEMM tiles:
    >= 1536 rows, 64-wide heads) runs as a pass of its own over the bf16 heads the projection wrote, so its input is rounded in front
    of the norm as well as behind it.  Which norms run unfused depends on the launch, so the caller names them:
      'self_qk'     q and k of the whole self-attention sequence (head sizes other than 64);
      'appended_k'  k of the tokens appended to the self-attention sequence (the appended-token K / V cache of a prompt batch with
                    fewer than 1536 appended rows, DiT_I23D_PixelArt._appended_kv);
      'cross_q'     the cross-attention query (fewer than 1536 conditional token rows)."""

    def __init__(self, dtype=torch.bfloat16, kernel_arith=False, unfused_norms=()):
        self.dtype, self.kernel_arith, self.unfused_norms = dtype, kernel_arith, frozenset(unfused_norms)
        assert self.unfused_norms <= {'self_qk', 'appended_k', 'cross_q'}, unfused_norms

    def __enter__(self):
        self.prev, OPERAND_ROUND[0] = OPERAND_ROUND[0], self.dtype
        self.prev_ks, KERNEL_ARITH[0] = KERNEL_ARITH[0], self.kernel_arith
        self.prev_un, UNFUSED_NORMS[0] = UNFUSED_NORMS[0], self.unfused_norms

    def __exit__(self, *a):
        OPERAND_ROUND[0] = self.prev
        KERNEL_ARITH[0] = self.prev_ks
        UNFUSED_NORMS[0] = self.prev_un


def _r(x):
    return x if OPERAND_ROUND[0] is None or x is None else x.to(OPERAND_ROUND[0]).to(x.dtype)


def linear(x, w, b=None):
    return F.linear(_r(x), _r(w), b)


def layer_norm(x, eps=1e-6, w=None, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def rms_norm(x, w, eps=1e-5):
    var = _fp(x).pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(var + eps)
    return x * w if w is not None else x


def _causal_masked(s):
    """scores [.., Nq, Nk] with the keys behind each query (key > query) at -inf"""
    future = torch.ones(s.shape[-2], s.shape[-1], dtype=torch.bool, device=s.device).triu(1)
    return s.masked_fill(future, float('-inf'))


def sdpa(q, k, v, one_tile=False, causal=False):
    """q,k,v [B,H,N,Dh]: softmax(q k^T / sqrt(Dh)) v, no dropout; causal: query i sees keys 0..i (the CLIP text tower).  one_tile:
    the attention runs inside the query projection's epilogue (all keys in one tile); only the kernel_arith restatement looks at it."""
    if OPERAND_ROUND[0] is None:
        s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
        return torch.softmax(_causal_masked(s) if causal else s, dim=-1) @ v
    if KERNEL_ARITH[0]:
        return _sdpa_kernel(q, k, v, one_tile, causal)
    # the kernels' arithmetic: q pre-scaled then rounded, un-normalised probabilities rounded for the P.V product, fp32 row sum
    s = _r(q * (q.shape[-1] ** -0.5)) @ _r(k).transpose(-1, -2)
    if causal:
        s = _causal_masked(s)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return (_r(p) @ _r(v)) / p.sum(-1, keepdim=True)


def _sdpa_kernel(q, k, v, one_tile, causal=False, dh_true=None):
    """operand_rounding(kernel_arith=True): the softmax of attention.hip's ring / streaming kernels and of the cross-attention
    epilogue, key tile by key tile with their running reference (see operand_rounding).  Scores are in log2 units.  causal: the
    short-sequence kernel (attn_short_kernel: Dh 64, <= 128 keys) - one pass over all keys, so the one_tile form with the masked scores
    at -inf: the reference is the row maximum over the unmasked keys and a masked probability is exactly 0.  dh_true: the heads are
    zero-padded to the width the kernel runs at (the U-Net's 32 / 40 / 48 -> 64, 96 -> 128; self_attention_hip): the width handed in
    chooses the kernel, the true one is the scale's."""
    Dh, Nq, Nk = q.shape[-1], q.shape[-2], k.shape[-2]
    c = (dh_true or Dh) ** -0.5 * 1.4426950408889634
    if causal:
        assert Dh == 64 and Nk <= 128, "causal masking exists in the short-sequence kernel only (Dh 64, <= 128 keys)"
        one_tile = True
    stream = Dh == 64 and Nk % 256 == 0 and not one_tile
    if stream:
        s = _r(_r(q) * c) @ _r(k).transpose(-1, -2)
    else:
        s = (_r(q) @ _r(k).transpose(-1, -2)) * c
    if causal:
        s = _causal_masked(s)
    vr = _r(v)
    tile = Nk if one_tile else (32 if stream else 64)
    m, o, l = None, 0.0, 0.0
    for k0 in range(0, Nk, tile):
        st = s[..., k0:k0 + tile]
        mt = st.amax(-1, keepdim=True)
        if m is None:
            m = mt
        else:
            grow = F.pad(mt > m + 8.0, (0, 0, 0, (-Nq) % 32))                      # the vote of a wave: 32 consecutive queries
            grow = grow.reshape(*grow.shape[:-2], -1, 32).any(-1, keepdim=True).expand(*grow.shape[:-2], -1, 32)
            grow = grow.reshape(*grow.shape[:-2], -1, 1)[..., :Nq, :]
            m_new = torch.where(grow, torch.maximum(m, mt), m)
            a = torch.exp2(m - m_new)
            o, l, m = o * a, l * a, m_new
        p = torch.exp2(st - m)
        l = l + p.sum(-1, keepdim=True)
        o = o + _r(p) @ vr[..., k0:k0 + tile, :]
    return o / l


def self_attention(sd, p, x, H, n_own=None):
    """n_own: the leading tokens of the sequence that are the network's own (the rest was appended); only the 'appended_k' restatement
    of operand_rounding(unfused_norms=...) looks at it."""
    B, N, C = x.shape
    qkv = linear(x, sd[p + 'qkv.weight'], sd[p + 'qkv.bias']).reshape(B, N, 3, H, C // H)
    q, k, v = qkv.unbind(2)                                  # [B,N,H,Dh]
    if p + 'q_norm.weight' in sd:
        if 'self_qk' in UNFUSED_NORMS[0]:
            q, k = _r(q), _r(k)
        elif 'appended_k' in UNFUSED_NORMS[0] and n_own is not None:
            k = torch.cat([k[:, :n_own], _r(k[:, n_own:])], dim=1)
        q = rms_norm(q, sd[p + 'q_norm.weight'])
        k = rms_norm(k, sd[p + 'k_norm.weight'])
    o = sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2))
    o = o.transpose(1, 2).reshape(B, N, C)
    return linear(o, sd[p + 'proj.weight'], sd[p + 'proj.bias'])


def cross_attention(sd, p, x, ctx, H, dim_head=64, in_projection=False):
    """in_projection: the caller's forward runs this attention inside the query projection GEMM when the shape allows
    (DiT_TriLatent.forward: tokens % 192 == 0, heads * 64 % 256 == 0, <= 96 keys); it changes nothing but the restatement of the
    softmax's rounding under operand_rounding(kernel_arith=True)."""
    B = x.shape[0]
    q = linear(x, sd[p + 'to_q.weight'])
    k = linear(ctx, sd[p + 'to_k.weight'])
    v = linear(ctx, sd[p + 'to_v.weight'])
    sp = lambda t: t.reshape(B, t.shape[1], H, dim_head).transpose(1, 2)
    q, k, v = sp(q), sp(k), sp(v)
    if p + 'q_norm.weight' in sd:
        q = rms_norm(_r(q) if 'cross_q' in UNFUSED_NORMS[0] else q, sd[p + 'q_norm.weight'])
        k = rms_norm(_r(k) if KERNEL_ARITH[0] else k, sd[p + 'k_norm.weight'])
    one_tile = in_projection and x.shape[1] % 192 == 0 and (H * dim_head) % 256 == 0 and ctx.shape[1] <= 96
    o = sdpa(q, k, v, one_tile).transpose(1, 2).reshape(B, x.shape[1], H * dim_head)
    return linear(o, sd[p + 'to_out.0.weight'], sd[p + 'to_out.0.bias'])


_GELU_ERF_POLY = (-2.556055811e-09, 2.088922457e-07, -7.419432677e-06, 1.523832179e-04, -2.042111475e-03, 1.916284487e-02,
                  -1.321282834e-01, 7.976111174e-01)


def gelu_erf_kernel(x):
    """the erf-GELU as the GEMM epilogue evaluates it (csrc/common.h gelu_erf2), in x's dtype"""
    u = x.clamp(-3.9985, 3.9985)
    t = u * u
    poly = torch.full_like(t, _GELU_ERF_POLY[0])
    for c in _GELU_ERF_POLY[1:]:
        poly = poly * t + c
    hx = x * 0.5
    return hx * (u * poly) + hx


def quick_gelu(x):
    """x * sigmoid(1.702 x), the fc1 activation of the OpenAI CLIP towers.  Exact in every mode: common.h::quick_gelu
    (x / (1 + __expf(-1.702 x))) is within fp32 ulps of it and the epilogue rounds the value to bf16 right behind it, so it is not
    restated under kernel_arith (measured on the towers of tests/cond_token_refs.py: no case's rho needs it)."""
    return x * torch.sigmoid(1.702 * x)


def fused_mlp(sd, p, x):
    h = linear(x, sd[p + 'mlp.0.weight']) + sd[p + 'mlp.1.bias']
    h = gelu_erf_kernel(h) if OPERAND_ROUND[0] is not None and KERNEL_ARITH[0] else F.gelu(h)      # erf GELU
    return linear(h, sd[p + 'mlp.2.weight']) + sd[p + 'mlp.3.bias']


def caption_embedder(sd, p, c):
    h = linear(c, sd[p + 'y_proj.fc1.weight'], sd[p + 'y_proj.fc1.bias'])
    h = F.gelu(h, approximate='tanh')
    return linear(h, sd[p + 'y_proj.fc2.weight'], sd[p + 'y_proj.fc2.bias'])


def t_embedder(sd, t):
    h = linear(timestep_embedding(t), sd['t_embedder.mlp.0.weight'], sd['t_embedder.mlp.0.bias'])
    return linear(F.silu(h), sd['t_embedder.mlp.2.weight'], sd['t_embedder.mlp.2.bias'])


def patchify_embed(sd, x, patch=2):
    """'b (c n) h w -> (b n) c h w', shared conv patch-embed, '(b n) l c -> b (n l) c'."""
    B, C3, Hh, Ww = x.shape
    C = C3 // 3
    xp = x.reshape(B, C, 3, Hh, Ww).permute(0, 2, 1, 3, 4).reshape(B * 3, C, Hh, Ww)
    tok = F.conv2d(xp, sd['x_embedder.proj.weight'], sd['x_embedder.proj.bias'], stride=patch)
    D = tok.shape[1]
    tok = tok.flatten(2).transpose(1, 2)                      # [(b n), l, D]
    return tok.reshape(B, 3 * tok.shape[1], D)


def unpatchify_trilatent(y, B, patch, c_out):
    """[B, 3*l, p*p*c] -> [B, c*3, H, W] with channel index c*3+n."""
    l = y.shape[1] // 3
    h = w = int(l ** 0.5)
    y = y.reshape(B * 3, h, w, patch, patch, c_out)
    y = torch.einsum('nhwpqc->nchpwq', y).reshape(B * 3, c_out, h * patch, w * patch)
    y = y.reshape(B, 3, c_out, h * patch, w * patch).permute(0, 2, 1, 3, 4)
    return y.reshape(B, c_out * 3, h * patch, w * patch).contiguous()


# --------------------------------------------------------------------- T23D
def t23d_block(sd, p, x, t_emb, ctx, H):
    mod = linear(F.silu(t_emb), sd[p + 'adaLN_modulation.1.weight'], sd[p + 'adaLN_modulation.1.bias'])
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
    h = layer_norm(x) * (1 + sc_a[:, None]) + sh_a[:, None]
    x = x + g_a[:, None] * self_attention(sd, p + 'attn.', h, H)
    x = x + cross_attention(sd, p + 'cross_attn.', x, ctx, H, in_projection=True)
    h = layer_norm(x) * (1 + sc_m[:, None]) + sh_m[:, None]
    return x + g_m[:, None] * fused_mlp(sd, p + 'mlp.', h)


def t23d_forward(sd, x, timesteps, context, num_heads, patch=2, return_tokens=False):
    """DiT_TriLatent.forward with vit_blk=TextCondDiTBlock, FinalLayer."""
    if isinstance(context, dict):
        context = context['crossattn']
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    t_emb = t_embedder(sd, timesteps)
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    ctx = caption_embedder(sd, 'clip_text_proj.', context)
    for i in range(depth):
        h = t23d_block(sd, f'blocks.{i}.', h, t_emb, ctx, num_heads)
    if return_tokens:
        return h
    return t23d_final(sd, h, t_emb, patch)


def t23d_final(sd, h, t_emb, patch=2):
    """FinalLayer + unpatchify of the token tensor h [B, 3*l, D] (what t23d_forward(return_tokens=True) returns) with the timestep
    embedding t_emb [B, D]: token-local, one group of p*p*C output numbers per (sample, plane, patch)."""
    mod = linear(F.silu(t_emb), sd['final_layer.adaLN_modulation.1.weight'],
                   sd['final_layer.adaLN_modulation.1.bias'])
    shift, scale = mod.chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale[:, None]) + shift[:, None]
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])     # fp32 in the HIP path too (final_layer kernel)
    c_out = y.shape[-1] // (patch * patch)
    return _fp(unpatchify_trilatent(y, h.shape[0], patch, c_out))


def t23d_pixart_forward(sd, x, timesteps, context, num_heads, patch=2):
    """DiT_TriLatent_PixelArt.forward (dit/dit_trilatent.py:146-250; registry 'DiT-PixelArt-L/2' / '-B/2') with
    PixelArtTextCondDiTBlock (dit_models_xformers.py:326-369): t = t_embedder + cap_embedder(LN -> Linear)(context['vector']), ONE
    shared adaLN whose output is added to each block's scale_shift_table, RMSNorm (affine, eps 1e-5) pre-norms, self-attention without
    qk-norm, cross-attention (64-dim heads, no qk-norm) over the text tokens normalised by the BLOCK's attention_y_norm, T2IFinalLayer."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    vec = _fp(context['vector'])
    cls = linear(layer_norm(vec, 1e-5, sd['cap_embedder.0.weight'], sd['cap_embedder.0.bias']),
                 sd['cap_embedder.1.weight'], sd['cap_embedder.1.bias'])
    ctx = _fp(context['crossattn'])
    t = t_embedder(sd, _fp(timesteps)) + cls
    t0 = linear(F.silu(t), sd['adaLN_modulation.1.weight'], sd['adaLN_modulation.1.bias'])
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    for i in range(depth):
        p = f'blocks.{i}.'
        mod = sd[p + 'scale_shift_table'][None] + t0.reshape(B, 6, -1)
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
        h = h + g_a * self_attention(sd, p + 'attn.', rms_norm(h, sd[p + 'norm1.weight']) * (1 + sc_a) + sh_a, num_heads)
        h = h + cross_attention(sd, p + 'cross_attn.', h, rms_norm(ctx, sd[p + 'attention_y_norm.weight']), num_heads)
        h = h + g_m * fused_mlp(sd, p + 'mlp.', rms_norm(h, sd[p + 'norm2.weight']) * (1 + sc_m) + sh_m)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])
    c_out = y.shape[-1] // (patch * patch)
    return _fp(unpatchify_trilatent(y, B, patch, c_out))


# --------------------------------------------------------------------- I23D
def i23d_block(sd, p, x, t0, dino_tok, clip_tok, H):
    B, N, D = x.shape
    mod = sd[p + 'scale_shift_table'][None] + t0.reshape(B, 6, -1)
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)     # each [B,1,D]
    h = rms_norm(x, sd[p + 'norm1.weight']) * (1 + sc_a) + sh_a
    h = torch.cat([h, dino_tok], dim=1)
    x = x + g_a * self_attention(sd, p + 'attn.', h, H, n_own=N)[:, :N]
    x = x + cross_attention(sd, p + 'cross_attn.', x, clip_tok, H)
    h = rms_norm(x, sd[p + 'norm2.weight']) * (1 + sc_m) + sh_m
    return x + g_m * fused_mlp(sd, p + 'mlp.', h)


def i23d_forward(sd, x, timesteps, context, num_heads, patch=2, clip_ctx_dim=1024):
    """DiT_I23D_PixelArt.forward (ImageCondDiTBlockPixelArtRMSNorm blocks, T2IFinalLayer)."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    vec = _fp(context['vector'])
    cls = linear(layer_norm(vec, 1e-5, sd['cap_embedder.0.weight'], sd['cap_embedder.0.bias']),
                   sd['cap_embedder.1.weight'], sd['cap_embedder.1.bias'])
    ca = _fp(context['crossattn'])
    clip_tok = rms_norm(ca[..., :clip_ctx_dim], sd['attention_y_norm.weight'])
    dino_tok = caption_embedder(sd, 'dino_proj.', ca[..., clip_ctx_dim:])
    t = t_embedder(sd, _fp(timesteps)) + cls
    t0 = linear(F.silu(t), sd['adaLN_modulation.1.weight'], sd['adaLN_modulation.1.bias'])
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    for i in range(depth):
        h = i23d_block(sd, f'blocks.{i}.', h, t0, dino_tok, clip_tok, num_heads)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])     # fp32 in the HIP path too (final_layer kernel)
    c_out = y.shape[-1] // (patch * patch)
    return _fp(unpatchify_trilatent(y, B, patch, c_out))


def i23d_plain_block(sd, p, x, t_emb, dino_tok, clip_tok, H):
    """ImageCondDiTBlock.forward (dit/dit_models_xformers.py:450-476): the block's own adaLN, affine-free LayerNorm pre-norms,
    [modulated x ; DINO] self-attention, cross-attention over the block's attention_y_norm(CLIP tokens)."""
    N = x.shape[1]
    mod = linear(F.silu(t_emb), sd[p + 'adaLN_modulation.1.weight'], sd[p + 'adaLN_modulation.1.bias'])
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
    h = layer_norm(x) * (1 + sc_a[:, None]) + sh_a[:, None]
    h = torch.cat([h, dino_tok], dim=1)
    x = x + g_a[:, None] * self_attention(sd, p + 'attn.', h, H, n_own=N)[:, :N]
    x = x + cross_attention(sd, p + 'cross_attn.', x, rms_norm(clip_tok, sd[p + 'attention_y_norm.weight']), H)
    h = layer_norm(x) * (1 + sc_m[:, None]) + sh_m[:, None]
    return x + g_m[:, None] * fused_mlp(sd, p + 'mlp.', h)


def i23d_plain_forward(sd, x, timesteps, context, num_heads, patch=2, clip_ctx_dim=1024):
    """DiT_I23D.forward (dit/dit_i23d.py:96-153): t = t_embedder + clip_text_proj(context['vector']); T2IFinalLayer."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    ca = _fp(context['crossattn'])
    cls = caption_embedder(sd, 'clip_text_proj.', _fp(context['vector']))
    clip_tok, dino_tok = ca[..., :clip_ctx_dim], caption_embedder(sd, 'dino_proj.', ca[..., clip_ctx_dim:])
    t = t_embedder(sd, _fp(timesteps)) + cls
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    for i in range(depth):
        h = i23d_plain_block(sd, f'blocks.{i}.', h, t, dino_tok, clip_tok, num_heads)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])
    return _fp(unpatchify_trilatent(y, B, patch, y.shape[-1] // (patch * patch)))


def i23d_mv_forward(sd, x, timesteps, context, num_heads, patch=2):
    """DiT_I23D_PixelArt_MVCond.forward (dit/dit_i23d.py:293-384): multi-view image conditioning.  The projected CLIP spatial
    tokens (clip_spatial_proj) are the ones appended to the self-attention sequence and the flattened multi-view DINO features
    context['concat'] [B, V, L, C] are the cross-attention context, raw (no attention_y_norm, no projection); dino_proj is gone."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    vec = _fp(context['vector'])
    cls = linear(layer_norm(vec, 1e-5, sd['cap_embedder.0.weight'], sd['cap_embedder.0.bias']),
                   sd['cap_embedder.1.weight'], sd['cap_embedder.1.bias'])
    clip_tok = caption_embedder(sd, 'clip_spatial_proj.', _fp(context['crossattn']))
    mv = _fp(context['concat'])
    dino_tok = mv.reshape(B, mv.shape[1] * mv.shape[2], mv.shape[3])
    t = t_embedder(sd, _fp(timesteps)) + cls
    t0 = linear(F.silu(t), sd['adaLN_modulation.1.weight'], sd['adaLN_modulation.1.bias'])
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    for i in range(depth):
        h = i23d_block(sd, f'blocks.{i}.', h, t0, clip_tok, dino_tok, num_heads)       # (appended, cross-attended)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])     # fp32 in the HIP path too (final_layer kernel)
    c_out = y.shape[-1] // (patch * patch)
    return _fp(unpatchify_trilatent(y, B, patch, c_out))


def i23d_pcd_forward(sd, x, timesteps, context, num_heads):
    """DiT_pcd_I23D_PixelArt_MVCond.forward (dit/dit_i23d.py:500-588, registry key 'DiT-PixArt-MV-PCD-L'): the tokens are the
    points of a point-cloud latent x [B, N, C] - no patchify, no positional embedding; x_embedder is a timm Mlp
    (Linear -> tanh-GELU -> Linear); conditioning and blocks as MVCond; the output stays [B, N, out_channels]."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    vec = _fp(context['vector'])
    cls = linear(layer_norm(vec, 1e-5, sd['cap_embedder.0.weight'], sd['cap_embedder.0.bias']),
                 sd['cap_embedder.1.weight'], sd['cap_embedder.1.bias'])
    clip_tok = caption_embedder(sd, 'clip_spatial_proj.', _fp(context['crossattn']))
    mv = _fp(context['concat'])
    dino_tok = mv.reshape(B, mv.shape[1] * mv.shape[2], mv.shape[3])
    t = t_embedder(sd, _fp(timesteps)) + cls
    t0 = linear(F.silu(t), sd['adaLN_modulation.1.weight'], sd['adaLN_modulation.1.bias'])
    h = linear(_fp(x), sd['x_embedder.fc1.weight'], sd['x_embedder.fc1.bias'])
    h = linear(F.gelu(h, approximate='tanh'), sd['x_embedder.fc2.weight'], sd['x_embedder.fc2.bias'])
    for i in range(depth):
        h = i23d_block(sd, f'blocks.{i}.', h, t0, clip_tok, dino_tok, num_heads)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    return _fp(linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias']))


def i23d_mv_noclip_forward(sd, x, timesteps, context, num_heads, patch=2):
    """DiT_I23D_PixelArt_MVCond_noClip.forward (dit/dit_i23d.py:387-492, the class the reference registers as
    'DiT-PixArt-MV-L/2'): no CLIP branch at all - t = t_embedder(timesteps), nothing is appended to the self-attention
    sequence (ImageCondDiTBlockPixelArtNoclip, dit_models_xformers.py:540-596), cross-attention over the flattened
    multi-view DINO features."""
    B = x.shape[0]
    depth = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('blocks.'))
    mv = _fp(context['concat'])
    dino_tok = mv.reshape(B, mv.shape[1] * mv.shape[2], mv.shape[3])
    t = t_embedder(sd, _fp(timesteps))
    t0 = linear(F.silu(t), sd['adaLN_modulation.1.weight'], sd['adaLN_modulation.1.bias'])
    h = patchify_embed(sd, x, patch) + sd['pos_embed']
    none = h.new_zeros(B, 0, h.shape[-1])
    for i in range(depth):
        h = i23d_block(sd, f'blocks.{i}.', h, t0, none, dino_tok, num_heads)
    shift, scale = (sd['final_layer.scale_shift_table'][None] + t[:, None]).chunk(2, dim=1)
    y = layer_norm(h) * (1 + scale) + shift
    y = F.linear(y, sd['final_layer.linear.weight'], sd['final_layer.linear.bias'])     # fp32 in the HIP path too (final_layer kernel)
    c_out = y.shape[-1] // (patch * patch)
    return _fp(unpatchify_trilatent(y, B, patch, c_out))


def i23d_forward_with_cfg(sd, x, t, context, cfg_scale, num_heads):
    eps = i23d_forward(sd, x, t, context, num_heads)
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    half = uncond + cfg_scale * (cond - uncond)
    return torch.cat([half, half], dim=0)
