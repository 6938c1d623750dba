"""DiT_I23D_PixelArt (image -> tri-plane latent flow-matching denoiser) on the HIP kernels.

Surface of the reference's dit/dit_i23d.py:173-291 (`DiT_models['DiT-PixArt-L/2'](input_size, num_classes,
learn_sigma, in_channels, context_dim, roll_out, pooling_ctx_dim)`, `forward(x, timesteps, context)` with the sgm
context dict {'crossattn': [B,256,2048] = CLIP(1024) || DINO(1024), 'vector': [B,768]}, `forward_with_cfg`) and its
state-dict keys.  Blocks are ImageCondDiTBlockPixelArtRMSNorm (dit/dit_models_xformers.py:481-539,604-618):
ONE shared adaLN whose output is added to a per-block learned scale_shift_table, RMSNorm pre-norms, self-attention over
[modulated x (768) ; projected DINO tokens (256)] with per-head RMSNorm on q/k, cross-attention to the RMS-normed CLIP
tokens, erf-GELU MLP; T2IFinalLayer.  Everything that depends only on the conditioning image (cap_embedder token,
DINO projection, normed CLIP tokens, every block's cross K / V^T) is computed once per prompt (prepare_context).
"""
import os

import torch
import torch.nn as nn

from .. import ops
from .dit_base import DiT
from .dit_models_xformers import (CaptionEmbedder, ImageCondDiTBlock, ImageCondDiTBlockPixelArtRMSNorm, Mlp, PixelArtTextCondDiTBlock,
                                  RMSNormP, T2IFinalLayer, bf16, f32, pack_caption, attn_head_pad)


class DiT_I23D_PixelArt(DiT):
    # the prompt-side modules of the class, in state-dict order behind final_layer ('clip_text_proj': in front of the blocks).
    # clip_spatial_proj is present in the single-view checkpoints and unused by their forward.
    PROMPT_MODULES = ('dino_proj', 'clip_spatial_proj', 'adaLN_modulation', 'cap_embedder', 'attention_y_norm')
    _norm_kind = (1, 1e-5)             # pre-norms: RMSNorm(eps 1e-5) with a weight; the plain DiT_I23D uses affine-free LayerNorm

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3, mixed_prediction=True,
                 context_dim=False, pooling_ctx_dim=768, roll_out=False, vit_blk=ImageCondDiTBlockPixelArtRMSNorm,
                 final_layer_blk=T2IFinalLayer):
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_ratio,
                         class_dropout_prob, num_classes, learn_sigma, mixing_logit_init, mixed_prediction, context_dim,
                         roll_out, vit_blk, T2IFinalLayer)
        self.clip_ctx_dim = 1024
        make = {'dino_proj': lambda: CaptionEmbedder(context_dim, hidden_size),
                'clip_spatial_proj': lambda: CaptionEmbedder(1024, hidden_size),
                'adaLN_modulation': lambda: nn.Sequential(nn.SiLU(), nn.Linear(hidden_size, 6 * hidden_size, bias=True)),
                'cap_embedder': lambda: nn.Sequential(nn.LayerNorm(pooling_ctx_dim), nn.Linear(pooling_ctx_dim, hidden_size)),
                'attention_y_norm': lambda: RMSNormP(1024)}
        for name in self.PROMPT_MODULES:
            if name in make:
                setattr(self, name, make[name]())
        self.pooling_ctx_dim = pooling_ctx_dim

    APPEND_PROJ = 'dino_proj'          # the CaptionEmbedder whose output tokens are appended to the self-attention sequence (None: none)
    _uc_first = False                  # the flow-matching engine's [c, uc] order: the unconditional samples trail

    def _pack_prompt(self, P, device):
        if 'cap_embedder' in self.PROMPT_MODULES:
            P['cap_ln_w'], P['cap_ln_b'] = f32(self.cap_embedder[0].weight, device), f32(self.cap_embedder[0].bias, device)
            P['cap_w'], P['cap_b'] = bf16(self.cap_embedder[1].weight, device), f32(self.cap_embedder[1].bias, device)
        if 'attention_y_norm' in self.PROMPT_MODULES:
            P['ynorm_w'] = f32(self.attention_y_norm.weight, device)
        if self.APPEND_PROJ is not None:
            pack_caption(P, 'd', getattr(self, self.APPEND_PROJ), device)
        P['fin_sst'] = f32(self.final_layer.scale_shift_table, device)          # [2, D]
        P['zeros'] = torch.zeros(max(self.embed_dim, self.pooling_ctx_dim), device=device)

    def _cls_token(self, vec):
        """pooled token: LayerNorm(affine, eps 1e-5) -> Linear   (dit_i23d.py:211-217,245)"""
        P, ws, D = self._packed, self._ws, self.embed_dim
        Bn = vec.shape[0]
        vn = ws.get('cap_vn', (Bn, self.pooling_ctx_dim), torch.bfloat16)
        ops.norm_modulate(vec.contiguous().float(), vn, Bn, self.pooling_ctx_dim, kind=0, eps=1e-5, weight=P['cap_ln_w'],
                          shift=P['cap_ln_b'], scale=P['zeros'], mod_rows=1 << 30, mod_ld=0)
        cls = torch.empty(Bn, D, device=vec.device, dtype=torch.float32)
        ops.gemm(vn, P['cap_w'], P['cap_b'], ops.EPI_F32, cls)
        return cls

    def _appended_tokens(self, feats):
        """CaptionEmbedder (Linear -> tanh-GELU -> Linear) of [Bn, L, C] features -> bf16 [Bn, L, D]."""
        Bn, L, _ = feats.shape
        return self._caption_mlp(feats, 'd', torch.empty(Bn, L, self.embed_dim, device=feats.device, dtype=torch.bfloat16))

    @torch.no_grad()
    def prepare_context(self, context):
        ca, vec = context['crossattn'], context['vector']
        self._ensure_packed(ca.device)
        Bn, Lc, _ = ca.shape
        C1 = self.clip_ctx_dim
        want = C1 + self.dino_proj.y_proj.fc1.in_features
        if ca.shape[-1] != want or vec.shape[-1] != self.pooling_ctx_dim:
            raise ValueError(f"context['crossattn'] must be [B, L, {want}] (CLIP {C1} || DINO) and context['vector'] [B, {self.pooling_ctx_dim}]; "
                             f"got {tuple(ca.shape)} / {tuple(vec.shape)}")
        cls = self._cls_token(vec)
        # CLIP tokens: the model's attention_y_norm once for every layer (dit_i23d.py:247), or without one (the plain DiT_I23D) each
        # BLOCK's own in front of its K / V GEMM; DINO tokens: tanh-GELU MLP
        clip, own_norm = ca[..., :C1], 'attention_y_norm' not in self.PROMPT_MODULES
        if not own_norm:
            clip = self._ws.get('clip_n', (Bn * Lc, C1), torch.bfloat16)
            ops.norm_modulate(ca[..., :C1].contiguous().float(), clip, Bn * Lc, C1, kind=1, eps=1e-5, weight=self._packed['ynorm_w'])
        dino = self._appended_tokens(ca[..., C1:])
        k_all, vt_all, lpad = self._cross_kv(clip, Bn, Lc, block_norm=own_norm)
        return self._finish_context({'k': k_all, 'vt': vt_all, 'Lc': Lc, 'lpad': lpad, 'Bn': Bn, 'cls': cls, 'dino': dino}, ca[..., :C1])

    def _multiview_context(self, mv, cls, appended):
        """the prepared context of the multi-view classes: cross-attention over the flattened DINO features mv [B, V, L, C], raw"""
        Bn, Lk = mv.shape[0], mv.shape[1] * mv.shape[2]
        mvb = self._ws.get('mv_in', (Bn * Lk, mv.shape[3]), torch.bfloat16)
        ops.cast_bf16(mv.reshape(Bn * Lk, mv.shape[3]).contiguous().float(), mvb)
        k_all, vt_all, lpad = self._cross_kv(mvb, Bn, Lk)
        return self._finish_context({'k': k_all, 'vt': vt_all, 'Lc': Lk, 'lpad': lpad, 'Bn': Bn, 'cls': cls, 'dino': appended}, mv.reshape(Bn, Lk, -1))

    # ------------------------------------------------------------------ the hooks of the forward template (dit_base.DiT.forward)
    def _conditioning(self, timesteps, cc, opts):
        """t = t_embedder(timesteps) + the pooled token: (SiLU(t) bf16, the adaLN GEMM's operand; t fp32 for the T2IFinalLayer)"""
        Bn, D = timesteps.shape[0], self.embed_dim
        temb, tsilu = self._timestep_embed(timesteps, '', silu=False)
        tsum = self._ws.get('tsum', (Bn, D), torch.float32)
        ops.add_act_cast(temb, cc['cls'], tsilu, tsum, Bn * D, 1)
        return tsilu, tsum

    def _modulation(self, tsilu, Bn, opts):
        """(i -> [Bn, 6D] view of block i's shift/scale/gate rows, row stride): t2i blocks = shared adaLN(t) + scale_shift_table[i]"""
        P, ws, D, depth = self._packed, self._ws, self.embed_dim, self.depth
        t0 = ws.get('t0', (Bn, 6 * D), torch.float32)
        ops.gemm(tsilu, P['ada_w'], P['ada_b'], ops.EPI_F32, t0)
        mod = ws.get('modb', (depth, Bn, 6 * D), torch.float32)
        ops.add_table_rows(t0, P['sst'], mod, depth, Bn, 6 * D)
        return (lambda i: mod[i]), 6 * D

    def _appended(self, cc, Bn, N):
        """The tokens appended to the self-attention sequence: their per-layer K / V^T, cached once per prompt (_appended_kv), or
        failing that the joint-sequence buffer [Bn, N + Ld, D] whose rows [N, N + Ld) of every sample hold them."""
        Ld = cc['dino'].shape[1]
        akv = self._appended_kv(cc, Bn, N) if Ld else None
        if akv is not None:
            return (akv[0], akv[1], N + Ld), None
        ha = self._ws.get('ha', (Bn, N + Ld, self.embed_dim), torch.bfloat16)
        if getattr(self, '_ha_src', None) is not cc['dino'] or getattr(self, '_ha_buf', None) is not ha:
            ha[:, N:].copy_(cc['dino'])                            # appended DINO tokens: constant per prompt, and the
            self._ha_src, self._ha_buf = cc['dino'], ha            # norm kernel only ever writes rows < N of each sample
        return None, ha

    APPEND_CACHE_MAX_BYTES = 16 << 30

    def _appended_kv(self, cc, Bn, N):
        """The tokens appended to the self-attention sequence (projected DINO / CLIP tokens) are constant per prompt, and so are
        their keys and values in every block: self-attention K / V^T buffers per layer ([depth, Bn, H, NA, Dh], 3.2 GB each at
        network batch 64 - sized for 288 GB of HBM) whose rows [N, NA) are filled ONCE here with the same QKV GEMM + head split
        (+ fused qk-norm) the blocks use; forward() then projects the x tokens only (25 % fewer QKV GEMM rows per layer and step
        at 768 + 256 tokens).  Needs the fused qk-norm epilogue (an unfused norm pass would re-normalise the cached rows every
        step); LN3D_NO_APPEND_CACHE=1 or a cache above APPEND_CACHE_MAX_BYTES fall back to projecting the whole sequence."""
        if 'akv' in cc and cc.get('akv_N') == N:
            return cc['akv']
        cc['akv'], cc['akv_N'] = None, N               # per token count: the point-cloud variant takes any number of points per call
        P, ws, D, H = self._packed, self._ws, self.embed_dim, self.num_heads
        Ld = cc['dino'].shape[1]
        Dh = D // H
        Dp = attn_head_pad(Dh)
        NA = N + Ld
        npad = (NA + 63) // 64 * 64
        qk = P['blocks'][0]['qn'] is not None
        if (os.environ.get('LN3D_NO_APPEND_CACHE') or N % 32 or Ld % 32
                or 2 * self.depth * Bn * H * npad * Dp * 2 > self.APPEND_CACHE_MAX_BYTES
                or (qk and not ops.heads_norm_fusable(Bn * N, 3 * H * Dp, N, Dh, Dp))):
            return None
        fused = qk and ops.heads_norm_fusable(Bn * Ld, 3 * H * Dp, Ld, Dh, Dp)    # small prompts batches: norm in a second pass
        dev = cc['dino'].device
        # The prepared context `cc` OWNS these buffers for its lifetime (every live context holds its own copy): the cache is taken
        # only while it fits a third of the device memory that is free right now, and an allocation failure falls back to the
        # full projection as well (several prepared prompts, or a smaller-HBM part, must not die in forward()).
        need = 2 * self.depth * Bn * H * npad * Dp * 2
        try:
            if dev.type == 'cuda' and need > torch.cuda.mem_get_info(dev)[0] // 3:
                return None
            sa_k = torch.zeros(self.depth, Bn, H, npad, Dp, dtype=torch.bfloat16, device=dev)
            sa_vt = torch.zeros(self.depth, Bn, H, Dp, npad, dtype=torch.bfloat16, device=dev)
        except torch.cuda.OutOfMemoryError:
            return None
        qs = ws.get('sa_q', (Bn, H, npad, Dp), torch.bfloat16, zero=True, extent=N)
        rows = cc['dino'].reshape(Bn * Ld, D)
        for i, q in enumerate(P['blocks']):
            # outputs 1 / 2 start at token N of every (sample, head): the epilogue addresses [b, h, t, :] / [b, h, :, t] with the
            # buffers' own tok_pad stride, so a base pointer moved by N tokens is all it takes
            ops.gemm(rows, q['qkv_w'], q['qkv_b'], ops.EPI_HEADS, qs, sa_k[i][:, :, N:], sa_vt[i][:, :, :, N:], M=Bn * Ld, tokens=Ld,
                     tok_pad=npad, heads=H, head_dim=Dh, transpose_mask=0b100, head_dim_pad=Dp,
                     head_norm0=q['qn'] if fused else None, head_norm1=q['kn'] if fused else None)
            if qk and not fused:       # whole buffer: the x rows are still zero here and stay zero under the norm
                ops.rmsnorm_heads(sa_k[i], q['kn'], Bn * H * npad, Dp, true_dim=Dh)
        qs.zero_()                                                      # the scratch queries of the appended rows are not used
        cc['akv'] = (sa_k, sa_vt, npad, Dp)
        return cc['akv']

    def _output(self, xt, tsum, mod_of, ld, Bn, N):
        """T2IFinalLayer (LN, scale_shift_table + t, Linear) + unpatchify -> [Bn, 3*C_out, S, S]"""
        P, D, S = self._packed, self.embed_dim, self.input_size
        out = torch.empty(Bn, self.out_channels * 3, S, S, dtype=torch.float32, device=xt.device)
        ops.final_layer(xt, tsum, tsum, D, P['fin_sst'][0], P['fin_sst'][1], P['fin_w'], P['fin_b'], out, Bn,
                        self.out_channels, S, self.patch_size, D)
        return out

    @torch.no_grad()
    def forward_with_cfg(self, x, t, context=None, cfg_scale=4.0, context_cache=None, **kw):
        eps = self.forward(x, t, context, context_cache=context_cache)
        ops.cfg_combine_dup(eps, float(cfg_scale))
        return eps


class DiT_I23D(DiT_I23D_PixelArt):
    """The plain image-conditioned DiT (reference dit/dit_i23d.py:24-170; registry 'DiT-XL/2', 'DiT-L/2', 'DiT-B/2', 'DiT-B/1' of
    dit_i23d.DiT_models): ImageCondDiTBlock blocks - every block has its OWN adaLN (no shared adaLN / scale_shift_table),
    affine-free LayerNorm(eps 1e-6) pre-norms and its own attention_y_norm for the CLIP tokens; the pooled token is
    clip_text_proj(context['vector']) (CaptionEmbedder, tanh-GELU MLP); T2IFinalLayer.  Runs on the same block machinery as the
    PixArt variant: only the modulation source, the pre-norm kind, the pooled token and where the CLIP tokens are normed differ."""

    PROMPT_MODULES = ('clip_text_proj', 'dino_proj', 'clip_spatial_proj')
    _norm_kind = (0, 1e-6)

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3, mixed_prediction=True,
                 context_dim=False, pooling_ctx_dim=768, roll_out=False, vit_blk=ImageCondDiTBlock, final_layer_blk=T2IFinalLayer):
        # the pooled vector goes through clip_text_proj, whose input width is context_dim
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_ratio, class_dropout_prob,
                         num_classes, learn_sigma, mixing_logit_init, mixed_prediction, context_dim, context_dim, roll_out, vit_blk,
                         T2IFinalLayer)

    def _modulation(self, tsilu, Bn, opts):
        P, ws, D, depth = self._packed, self._ws, self.embed_dim, self.depth
        mod = ws.get('modall', (Bn, depth * 6 * D), torch.float32)
        ops.gemm(tsilu, P['ada_w'], P['ada_b'], ops.EPI_F32, mod)
        return (lambda i: mod[:, i * 6 * D:]), depth * 6 * D

    def _cls_token(self, vec):
        """clip_text_proj(context['vector']): Linear -> tanh-GELU -> Linear, fp32 out (dit_i23d.py:112)"""
        return self._caption_mlp(vec, 'c', torch.empty(vec.shape[0], self.embed_dim, device=vec.device, dtype=torch.float32))


class DiT_I23D_PixelArt_MVCond(DiT_I23D_PixelArt):
    """Multi-view image conditioned variant (reference dit/dit_i23d.py:293-384): the projected CLIP spatial tokens
    (clip_spatial_proj) are appended to the self-attention sequence, the flattened multi-view DINO features context['concat']
    [B, V, L, C] are the cross-attention context (raw: no attention_y_norm, no projection); `dino_proj` does not exist.
    Same blocks / kernels as the single-view model: only the prompt-side preparation differs."""

    PROMPT_MODULES = ('clip_spatial_proj', 'adaLN_modulation', 'cap_embedder', 'attention_y_norm')

    APPEND_PROJ = 'clip_spatial_proj'

    @torch.no_grad()
    def prepare_context(self, context):
        ca, vec, mv = context['crossattn'], context['vector'], context['concat']
        if ca.shape[-1] != self.clip_spatial_proj.y_proj.fc1.in_features or mv.dim() != 4:
            raise ValueError(f"MVCond context: 'crossattn' [B, L, {self.clip_spatial_proj.y_proj.fc1.in_features}] (CLIP spatial tokens), "
                             f"'concat' [B, V, L, C] (multi-view DINO); got {tuple(ca.shape)} / {tuple(mv.shape)}")
        self._ensure_packed(ca.device)
        cls = self._cls_token(vec)
        return self._multiview_context(mv, cls, self._appended_tokens(ca))


class DiT_I23D_PixelArt_MVCond_noClip(DiT_I23D_PixelArt):
    """Multi-view variant without any CLIP branch (reference dit/dit_i23d.py:387-492; registered there as
    'DiT-PixArt-MV-L/2'): t = t_embedder(timesteps), nothing is appended to the self-attention sequence
    (ImageCondDiTBlockPixelArtNoclip), cross-attention over the flattened multi-view DINO features context['concat'];
    dino_proj, clip_spatial_proj and cap_embedder do not exist."""

    PROMPT_MODULES = ('adaLN_modulation', 'attention_y_norm')

    APPEND_PROJ = None

    @torch.no_grad()
    def prepare_context(self, context):
        mv = context['concat']
        dev = mv.device
        self._ensure_packed(dev)
        Bn, D = mv.shape[0], self.embed_dim
        return self._multiview_context(mv, torch.zeros(Bn, D, device=dev), torch.zeros(Bn, 0, D, device=dev, dtype=torch.bfloat16))


class DiT_TriLatent_PixelArt(DiT_I23D_PixelArt):
    """T23D DiT with PixArt-style blocks (reference dit/dit_trilatent.py:146-270; registry 'DiT-PixelArt-L/2', 'DiT-PixelArt-B/2'):
    t = t_embedder + cap_embedder(context['vector']), one shared adaLN + per-block scale_shift_table, PixelArtTextCondDiTBlock
    (RMSNorm pre-norms, no qk-norm, cross-attention over the text tokens normalised per block), T2IFinalLayer, and the
    `forward_with_cfg(x, t, context=..., cfg_scale=...)` the flow-matching engine calls - i.e. the T23D denoiser of that engine.
    Runs on the I23D block machinery: nothing is appended to the self-attention sequence, the per-block normalised context's
    K / V^T are computed once per prompt."""

    PROMPT_MODULES = ('adaLN_modulation', 'cap_embedder')

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3, mixed_prediction=True,
                 context_dim=False, roll_out=False, vit_blk=None, final_layer_blk=T2IFinalLayer):
        # the text context is both the cross-attention tokens and (pooled) the cap_embedder's input
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_ratio, class_dropout_prob,
                         num_classes, learn_sigma, mixing_logit_init, mixed_prediction, context_dim, context_dim, roll_out,
                         PixelArtTextCondDiTBlock, T2IFinalLayer)
        self.clip_ctx_dim = context_dim

    APPEND_PROJ = None

    @torch.no_grad()
    def prepare_context(self, context):
        ca, vec = context['crossattn'], context['vector']
        if ca.shape[-1] != self.clip_ctx_dim or vec.shape[-1] != self.pooling_ctx_dim:
            raise ValueError(f"context['crossattn'] [B, L, {self.clip_ctx_dim}] text tokens and context['vector'] [B, {self.pooling_ctx_dim}]; "
                             f"got {tuple(ca.shape)} / {tuple(vec.shape)}")
        dev = ca.device
        self._ensure_packed(dev)
        Bn, Lc, _ = ca.shape
        D = self.embed_dim
        cls = self._cls_token(vec)
        k_all, vt_all, lpad = self._cross_kv(ca, Bn, Lc, block_norm=True)               # the BLOCK's attention_y_norm
        return self._finish_context({'k': k_all, 'vt': vt_all, 'Lc': Lc, 'lpad': lpad, 'Bn': Bn, 'cls': cls,
                              'dino': torch.zeros(Bn, 0, D, device=dev, dtype=torch.bfloat16)}, ca)


def DiT_L_TriLatent_Pixelart_2(**kwargs):         # dit_trilatent.py:311-318 ('DiT-PixelArt-L/2')
    kwargs.pop('vit_blk', None)
    return DiT_TriLatent_PixelArt(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_B_TriLatent_Pixelart_2(**kwargs):         # dit_trilatent.py:302-309 ('DiT-PixelArt-B/2')
    kwargs.pop('vit_blk', None)
    return DiT_TriLatent_PixelArt(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


class DiT_pcd_I23D_PixelArt_MVCond(DiT_I23D_PixelArt_MVCond):
    """Point-cloud latent variant (reference dit/dit_i23d.py:500-588; registry key 'DiT-PixArt-MV-PCD-L'): the tokens are the N
    points of x [B, N, in_channels]; x_embedder is a timm Mlp (Linear -> tanh-GELU -> Linear) instead of the conv patch-embed,
    there is no positional embedding and no unpatchify - the output is [B, N, out_channels].  Conditioning and blocks as MVCond.
    On the HIP path the embedder runs as two GEMMs with the input channels zero-padded to the GEMM's K granule, and the final
    Linear as a bf16 GEMM (the output width is padded to a multiple of 4 and sliced)."""

    def _build_embedder(self):
        self.x_embedder = Mlp(self.in_channels, self.embed_dim, self.embed_dim)

    def _pack_embedder(self, P, device):
        C, D = self.in_channels, self.embed_dim
        kp = (C + 63) // 64 * 64
        w1 = torch.zeros(D, kp)
        w1[:, :C] = self.x_embedder.fc1.weight.detach().float().cpu()
        P['xe_w1'], P['xe_b1'] = bf16(w1, device), f32(self.x_embedder.fc1.bias, device)
        P['xe_w2'], P['xe_b2'] = bf16(self.x_embedder.fc2.weight, device), f32(self.x_embedder.fc2.bias, device)
        P['xe_kpad'] = kp
        co = self.final_layer.linear.weight.shape[0]
        cp = (co + 3) // 4 * 4
        fw = torch.zeros(cp, D)
        fw[:co] = self.final_layer.linear.weight.detach().float().cpu()
        fb = torch.zeros(cp)
        fb[:co] = self.final_layer.linear.bias.detach().float().cpu()
        P['finp_w'], P['finp_b'], P['finp_n'] = bf16(fw, device), f32(fb, device), co

    def _num_tokens(self, x):
        return x.shape[1]

    def _embed_tokens(self, x, in_scale, Bx, Bn, N):
        P, ws, D = self._packed, self._ws, self.embed_dim
        assert x.dim() == 3 and x.shape[2] == self.in_channels, "point-cloud latent [B, N, in_channels]"
        xin = x.float()
        if in_scale is not None:                       # c_in of a denoiser wrapper, one factor per network row
            xin = xin.repeat(Bn // Bx, 1, 1) * in_scale.view(-1, 1, 1)
        elif Bn != Bx:
            xin = xin.repeat(Bn // Bx, 1, 1)
        xb = ws.get('pcd_in', (Bn * N, P['xe_kpad']), torch.bfloat16, zero=True)
        xb[:, :self.in_channels] = xin.reshape(Bn * N, self.in_channels).to(torch.bfloat16)
        h1 = ws.get('pcd_h', (Bn * N, D), torch.bfloat16)
        ops.gemm(xb, P['xe_w1'], P['xe_b1'], ops.EPI_GELU_TANH, h1)
        xt = ws.get('x', (Bn * N, D), torch.float32)
        ops.gemm(h1, P['xe_w2'], P['xe_b2'], ops.EPI_F32, xt)
        return xt

    def _output(self, xt, tsum, mod_of, ld, Bn, N):
        P, ws, D = self._packed, self._ws, self.embed_dim
        yb = ws.get('pcd_fin', (Bn * N, D), torch.bfloat16)
        ops.norm_modulate(xt, yb, Bn * N, D, kind=0, eps=1e-6, shift=tsum, scale=tsum, mod_rows=N, mod_ld=D,
                          shift_table=P['fin_sst'][0], scale_table=P['fin_sst'][1])
        out = torch.empty(Bn * N, P['finp_w'].shape[0], device=xt.device, dtype=torch.float32)
        ops.gemm(yb, P['finp_w'], P['finp_b'], ops.EPI_F32, out)
        return out[:, :P['finp_n']].reshape(Bn, N, P['finp_n']).contiguous()


def DiT_L_Pixelart_MV_pcd(**kwargs):          # reference dit_i23d.py:675-681
    return DiT_pcd_I23D_PixelArt_MVCond(depth=24, hidden_size=1024, patch_size=1, num_heads=16, **kwargs)


def DiT_L_Pixelart_MV_2_noclip(**kwargs):
    return DiT_I23D_PixelArt_MVCond_noClip(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_L_Pixelart_MV_2(**kwargs):
    return DiT_I23D_PixelArt_MVCond(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_XL_Pixelart_MV_2(**kwargs):       # reference dit_i23d.py:659-664; head size 72 runs in zero-padded 128-wide heads
    return DiT_I23D_PixelArt_MVCond(depth=28, hidden_size=1152, patch_size=2, num_heads=16, **kwargs)


def DiT_B_Pixelart_MV_2(**kwargs):
    return DiT_I23D_PixelArt_MVCond(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def DiT_L_Pixelart_2(**kwargs):
    return DiT_I23D_PixelArt(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_B_Pixelart_2(**kwargs):
    return DiT_I23D_PixelArt(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def DiT_XL_2(**kwargs):                   # reference dit_i23d.py:597-626: the plain DiT_I23D sizes
    return DiT_I23D(depth=28, hidden_size=1152, patch_size=2, num_heads=16, **kwargs)


def DiT_L_2(**kwargs):
    return DiT_I23D(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_B_2(**kwargs):
    return DiT_I23D(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def DiT_B_1(**kwargs):
    return DiT_I23D(depth=12, hidden_size=768, patch_size=1, num_heads=12, **kwargs)


MV_NOCLIP_ARCHS = {'DiT-PixArt-MV-L/2'}        # registry keys built on DiT_I23D_PixelArt_MVCond_noClip (no CLIP tokens in the context)
DiT_models = {'DiT-XL/2': DiT_XL_2, 'DiT-L/2': DiT_L_2, 'DiT-B/2': DiT_B_2, 'DiT-B/1': DiT_B_1,
              'DiT-PixArt-L/2': DiT_L_Pixelart_2, 'DiT-PixArt-B/2': DiT_B_Pixelart_2,
              # reference registry (dit_i23d.py:686-696): 'MV-L/2' is the no-CLIP class, 'MV-B/2' the CLIP+DINO one
              'DiT-PixArt-MV-L/2': DiT_L_Pixelart_MV_2_noclip, 'DiT-PixArt-MV-B/2': DiT_B_Pixelart_MV_2,
              'DiT-PixArt-MVCond-L/2': DiT_L_Pixelart_MV_2, 'DiT-PixArt-MV-XL/2': DiT_XL_Pixelart_MV_2,
              'DiT-PixArt-MV-PCD-L': DiT_L_Pixelart_MV_pcd}
