"""`DiT`: the one base of the DiT denoiser family - what the text-conditioned DiT_TriLatent (dit_trilatent.py) and the image-conditioned
DiT_I23D_PixelArt with its variants (dit_i23d.py) share, and the ONE per-step block loop both run.

The base owns the constructor (reference dit/dit_models_xformers.py:681-835), the weight pack, the per-prompt helpers, the matmul
precision switch and the forward template:

  forward     : device / pack / prepared-cache checks -> `_conditioning` (timestep embedding, + the pooled token where the class has
                one) -> `_modulation` (i -> block i's adaLN rows, row stride) -> `_embed_tokens` -> the block loop -> `_output`
  per block   : `_self_attention_block`  pre-norm+modulate -> QKV GEMM (head-split epilogue, V^T emitted, qk-norm) -> fused attention
                                         -> proj GEMM (gate*out + residual epilogue, bf16 copy of x, the fold's constant rows)
                `_cross_attend`          to_q GEMM (head split, q-norm) -> attention over the prompt's cached K / V^T, on the samples
                                         that are not folded; then the to_out GEMM (residual epilogue)
                MLP                      pre-norm+modulate -> fc1 GEMM (erf-GELU epilogue) -> fc2 GEMM (gate*out + residual epilogue)
The residual stream, norm statistics, softmax and all accumulators are fp32; GEMM operands are bf16, or MX-FP8 (include/ln3d_mx.h)
where the pack holds ops.MX weights: every step takes the operand kind from what it is handed, not from the class.

A family class states its blocks, which prompt-side modules it has (PROMPT_MODULES), its pre-norm kind, which precisions its pack
supports (PACK_PRECISIONS) and the hooks above.  dit_i23d.py does not import dit_trilatent.py; that one imports from dit_i23d.py only
the two PixArt-style T23D factories its registry lists.
"""
import os

import torch
import torch.nn as nn

from .. import ops, _cache
from .dit_models_xformers import (CaptionEmbedder, DiTBlock, FinalLayer, PatchEmbed, TimestepEmbedder, Workspace, bf16, f32,
                                  get_2d_sincos_pos_embed, self_attention_hip, pack_block, pack_block_mx, pack_caption)


class DiT(_cache.PackedWeights, nn.Module):
    PROMPT_MODULES = ('clip_text_proj',)   # the prompt-side modules of the class, in state-dict order (clip_text_proj sits in front of the blocks)
    MATMUL_PRECISIONS = ('bf16', 'mxfp8')
    PACK_PRECISIONS = ('bf16',)            # what the class's pack and forward hooks are built for
    _matmul_precision = 'bf16'
    _norm_kind = (0, 1e-6)                 # the blocks' pre-norms: affine-free LayerNorm(eps 1e-6); (1, 1e-5): RMSNorm with a weight
    _uc_first = True                       # the unconditional CFG samples lead the batch: VanillaCFG's [uc, c] order

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16,
                 mlp_ratio=4, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3,
                 mixed_prediction=True, context_dim=False, roll_out=False, vit_blk=DiTBlock,
                 final_layer_blk=FinalLayer):
        super().__init__()
        self.plane_n = 3
        self.depth, self.mlp_ratio, self.learn_sigma = depth, mlp_ratio, learn_sigma
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.patch_size, self.num_heads, self.embed_dim = patch_size, num_heads, hidden_size
        self.input_size = input_size
        self.roll_out = roll_out
        self._build_embedder()
        self.t_embedder = TimestepEmbedder(hidden_size)
        self.y_embedder = None
        if 'clip_text_proj' in self.PROMPT_MODULES:
            self.clip_text_proj = CaptionEmbedder(context_dim, hidden_size) if context_dim is not None else None
        self.context_dim = context_dim
        self.blocks = nn.ModuleList([vit_blk(hidden_size=hidden_size, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                             context_dim=context_dim) for _ in range(depth)])
        self.final_layer = final_layer_blk(hidden_size, patch_size, self.out_channels)
        self.initialize_weights()
        self._ws = None

    def _build_embedder(self):
        """token embedder and positional embedding: the conv patch-embed shared by the three planes + the 3D-aware sincos table"""
        self.x_embedder = PatchEmbed(self.input_size, self.patch_size, self.in_channels, self.embed_dim, bias=True)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.x_embedder.num_patches, self.embed_dim), requires_grad=False)
        assert self.roll_out
        self.init_PE_3D_aware()

    def init_PE_3D_aware(self):
        L = self.x_embedder.num_patches
        D = self.embed_dim
        pe = get_2d_sincos_pos_embed(D, (self.plane_n, L)).reshape(self.plane_n * L, D)
        self.pos_embed = nn.Parameter(torch.from_numpy(pe).float().unsqueeze(0), requires_grad=False)

    def initialize_weights(self):
        # same rules as the reference (:777-819); sampling uses loaded / synthetic weights anyway
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        if isinstance(self.x_embedder, PatchEmbed):
            w = self.x_embedder.proj.weight.data
            nn.init.xavier_uniform_(w.view([w.shape[0], -1]))
            nn.init.constant_(self.x_embedder.proj.bias, 0)
        nn.init.normal_(self.t_embedder.mlp[0].weight, std=0.02)
        nn.init.normal_(self.t_embedder.mlp[2].weight, std=0.02)
        for blk in self.blocks:
            if getattr(blk, 'adaLN_modulation', None) is not None:
                nn.init.constant_(blk.adaLN_modulation[-1].weight, 0)
                nn.init.constant_(blk.adaLN_modulation[-1].bias, 0)
        if getattr(self.final_layer, 'adaLN_modulation', None) is not None:
            nn.init.constant_(self.final_layer.adaLN_modulation[-1].weight, 0)
            nn.init.constant_(self.final_layer.adaLN_modulation[-1].bias, 0)
        nn.init.constant_(self.final_layer.linear.weight, 0)
        nn.init.constant_(self.final_layer.linear.bias, 0)

    # ------------------------------------------------------------------ matmul precision
    def set_matmul_precision(self, precision):
        """'bf16' (default: the reference's numerics up to bf16 GEMM operands) or 'mxfp8': the QKV, fc1 and fc2 GEMMs of every block
        on OCP MXFP8 operands (e4m3 elements, one E8M0 scale per 32 values along K), quantized on the device from the fp32 master
        weights when the model is packed.  Only the active precision's operands are kept; a change drops the packed copies.  A class
        takes the precisions its pack is built for (PACK_PRECISIONS)."""
        if precision not in self.MATMUL_PRECISIONS:
            raise ValueError(f"matmul precision {precision!r}: expected one of {self.MATMUL_PRECISIONS}")
        if precision not in self.PACK_PRECISIONS:
            raise ValueError(f"{type(self).__name__}: the {precision} path is built for the T23D DiT_TriLatent forward only")
        if precision != self._matmul_precision:
            self._matmul_precision = precision
            self._packed = None
            self._ws = None
        return self

    @property
    def matmul_precision(self):
        return self._matmul_precision

    # ------------------------------------------------------------------ packing
    def _pack(self, P, device):
        H = self.num_heads
        self._pack_embedder(P, device)
        P['t_w0'], P['t_b0'] = bf16(self.t_embedder.mlp[0].weight, device), f32(self.t_embedder.mlp[0].bias, device)
        P['t_w2'], P['t_b2'] = bf16(self.t_embedder.mlp[2].weight, device), f32(self.t_embedder.mlp[2].bias, device)
        if getattr(self, 'clip_text_proj', None) is not None:
            pack_caption(P, 'c', self.clip_text_proj, device)
        shared = getattr(self, 'adaLN_modulation', None)
        if shared is not None:                                           # PixArt: ONE shared adaLN + per-block tables
            ada = [shared[1]]
            P['sst'] = f32(torch.stack([b.scale_shift_table.reshape(-1) for b in self.blocks], 0), device)   # [depth, 6D]
        else:                                     # every block's own adaLN (and a FinalLayer's), one GEMM: [depth*6D (+2D), D]
            ada = [m.adaLN_modulation[1] for m in (*self.blocks, self.final_layer) if m.adaLN_modulation is not None]
        P['ada_w'], P['ada_b'] = bf16(torch.cat([a.weight for a in ada], 0), device), f32(torch.cat([a.bias for a in ada], 0), device)
        self._pack_prompt(P, device)
        P['blocks'] = [pack_block(b, H, self.embed_dim // H, device) for b in self.blocks]
        P['precision'] = self._matmul_precision
        if P['precision'] == 'mxfp8':
            P['blocks'] = [pack_block_mx(q, b, device) for q, b in zip(P['blocks'], self.blocks)]
        P['fin_w'], P['fin_b'] = f32(self.final_layer.linear.weight, device), f32(self.final_layer.linear.bias, device)
        self._ws = Workspace(device)

    def _pack_embedder(self, P, device):
        D = self.embed_dim
        P['pe_w'] = f32(self.x_embedder.proj.weight.reshape(D, -1), device)
        P['pe_b'] = f32(self.x_embedder.proj.bias, device)
        P['pos'] = f32(self.pos_embed[0], device)

    def _pack_prompt(self, P, device):
        """model-level weights of the prompt-side preparation beyond the caption MLP (none here)"""

    # ------------------------------------------------------------------ context helpers (constant per prompt)
    def _caption_mlp(self, x, pfx, out):
        """CaptionEmbedder (Linear -> tanh-GELU -> Linear) with the packed weights P[pfx + '_w1' ...] of x [..., C] -> out [..., D]:
        bf16 tokens or fp32 rows, by out's dtype."""
        P, ws = self._packed, self._ws
        R = x.numel() // x.shape[-1]
        xb = ws.get('cap_in', (R, x.shape[-1]), torch.bfloat16)
        ops.cast_bf16(x.contiguous().float(), xb)
        h1 = ws.get('cap_h', (R, self.embed_dim), torch.bfloat16)
        ops.gemm(xb, P[pfx + '_w1'], P[pfx + '_b1'], ops.EPI_GELU_TANH, h1)
        ops.gemm(h1, P[pfx + '_w2'], P[pfx + '_b2'], ops.EPI_BF16 if out.dtype == torch.bfloat16 else ops.EPI_F32, out)
        return out

    def _cross_kv(self, ctx, Bn, Lk, block_norm=False):
        """Every block's cross-attention K / V^T (and the block's k-norm, if it has one) of the context: ctx [Bn*Lk, C] bf16, or with
        block_norm the raw context [Bn, Lk, C], normalised by each block's own attention_y_norm in front of that block's GEMM."""
        P, H = self._packed, self.num_heads
        lpad = (Lk + 63) // 64 * 64
        dev = ctx.device
        k_all = torch.zeros(self.depth, Bn, H, lpad, 64, dtype=torch.bfloat16, device=dev)
        vt_all = torch.zeros(self.depth, Bn, H, 64, lpad, dtype=torch.bfloat16, device=dev)
        if block_norm:
            raw, C = ctx.contiguous().float(), ctx.shape[-1]
            ctx = self._ws.get('ctx_n', (Bn * Lk, C), torch.bfloat16)
        for i, q in enumerate(P['blocks']):
            if block_norm:
                ops.norm_modulate(raw, ctx, Bn * Lk, C, kind=1, eps=1e-5, weight=q['ynorm'])
            ops.gemm(ctx, q['ckv_w'], None, ops.EPI_HEADS, k_all[i], vt_all[i], M=Bn * Lk, tokens=Lk, tok_pad=lpad, heads=H,
                     head_dim=64, transpose_mask=0b10)
            if q['ckn'] is not None:
                ops.rmsnorm_heads(k_all[i], q['ckn'], Bn * H * lpad, 64)
        return k_all, vt_all, lpad

    def _fold_uc(self, cc, rows):
        """Samples whose cross-attention context rows are all IDENTICAL - the zero embeddings of the unconditional CFG branch
        (force_uc_zero_embeddings, sgm_DiffusionEngine.py:448-452; pipeline._zero_uc; every K / V row of a sample is a row-wise
        function of its context row, so they are identical too): every key of such a sample is the same vector, softmax over
        identical scores is uniform whatever the query, and the cross-attention sub-block is the constant to_out(v) + b per
        (layer, sample).  For a run of such samples at the unconditional end of the batch (leading when _uc_first, else trailing:
        the flow-matching engine's [c, uc]) the constants are computed here, once per prompt, with the same kernels (bf16 V row ->
        to_out GEMM, fp32 accumulate); forward() adds them in the gate / residual epilogue of the self-attention projection and runs
        to_q / attention / to_out on the other samples only (LN3D_NO_UC_FOLD=1: off).  `rows`: [Bn, L, C] raw context the K / V
        were made from.  A batch that is uniform throughout is not folded (with one context row, every batch is)."""
        cc['fold'] = 0
        Bn = cc['Bn']
        if os.environ.get('LN3D_NO_UC_FOLD') or cc['Lc'] < 2 or Bn < 2:
            return cc
        same = (rows == rows[:, :1]).flatten(1).all(1).tolist()              # one host read per prompt
        if not self._uc_first:
            same.reverse()
        fold = 0
        while fold < Bn and same[fold]:
            fold += 1
        if not 0 < fold < Bn:
            return cc
        P, H, D = self._packed, self.num_heads, self.embed_dim
        uc = slice(0, fold) if self._uc_first else slice(Bn - fold, Bn)
        const = torch.zeros(self.depth, Bn, D, dtype=torch.float32, device=rows.device)       # the other samples' rows stay 0
        for i, q in enumerate(P['blocks']):
            v_row = cc['vt'][i, uc, :, :, 0].reshape(fold, H * 64).contiguous()        # V^T[b, h, d, key 0] = the attention output
            ops.gemm(v_row, q['co_w'], q['co_b'], ops.EPI_F32, const[i, uc])
        cc['fold'], cc['const'] = fold, const
        return cc

    def _finish_context(self, cc, rows):
        """Last step of every prepare_context: the cache is stamped with the epoch of the weights its K / V^T were made from (forward()
        refuses it under any other, _check_prepared), then the zero-context fold."""
        cc['epoch'] = self._packed['epoch']
        return self._fold_uc(cc, rows)

    def _check_prepared(self, cache, maker):
        """A prepared context / timestep cache holds values computed from the weights of ONE epoch (ln3diff_amd/_cache.py); after any
        weight change - the epoch is global, so a load into another module counts - it is refused instead of being mixed with the
        re-packed blocks.  One host integer compare: no device read, nothing inside a captured graph."""
        if cache.get('epoch') != self._packed['epoch']:
            raise RuntimeError(f"{type(self).__name__}: this cache was made by {maker}() before the weights changed (weights epoch "
                               f"{cache.get('epoch')}, now {self._packed['epoch']}); call {maker}() again")

    def _conditioned(self, fold, N):
        """(first token row, first sample) of the samples that run the cross-attention GEMMs: the ones behind a leading fold
        (_uc_first), or from 0 in front of a trailing one - there the pointers are the buffers' own."""
        return (fold * N, fold) if self._uc_first else (0, 0)

    # ------------------------------------------------------------------ forward: the steps every class shares
    def _timestep_embed(self, timesteps, tag, silu):
        """t [R] -> sincos(256) -> Linear + SiLU -> Linear: (t_emb f32 [R, D], scratch bf16 [R, D]).  With `silu` the second GEMM's
        epilogue also writes SiLU(t_emb) into the bf16 scratch (the adaLN GEMM's operand); without, the caller fills it."""
        P, ws, D = self._packed, self._ws, self.embed_dim
        R = timesteps.shape[0]
        t32 = timesteps.to(device=ws.device, dtype=torch.float32).contiguous()
        tf = ws.get(tag + 'tfreq', (R, 256), torch.bfloat16)
        ops.timestep_embedding(t32, tf, R, 256)
        th = ws.get(tag + 'th', (R, D), torch.bfloat16)
        ops.gemm(tf, P['t_w0'], P['t_b0'], ops.EPI_SILU, th)
        temb = ws.get(tag + 'temb', (R, D), torch.float32)
        tsilu = ws.get(tag + 'tsilu', (R, D), torch.bfloat16)
        ops.gemm(th, P['t_w2'], P['t_b2'], ops.EPI_F32_SILU if silu else ops.EPI_F32, temb, tsilu if silu else None)
        return temb, tsilu

    def _num_tokens(self, x):
        return 3 * (self.input_size // self.patch_size) ** 2

    def _embed_tokens(self, x, in_scale, Bx, Bn, N):
        """patchify + shared conv patch-embed + positional embedding (+ optional EDM c_in scale) -> fp32 tokens [Bn*N, D]"""
        P, D = self._packed, self.embed_dim
        xt = self._ws.get('x', (Bn * N, D), torch.float32)
        ops.patch_embed(x.contiguous().float(), in_scale, P['pe_w'], P['pe_b'], P['pos'], xt, Bx, Bn, self.in_channels, self.input_size,
                        self.patch_size, D)
        return xt

    def _appended(self, cc, Bn, N):
        """(cached K / V^T of the tokens a class appends to the self-attention sequence, or the joint-sequence buffer): none here"""
        return None, None

    def _norm_mod(self, x, h, w, shift, scale, N, ld, **joint):
        """pre-norm + adaLN modulate of the rows of x -> h, the QKV / fc1 operand: bf16, or MXFP8 when h is an ops.MX.  `joint`:
        rows_in / rows_out, when every sample's rows go to the head of a longer sequence in h."""
        rows, D = x.shape
        kind, eps = self._norm_kind
        (ops.norm_modulate_mx if isinstance(h, ops.MX) else ops.norm_modulate)(
            x, h, rows, D, kind=kind, eps=eps, weight=w, shift=shift, scale=scale, mod_rows=N, mod_ld=ld, **joint)
        return h

    def _self_attention(self, i, q, xt, h, shift, scale, Bn, N, ld, akv=None, ha=None, tag='sa_'):
        """Block i's pre-norm + modulate -> QKV GEMM with head split (and qk-norm) -> attention over the Bn samples of xt [Bn*N, D]:
        bf16 [Bn*N, H * attn_out_dim].  Three forms: the plain sequence through the operand h; with `ha` [Bn, NA, D] the joint
        sequence whose rows [N, NA) of every sample hold the appended tokens (the norm writes rows < N only, all NA rows are keys,
        the N x rows are queries); with `akv` the appended rows' K / V^T cached per layer (_appended_kv)."""
        ws, D, H = self._ws, self.embed_dim, self.num_heads
        NA, kv = N, None
        if akv is not None:            # queries / keys / values of the x tokens only (Bn * N rows instead of Bn * NA: the appended
            sa_k, sa_vt, NA = akv      # part of the joint sequence never changes): their K / V^T land in front of the cached rows
            kv = (sa_k[i], sa_vt[i])
        if ha is not None:
            NA = ha.shape[1]
            h = self._norm_mod(xt, ha, q['n1'], shift, scale, N, ld, rows_in=N, rows_out=NA)
        else:
            self._norm_mod(xt, h, q['n1'], shift, scale, N, ld)
        return self_attention_hip(ws, tag, h, Bn, NA, D, H, q['qkv_w'], q['qkv_b'], q['qn'], q['kn'], nq=N, kv=kv)

    def _self_attention_block(self, i, q, mi, ld, cc, xt, h, xb, Bn, N, akv, ha, twins):
        """x += gate * proj(self-attention(norm-modulate(x))) on the fp32 stream xt, with its bf16 copy xb for the cross-attention
        query.  Samples of the zero-context fold have a constant cross-attention output (prepare_context): it rides on this epilogue
        as a per-sample row.  `twins`: the caller's cfg_twins statement (DiT_TriLatent's block-0 dedup; nothing here)."""
        D = self.embed_dim
        ao = self._self_attention(i, q, xt, h, mi, mi[:, D:], Bn, N, ld, akv, ha)
        ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt, xb, gate=mi[:, 2 * D:], gate_rows=N, gate_ld=ld,
                 res_bias=cc['const'][i] if cc.get('fold', 0) else None, res_bias_ld=D)

    def _cross_attend(self, i, q, cc, xb_c, qc, oc_c, b0, Bc, N, fuse_cq):
        """Cross-attention of the Bc conditional samples from sample b0 on (xb_c: their bf16 rows; no pre-norm, no gate; reference
        :318) over the prompt's cached K / V^T -> oc_c: to_q GEMM with head split, the block's q-norm (None without) inside its
        epilogue when `fuse_cq` or as a pass of its own, then attention."""
        H, cqn = self.num_heads, q['cqn']
        ops.gemm(xb_c, q['cq_w'], None, ops.EPI_HEADS, qc, M=Bc * N, tokens=N, tok_pad=N, heads=H, head_dim=64,
                 head_norm0=cqn if fuse_cq else None)
        if cqn is not None and not fuse_cq:
            ops.rmsnorm_heads(qc, cqn, Bc * H * N, 64)
        ops.attention(qc, cc['k'][i, b0:], cc['vt'][i, b0:], oc_c, Bc, H, N, N, cc['Lc'], cc['lpad'], 64)

    def _fc1(self, probe, i, hb, q, f1):
        """Block i's MLP fc1 GEMM (erf-GELU epilogue; MX-FP8 in and out when hb is an ops.MX).  `probe`: bench.py's `_fc1_probe`
        measurement hook {'layer', 'events', 'max'}: HIP events on the launch stream around this one GEMM of that layer, inside the real step."""
        if probe is not None and i == probe['layer'] and len(probe['events']) < probe['max']:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._fc1_launch(hb, q, f1)
            e1.record()
            probe['events'].append((e0, e1))
        else:
            self._fc1_launch(hb, q, f1)

    @staticmethod
    def _fc1_launch(hb, q, f1):
        if isinstance(hb, ops.MX):
            ops.gemm_mx(hb, q['fc1_w'], q['fc1_b'], ops.EPI_GELU_ERF, f1.q, out_scale=f1.s)
        else:
            ops.gemm(hb, q['fc1_w'], q['fc1_b'], ops.EPI_GELU_ERF, f1)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x, timesteps=None, context=None, y=None, get_attr='', context_cache=None, in_scale=None, **kwargs):
        """float32 [B, C*3, H, W] (the point-cloud variant: [B, N, C]).  context_cache: what prepare_context(context) returned;
        in_scale: a denoiser wrapper's c_in, one factor per network row; further keywords are the class's own (DiT_TriLatent:
        mod_cache, cfg_twins) and otherwise ignored."""
        if get_attr != '':
            return getattr(self, get_attr)
        assert context is not None or context_cache is not None
        if not x.is_cuda:
            raise RuntimeError(f"ln3diff_amd.{type(self).__name__} runs on the HIP device only (no CPU fallback)")
        self._ensure_packed(x.device)
        P, ws = self._packed, self._ws
        cc = context_cache if context_cache is not None else self.prepare_context(context)
        self._check_prepared(cc, 'prepare_context')
        D, H = self.embed_dim, self.num_heads
        Bn, Bx = timesteps.shape[0], x.shape[0]
        assert cc['Bn'] == Bn
        N = self._num_tokens(x)
        M = Bn * N

        tsilu, tsum = self._conditioning(timesteps, cc, kwargs)
        mod_of, ld = self._modulation(tsilu, Bn, kwargs)
        xt = self._embed_tokens(x, in_scale, Bx, Bn, N)
        akv, ha = self._appended(cc, Bn, N)

        q0 = P['blocks'][0]
        mx = isinstance(q0['fc1_w'], ops.MX)                   # MXFP8 operands of QKV / fc1 (norm+modulate output) and fc2 (GELU output)
        h = ops.MX(ws.get('hq', (M, D), torch.uint8), ws.get('hqs', (M, D // 32), torch.uint8)) if mx else ws.get('h', (M, D), torch.bfloat16)
        xb = ws.get('xb', (M, D), torch.bfloat16)
        qc = ws.get('qc', (Bn, H, N, 64), torch.bfloat16)
        oc = ws.get('oc', (M, H * 64), torch.bfloat16)
        if mx:
            F = q0['fc1_w'].q.shape[0]
            f1 = ops.MX(ws.get('f1q', (M, F), torch.uint8), ws.get('f1s', (M, F // 32), torch.uint8))
        else:
            f1 = ws.get('f1', (M, q0['fc1_w'].shape[0]), torch.bfloat16)
        fc2 = ops.gemm_mx if isinstance(f1, ops.MX) else ops.gemm
        probe = getattr(self, '_fc1_probe', None)
        fold = cc.get('fold', 0)                               # samples with a constant cross-attention output (_fold_uc)
        r0, b0 = self._conditioned(fold, N)
        Bc = Bn - fold
        xt_c, xb_c, oc_c = xt[r0:], xb[r0:], oc[r0:]
        fuse_cq = q0['cqn'] is not None and ops.heads_norm_fusable(Bc * N, H * 64, N, 64)
        twins = bool(kwargs.get('cfg_twins', False)) and 2 * Bx == Bn and ld == 0
        for i, q in enumerate(P['blocks']):
            mi = mod_of(i)                                     # [Bn or 1, 6D..]: shift / scale / gate of the attention, then of the MLP
            self._self_attention_block(i, q, mi, ld, cc, xt, h, xb, Bn, N, akv, ha, twins)
            self._cross_attend(i, q, cc, xb_c, qc, oc_c, b0, Bc, N, fuse_cq)
            ops.gemm(oc_c, q['co_w'], q['co_b'], ops.EPI_GATE_RES, xt_c, M=Bc * N)
            self._fc1(probe, i, self._norm_mod(xt, h, q['n2'], mi[:, 3 * D:], mi[:, 4 * D:], N, ld), q, f1)
            fc2(f1, q['fc2_w'], q['fc2_b'], ops.EPI_GATE_RES, xt, gate=mi[:, 5 * D:], gate_rows=N, gate_ld=ld)
        return self._output(xt, tsum, mod_of, ld, Bn, N)
