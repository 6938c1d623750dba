"""DiT_TriLatent (text -> tri-plane latent denoiser) on the HIP kernels.

Same constructor / forward surface and state-dict keys as the reference's
dit/dit_trilatent.py:22-143 (`DiT_models[arch](input_size, num_classes, learn_sigma, in_channels,
context_dim, roll_out, vit_blk)`, `forward(x, timesteps, context, y=None, get_attr='', **kw)`
returning float32 [B, C*3, H, W]); the forward pass is a fixed sequence of HIP launches:

  per forward : timestep sin/cos -> 2 GEMMs (SiLU fused) -> ONE GEMM for every block's adaLN (depth*6D+2D cols)
                caption MLP (2 GEMMs, tanh-GELU fused) -> per-block K/V^T of the context (cacheable per prompt)
                patch-embed(+pos-embed, + optional EDM c_in scale)
  per block   : LN+modulate -> QKV GEMM (head-split epilogue, V^T emitted) -> fused attention ->
                proj GEMM (gate*out + residual epilogue, bf16 copy of x) -> to_q GEMM -> fused cross
                attention -> to_out GEMM (residual epilogue) -> LN+modulate -> fc1 GEMM (erf-GELU epilogue)
                -> fc2 GEMM (gate*out + residual epilogue)
  final       : LN+modulate+Linear(D->p*p*C)+unpatchify in one kernel.
The residual stream, LN statistics, softmax and all accumulators are fp32; GEMM operands are bf16.
set_matmul_precision('mxfp8') (opt-in; no reference counterpart) runs the QKV, fc1 and fc2 GEMMs of every block on MX-FP8 operands
(include/ln3d_mx.h): the two LN+modulate kernels write MXFP8, fc1's GELU epilogue writes MXFP8 for fc2; everything else stays bf16.
"""
import os

import torch
import torch.nn as nn

from .. import ops, _cache
from .dit_models_xformers import (CaptionEmbedder, DiTBlock, FinalLayer, PatchEmbed, T2IFinalLayer,  # noqa: F401
                                  TextCondDiTBlock, TimestepEmbedder, Workspace, bf16, f32,
                                  get_2d_sincos_pos_embed, self_attention_hip, pack_block, pack_block_mx, pack_caption)


class DiT(_cache.PackedWeights, nn.Module):
    """Base container (reference dit/dit_models_xformers.py:681-835)."""

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16,
                 mlp_ratio=4.0, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3,
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
        self.x_embedder = PatchEmbed(input_size, patch_size, in_channels, hidden_size, bias=True)
        self.t_embedder = TimestepEmbedder(hidden_size)
        self.y_embedder = None
        self.clip_text_proj = CaptionEmbedder(context_dim, hidden_size) if context_dim is not None else None
        self.context_dim = context_dim
        self.pos_embed = nn.Parameter(torch.zeros(1, self.x_embedder.num_patches, hidden_size), requires_grad=False)
        self.blocks = nn.ModuleList([vit_blk(hidden_size=hidden_size, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                             context_dim=context_dim) for _ in range(depth)])
        self.final_layer = final_layer_blk(hidden_size, patch_size, self.out_channels)
        self.initialize_weights()
        self._ws = None

    def initialize_weights(self):
        # same rules as the reference (:777-819); sampling uses loaded / synthetic weights anyway
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
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


class DiT_TriLatent(DiT):
    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16,
                 mlp_ratio=4, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3,
                 mixed_prediction=True, context_dim=False, roll_out=False, vit_blk=DiTBlock,
                 final_layer_blk=FinalLayer):
        super().__init__(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_ratio,
                         class_dropout_prob, num_classes, learn_sigma, mixing_logit_init, mixed_prediction,
                         context_dim, roll_out, vit_blk, final_layer_blk)
        assert self.roll_out
        self.init_PE_3D_aware()

    def init_PE_3D_aware(self):
        L = self.x_embedder.num_patches
        D = self.embed_dim
        pe = get_2d_sincos_pos_embed(D, (self.plane_n, L)).reshape(self.plane_n * L, D)
        self.pos_embed = nn.Parameter(torch.from_numpy(pe).float().unsqueeze(0), requires_grad=False)

    # ------------------------------------------------------------------ matmul precision
    MATMUL_PRECISIONS = ('bf16', 'mxfp8')
    _matmul_precision = 'bf16'

    def set_matmul_precision(self, precision):
        """'bf16' (default: the reference's numerics up to bf16 GEMM operands) or 'mxfp8': the QKV, fc1 and fc2 GEMMs of every block
        on OCP MXFP8 operands (e4m3 elements, one E8M0 scale per 32 values along K), quantized on the device from the fp32 master
        weights when the model is packed.  Only the active precision's operands are kept; a change drops the packed copies."""
        if precision not in self.MATMUL_PRECISIONS:
            raise ValueError(f"matmul precision {precision!r}: expected one of {self.MATMUL_PRECISIONS}")
        if precision != 'bf16' and type(self).forward is not DiT_TriLatent.forward:
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

    # ------------------------------------------------------------------ context helpers shared by every denoiser of the family
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

    _uc_first = True                   # the unconditional CFG samples lead the batch: VanillaCFG's [uc, c] order

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

    # ------------------------------------------------------------------ context (constant per prompt)
    def prepare_context(self, context):
        """clip_text_proj + every block's cross-attention K / V^T.  They depend only on the prompt, so the
        samplers call this once per run instead of once per step (the reference recomputes them 250x)."""
        if isinstance(context, dict):
            context = context['crossattn']
        self._ensure_packed(context.device)
        Bn, Lc, _ = context.shape
        cp = self._caption_mlp(context, 'c', self._ws.get('ctx_p', (Bn * Lc, self.embed_dim), torch.bfloat16))
        k_all, vt_all, lpad = self._cross_kv(cp, Bn, Lc)
        # K copy whose 64 head dims are stored in the 16-group order [0-3, 8-11, 4-7, 12-15]: the order in which the query
        # projection's accumulators hand q to the MFMA when cross-attention runs inside that GEMM (LN3D_EPI_CROSS_ATTN)
        kp_all = k_all[..., ops.vt_key_order(64, context.device)].contiguous()
        return self._finish_context({'k': k_all, 'kp': kp_all, 'vt': vt_all, 'Lc': Lc, 'lpad': lpad, 'Bn': Bn}, context)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def _timestep_modulation(self, timesteps, mod, tag):
        """t -> sincos(256) -> MLP -> SiLU -> adaLN Linear of every block + final layer, all rows of `timesteps` at once."""
        P, ws, D = self._packed, self._ws, self.embed_dim
        R = timesteps.shape[0]
        t32 = timesteps.to(device=mod.device, dtype=torch.float32).contiguous()
        tf = ws.get(tag + 'tfreq', (R, 256), torch.bfloat16)
        ops.timestep_embedding(t32, tf, R, 256)
        th = ws.get(tag + 'th', (R, D), torch.bfloat16)
        ops.gemm(tf, P['t_w0'], P['t_b0'], ops.EPI_SILU, th)
        temb = ws.get(tag + 'temb', (R, D), torch.float32)
        tsilu = ws.get(tag + 'tsilu', (R, D), torch.bfloat16)
        ops.gemm(th, P['t_w2'], P['t_b2'], ops.EPI_F32_SILU, temb, tsilu)
        ops.gemm(tsilu, P['ada_w'], P['ada_b'], ops.EPI_F32, mod)

    MODCACHE_MAX_BYTES = 4 << 30

    def prepare_timesteps(self, t_table):
        """t_table [n_steps, Bn] (the sampler's whole schedule): the timestep-only part of the network (embedder MLP and the
        [24*6+2]*D-wide adaLN projection, 306 MB of weights at DiT-L/2) is evaluated for all steps in ONE pass instead of
        re-streaming those weights every step.  Returns the cache for forward(..., mod_cache=(cache, step)): {'mod': [n * rows,
        nmod] f32, 'rows': rows}.  When every sample of a step has the same timestep (all samplers of this path) ONE row per step is
        kept (rows = 1: 150 MB at 250 steps instead of 2.4 GB at network batch 16) and the kernels read it with a sample stride of 0.
        A schedule whose cache would exceed MODCACHE_MAX_BYTES returns None: the caller runs the modulation GEMMs per step.
        The rows are storage of the returned cache's own (one allocation per sampling run): a second prepared schedule, of the same
        length or not, leaves this one alone."""
        dev = next(self.parameters()).device
        self._ensure_packed(dev)
        n, Bn = t_table.shape
        nmod = self.depth * 6 * self.embed_dim + 2 * self.embed_dim
        rows = 1 if bool((t_table == t_table[:, :1]).all()) else Bn
        if n * rows * nmod * 4 > self.MODCACHE_MAX_BYTES:
            return None
        mod_all = torch.empty(n * rows, nmod, dtype=torch.float32, device=dev)
        self._timestep_modulation(t_table[:, :rows].reshape(-1).to(dev), mod_all, 'ma')
        return {'mod': mod_all, 'rows': rows, 'epoch': self._packed['epoch']}

    def _check_prepared(self, cache, maker):
        """A prepared context / timestep cache holds values computed from the weights of ONE epoch (ln3diff_amd/_cache.py); after any
        weight change - the epoch is global, so a load into another module counts - it is refused instead of being mixed with the
        re-packed blocks.  One host integer compare: no device read, nothing inside a captured graph."""
        if cache.get('epoch') != self._packed['epoch']:
            raise RuntimeError(f"{type(self).__name__}: this cache was made by {maker}() before the weights changed (weights epoch "
                               f"{cache.get('epoch')}, now {self._packed['epoch']}); call {maker}() again")

    def forward(self, x, timesteps=None, context=None, y=None, get_attr='', context_cache=None, in_scale=None,
                mod_cache=None, **kwargs):
        if get_attr != '':
            return getattr(self, get_attr)
        assert context is not None or context_cache is not None
        if not x.is_cuda:
            raise RuntimeError("ln3diff_amd.DiT_TriLatent runs on the HIP device only (no CPU fallback)")
        dev = x.device
        self._ensure_packed(dev)
        P, ws = self._packed, self._ws
        D, H, depth = self.embed_dim, self.num_heads, self.depth
        Bn = timesteps.shape[0]
        Bx = x.shape[0]
        S, p, C = self.input_size, self.patch_size, self.in_channels
        L = (S // p) ** 2
        N = 3 * L
        M = Bn * N
        cc = context_cache if context_cache is not None else self.prepare_context(context)
        self._check_prepared(cc, 'prepare_context')
        assert cc['Bn'] == Bn

        # -- timestep embedding and all adaLN modulations (or the rows prepared for the whole schedule)
        nmod = depth * 6 * D + 2 * D
        ld = nmod                                              # stride between the samples' modulation rows
        if mod_cache is not None:
            mc, step = mod_cache
            self._check_prepared(mc, 'prepare_timesteps')
            rows = mc['rows']
            assert rows in (1, Bn) and mc['mod'].shape[1] == nmod
            mod = mc['mod'][step * rows:(step + 1) * rows]
            ld = nmod if rows == Bn else 0                     # one shared row per step: every sample reads row 0
        else:
            mod = ws.get('mod', (Bn, nmod), torch.float32)
            self._timestep_modulation(timesteps, mod, 'm')

        # -- tokens
        xt = ws.get('x', (M, D), torch.float32)
        ops.patch_embed(x.contiguous().float(), in_scale, P['pe_w'], P['pe_b'], P['pos'], xt, Bx, Bn, C, S, p, D)
        hb = ws.get('h', (M, D), torch.bfloat16)
        xb = ws.get('xb', (M, D), torch.bfloat16)
        qc = ws.get('qc', (Bn, H, N, 64), torch.bfloat16)
        oc = ws.get('oc', (M, H * 64), torch.bfloat16)
        mx = P['precision'] == 'mxfp8'
        if mx:                                                 # MXFP8 operands of QKV / fc1 (LN+modulate output) and fc2 (GELU output)
            F = P['blocks'][0]['fc1_w'].q.shape[0]
            hq = ops.MX(ws.get('hq', (M, D), torch.uint8), ws.get('hqs', (M, D // 32), torch.uint8))
            f1 = ops.MX(ws.get('f1q', (M, F), torch.uint8), ws.get('f1s', (M, F // 32), torch.uint8))
        else:
            f1 = ws.get('f1', (M, P['blocks'][0]['fc1_w'].shape[0]), torch.bfloat16)

        def norm_mod(rows, shift, scale):
            """LN + adaLN modulate of xt[:rows] -> the QKV / fc1 operand (bf16, or MXFP8 in mxfp8 mode)"""
            if mx:
                ops.norm_modulate_mx(xt[:rows], hq.rows(0, rows), rows, D, kind=0, eps=1e-6, shift=shift, scale=scale, mod_rows=N, mod_ld=ld)
                return hq.rows(0, rows)
            ops.norm_modulate(xt[:rows], hb[:rows], rows, D, kind=0, eps=1e-6, shift=shift, scale=scale, mod_rows=N, mod_ld=ld)
            return hb[:rows]

        probe = getattr(self, '_fc1_probe', None)
        fused_cross = N % 192 == 0 and (H * 64) % 256 == 0 and cc['Lc'] <= 96 and 'kp' in cc
        fold = cc.get('fold', 0)
        r0 = fold * N                                          # first token row that still runs the cross-attention GEMMs
        # r5: under classifier-free guidance the two halves of the network batch ([uc ; c]: the same latents, timestep and input scale
        # twice) are IDENTICAL until the first cross-attention separates them, so block 0's norm, QKV projection and self-attention run
        # on one half and its output projection is applied to both halves' residual rows - exact algebra (summation order aside), with or
        # without the zero-context fold.  `cfg_twins=True` is the caller's statement that sample b and sample b + Bn / 2 enter alike (the
        # samplers fill t and c_in with one constant per step; checking it here would be a device read per step); every sample must also
        # share its modulation row (mod_ld == 0).
        half = Bn // 2
        dedup0 = bool(kwargs.get('cfg_twins', False)) and 2 * Bx == Bn and ld == 0 and fold in (0, half)
        for i, q in enumerate(P['blocks']):
            o6 = i * 6 * D
            sh_a, sc_a, g_a = mod[:, o6:], mod[:, o6 + D:], mod[:, o6 + 2 * D:]
            sh_m, sc_m, g_m = mod[:, o6 + 3 * D:], mod[:, o6 + 4 * D:], mod[:, o6 + 5 * D:]
            if i == 0 and dedup0:
                Mh = half * N
                ao = self_attention_hip(ws, 'sa0_', norm_mod(Mh, sh_a, sc_a), half, N, D, H, q['qkv_w'], q['qkv_b'])
                # first half: with the fold these are the unconditional rows (+ their constant cross-attention, no bf16 copy needed)
                ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt[:Mh], None if fold else xb[:Mh], gate=g_a, gate_rows=N,
                         gate_ld=ld, res_bias=cc['const'][i] if fold else None, res_bias_ld=D)
                ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt[Mh:], xb[Mh:], gate=g_a, gate_rows=N, gate_ld=ld)
            else:
                ao = self_attention_hip(ws, 'sa_', norm_mod(M, sh_a, sc_a), Bn, N, D, H, q['qkv_w'], q['qkv_b'])
                # samples [0, fold) have a constant cross-attention output (prepare_context): it rides on this epilogue as a per-sample row
                ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt, xb, gate=g_a, gate_rows=N, gate_ld=ld,
                         res_bias=cc['const'][i] if fold else None, res_bias_ld=D)
            # cross attention on x (no pre-norm, no gate; reference :318) for the remaining samples
            if fused_cross:     # q projection + attention over the cached text context in ONE kernel (q stays in registers)
                ops.gemm(xb[r0:], q['cq_w'], None, ops.EPI_CROSS_ATTN, oc[r0:], cc['kp'][i][fold:], cc['vt'][i][fold:], M=M - r0, tokens=N, heads=H,
                         head_dim=64, ctx_keys=cc['Lc'], ctx_pad=cc['lpad'], ctx_scale=64 ** -0.5)
            else:               # shapes the fused epilogue does not take (tokens % 192, heads * 64 % 256, more than 96 context keys)
                ops.gemm(xb[r0:], q['cq_w'], None, ops.EPI_HEADS, qc, M=M - r0, tokens=N, tok_pad=N, heads=H, head_dim=64)
                ops.attention(qc, cc['k'][i][fold:], cc['vt'][i][fold:], oc[r0:], Bn - fold, H, N, N, cc['Lc'], cc['lpad'], 64)
            ops.gemm(oc[r0:], q['co_w'], q['co_b'], ops.EPI_GATE_RES, xt[r0:])
            self._fc1(probe, i, norm_mod(M, sh_m, sc_m), q, f1)
            if mx:
                ops.gemm_mx(f1, q['fc2_w'], q['fc2_b'], ops.EPI_GATE_RES, xt, gate=g_m, gate_rows=N, gate_ld=ld)
            else:
                ops.gemm(f1, q['fc2_w'], q['fc2_b'], ops.EPI_GATE_RES, xt, gate=g_m, gate_rows=N, gate_ld=ld)

        of = depth * 6 * D
        out = torch.empty(Bn, self.out_channels * 3, S, S, dtype=torch.float32, device=dev)
        ops.final_layer(xt, mod[:, of:], mod[:, of + D:], ld, None, None, P['fin_w'], P['fin_b'], out, Bn,
                        self.out_channels, S, p, D)
        return out


def DiT_XL_2(**kwargs):
    return DiT_TriLatent(depth=28, hidden_size=1152, patch_size=2, num_heads=16, **kwargs)


def DiT_L_2(**kwargs):
    return DiT_TriLatent(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_B_2(**kwargs):
    return DiT_TriLatent(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def DiT_B_1(**kwargs):          # reference dit_trilatent.py:296-301: no spatial compression, 3 x 1024 tokens per sample
    return DiT_TriLatent(depth=12, hidden_size=768, patch_size=1, num_heads=12, **kwargs)


def _pixart(name):
    def make(**kwargs):               # the PixArt-style T23D class lives with the I23D block machinery it runs on (import cycle otherwise)
        from . import dit_i23d
        return getattr(dit_i23d, name)(**kwargs)
    make.__name__ = name
    return make


DiT_models = {'DiT-XL/2': DiT_XL_2, 'DiT-L/2': DiT_L_2, 'DiT-B/2': DiT_B_2, 'DiT-B/1': DiT_B_1,
              'DiT-PixelArt-L/2': _pixart('DiT_L_TriLatent_Pixelart_2'), 'DiT-PixelArt-B/2': _pixart('DiT_B_TriLatent_Pixelart_2')}
