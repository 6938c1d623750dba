"""DiT_TriLatent (text -> tri-plane latent denoiser) on the HIP kernels.

Same constructor / forward surface and state-dict keys as the reference's
dit/dit_trilatent.py:22-143 (`DiT_models[arch](input_size, num_classes, learn_sigma, in_channels,
context_dim, roll_out, vit_blk)`, `forward(x, timesteps, context, y=None, get_attr='', **kw)`
returning float32 [B, C*3, H, W]).  The class derives from the family's base (dit_base.DiT: constructor, pack, prompt helpers and the
ONE forward template with its block loop) and states what is its own: the caption MLP of the text tokens, every block's and the
FinalLayer's adaLN in one GEMM, prepare_timesteps (that GEMM for a whole schedule), the cfg_twins dedup of block 0, the fused
cross-attention epilogue with its permuted key copy, and the MX-FP8 operands.  Per forward: timestep sin/cos -> 2 GEMMs (SiLU fused)
-> ONE GEMM for every block's adaLN (depth*6D+2D cols), patch-embed (+pos-embed, + optional EDM c_in scale), the base's block loop,
and LN+modulate+Linear(D->p*p*C)+unpatchify in one kernel; per prompt: caption MLP (2 GEMMs, tanh-GELU fused) -> per-block K/V^T.
set_matmul_precision('mxfp8') (opt-in; no reference counterpart) runs the QKV, fc1 and fc2 GEMMs of every block on MX-FP8 operands
(include/ln3d_mx.h): the two LN+modulate kernels write MXFP8, fc1's GELU epilogue writes MXFP8 for fc2; everything else stays bf16.
"""
import torch

from .. import ops
from .dit_base import DiT
from .dit_models_xformers import (CaptionEmbedder, DiTBlock, FinalLayer, PatchEmbed, T2IFinalLayer,  # noqa: F401
                                  TextCondDiTBlock, TimestepEmbedder, Workspace)
from .dit_i23d import DiT_L_TriLatent_Pixelart_2, DiT_B_TriLatent_Pixelart_2


class DiT_TriLatent(DiT):
    PACK_PRECISIONS = ('bf16', 'mxfp8')

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

    # ------------------------------------------------------------------ timestep-only part: every block's adaLN + the final layer's, one GEMM
    MODCACHE_MAX_BYTES = 4 << 30

    @torch.no_grad()
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
        P = self._ensure_packed(dev)
        n, Bn = t_table.shape
        nmod = self.depth * 6 * self.embed_dim + 2 * self.embed_dim
        rows = 1 if bool((t_table == t_table[:, :1]).all()) else Bn
        if n * rows * nmod * 4 > self.MODCACHE_MAX_BYTES:
            return None
        mod_all = torch.empty(n * rows, nmod, dtype=torch.float32, device=dev)
        _, tsilu = self._timestep_embed(t_table[:, :rows].reshape(-1).to(dev), 'ma', silu=True)
        ops.gemm(tsilu, P['ada_w'], P['ada_b'], ops.EPI_F32, mod_all)
        return {'mod': mod_all, 'rows': rows, 'epoch': P['epoch']}

    # ------------------------------------------------------------------ the hooks of the forward template (dit_base.DiT.forward)
    def _conditioning(self, timesteps, cc, opts):
        """SiLU(t_embedder(t)), the adaLN GEMM's operand - or nothing, with the rows prepared for the whole schedule"""
        if opts.get('mod_cache') is not None:
            return None, None
        return self._timestep_embed(timesteps, 'm', silu=True)[1], None

    def _modulation(self, tsilu, Bn, opts):
        """(i -> the modulation rows from block i's slice on; i = depth: the final layer's, row stride): one GEMM for every block and
        the final layer, or step `step` of mod_cache = (prepare_timesteps(...), step) - ONE shared row (stride 0) when it holds one."""
        P, D = self._packed, self.embed_dim
        nmod = self.depth * 6 * D + 2 * D
        ld = nmod                                              # stride between the samples' modulation rows
        if tsilu is None:
            mc, step = opts['mod_cache']
            self._check_prepared(mc, 'prepare_timesteps')
            rows = mc['rows']
            assert rows in (1, Bn) and mc['mod'].shape[1] == nmod
            mod = mc['mod'][step * rows:(step + 1) * rows]
            ld = nmod if rows == Bn else 0                     # one shared row per step: every sample reads row 0
        else:
            mod = self._ws.get('mod', (Bn, nmod), torch.float32)
            ops.gemm(tsilu, P['ada_w'], P['ada_b'], ops.EPI_F32, mod)
        return (lambda i: mod[:, i * 6 * D:]), ld

    def _self_attention_block(self, i, q, mi, ld, cc, xt, h, xb, Bn, N, akv, ha, twins):
        # r5: under classifier-free guidance the two halves of the network batch ([uc ; c]: the same latents, timestep and input scale
        # twice) are IDENTICAL until the first cross-attention separates them, so block 0's norm, QKV projection and self-attention run
        # on one half and its output projection is applied to both halves' residual rows - exact algebra (summation order aside), with or
        # without the zero-context fold.  `cfg_twins=True` is the caller's statement that sample b and sample b + Bn / 2 enter alike (the
        # samplers fill t and c_in with one constant per step; checking it here would be a device read per step); every sample must also
        # share its modulation row (mod_ld == 0: `twins` says both).
        half, fold = Bn // 2, cc.get('fold', 0)
        if not (i == 0 and twins and fold in (0, half)):
            return super()._self_attention_block(i, q, mi, ld, cc, xt, h, xb, Bn, N, akv, ha, twins)
        D, Mh = self.embed_dim, half * N
        ao = self._self_attention(i, q, xt[:Mh], h.rows(0, Mh) if isinstance(h, ops.MX) else h[:Mh], mi, mi[:, D:], half, N, ld,
                                  tag='sa0_')
        # first half: with the fold these are the unconditional rows (+ their constant cross-attention, no bf16 copy needed)
        ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt[:Mh], None if fold else xb[:Mh], gate=mi[:, 2 * D:], gate_rows=N,
                 gate_ld=ld, res_bias=cc['const'][i] if fold else None, res_bias_ld=D)
        ops.gemm(ao, q['proj_w'], q['proj_b'], ops.EPI_GATE_RES, xt[Mh:], xb[Mh:], gate=mi[:, 2 * D:], gate_rows=N, gate_ld=ld)

    def _cross_attend(self, i, q, cc, xb_c, qc, oc_c, b0, Bc, N, fuse_cq):
        H = self.num_heads
        if not (N % 192 == 0 and (H * 64) % 256 == 0 and cc['Lc'] <= 96 and 'kp' in cc):
            # shapes the fused epilogue does not take (tokens % 192, heads * 64 % 256, more than 96 context keys)
            return super()._cross_attend(i, q, cc, xb_c, qc, oc_c, b0, Bc, N, fuse_cq)
        # q projection + attention over the cached text context in ONE kernel (q stays in registers)
        ops.gemm(xb_c, q['cq_w'], None, ops.EPI_CROSS_ATTN, oc_c, cc['kp'][i, b0:], cc['vt'][i, b0:], M=Bc * N, tokens=N, heads=H,
                 head_dim=64, ctx_keys=cc['Lc'], ctx_pad=cc['lpad'], ctx_scale=64 ** -0.5)

    def _output(self, xt, tsum, mod_of, ld, Bn, N):
        """FinalLayer (LN, its adaLN slice of the modulation rows, Linear) + unpatchify -> [Bn, 3*C_out, S, S]"""
        P, D, S = self._packed, self.embed_dim, self.input_size
        fin = mod_of(self.depth)
        out = torch.empty(Bn, self.out_channels * 3, S, S, dtype=torch.float32, device=xt.device)
        ops.final_layer(xt, fin, fin[:, D:], ld, None, None, P['fin_w'], P['fin_b'], out, Bn, self.out_channels, S, self.patch_size, D)
        return out


def DiT_XL_2(**kwargs):
    return DiT_TriLatent(depth=28, hidden_size=1152, patch_size=2, num_heads=16, **kwargs)


def DiT_L_2(**kwargs):
    return DiT_TriLatent(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def DiT_B_2(**kwargs):
    return DiT_TriLatent(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def DiT_B_1(**kwargs):          # reference dit_trilatent.py:296-301: no spatial compression, 3 x 1024 tokens per sample
    return DiT_TriLatent(depth=12, hidden_size=768, patch_size=1, num_heads=12, **kwargs)


DiT_models = {'DiT-XL/2': DiT_XL_2, 'DiT-L/2': DiT_L_2, 'DiT-B/2': DiT_B_2, 'DiT-B/1': DiT_B_1,
              # the PixArt-style T23D class lives with the PixArt machinery it runs on (dit_i23d.py)
              'DiT-PixelArt-L/2': DiT_L_TriLatent_Pixelart_2, 'DiT-PixelArt-B/2': DiT_B_TriLatent_Pixelart_2}
