"""Thin torch-tensor wrappers over the C ABI (include/ln3d.h).  torch is used for device
memory and streams only; every op below is a HIP kernel launch on torch's current stream."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import (EPI_F32, EPI_BF16, EPI_GELU_ERF, EPI_GELU_TANH, EPI_SILU, EPI_GATE_RES,  # noqa: F401
                   EPI_HEADS, EPI_F32_SILU, EPI_QUICK_GELU, EPI_CROSS_ATTN)


_NEED_DEVICE = "ln3diff_amd ops need device tensors (no CPU fallback exists)"


def _p(t):
    """the address of a device tensor (None stays NULL): the one place a tensor becomes a kernel argument, so the one place that refuses
    a host tensor"""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(_NEED_DEVICE)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def reload_env():
    """Re-read the library's one measurement switch (LN3D_GEMM_TILE, the tile override the tests sweep: parsed once per process)."""
    L.lib().ln3d_reload_env()


def gemm(x, w, bias, epilogue, out0, out1=None, out2=None, *, M=None, ldo=None, gate=None, gate_rows=1,
         gate_ld=0, tokens=0, tok_pad=0, heads=0, head_dim=0, transpose_mask=0, head_dim_pad=0, ctx_keys=0, ctx_pad=0,
         ctx_scale=0.0, head_norm0=None, head_norm1=None, head_norm_eps=1e-5, res_bias=None, res_bias_ld=0):
    """out = epi(x[M,K] @ w[N,K]^T + bias).  x, w bf16 (row stride = shape[-1])."""
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    a = L.GemmArgs()
    K = w.shape[1]
    if x.shape[-1] != K:
        raise ValueError(f"gemm: activation has {x.shape[-1]} input features, the weight expects {K}")
    a.X, a.ldx, a.W, a.ldw = _p(x), x.stride(-2) if x.dim() > 1 else K, _p(w), w.stride(0)
    a.bias = _p(bias)
    a.M = int(M if M is not None else x.numel() // K)
    a.N, a.K = w.shape[0], K
    a.epilogue = epilogue
    a.out0, a.out1, a.out2 = _p(out0), _p(out1), _p(out2)
    a.ldo = int(ldo if ldo is not None else w.shape[0])
    a.gate, a.gate_rows, a.gate_ld = _p(gate), gate_rows, gate_ld
    a.tokens, a.tok_pad, a.heads, a.head_dim, a.transpose_mask = tokens, tok_pad, heads, head_dim, transpose_mask
    a.head_dim_pad = head_dim_pad
    a.ctx_keys, a.ctx_pad, a.ctx_scale = ctx_keys, ctx_pad, float(ctx_scale)
    a.head_norm0, a.head_norm1, a.head_norm_eps = _p(head_norm0), _p(head_norm1), float(head_norm_eps)
    a.res_bias, a.res_bias_ld = _p(res_bias), int(res_bias_ld)
    L.check(L.lib().ln3d_gemm_bf16(a, _stream()), "gemm")


class MX:
    """An MXFP8 matrix [R, K] (include/ln3d_mx.h): q e4m3 bytes [R, K] (torch.uint8) and s E8M0 scale bytes [R, K / 32] (torch.uint8),
    both row-major and contiguous."""
    __slots__ = ('q', 's')

    def __init__(self, q, s):
        self.q, self.s = q, s

    @staticmethod
    def empty(R, K, device):
        return MX(torch.empty(R, K, dtype=torch.uint8, device=device), torch.empty(R, K // 32, dtype=torch.uint8, device=device))

    def rows(self, r0, r1=None):
        """row slice [r0, r1) (views)"""
        return MX(self.q[r0:r1], self.s[r0:r1])


def quantize_mx(x, out=None):
    """x [R, K] f32 or bf16 (row stride = x.stride(0)) -> MX (one E8M0 scale per 32 values, OCP e4m3 elements)."""
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2 and x.stride(1) == 1
    R, K = x.shape
    out = out if out is not None else MX.empty(R, K, x.device)
    L.check(L.lib().ln3d_quantize_mx(_p(x), x.dtype == torch.bfloat16, x.stride(0), R, K, _p(out.q), out.q.stride(0), _p(out.s),
                                     out.s.stride(0), _stream()), "quantize_mx")
    return out


def gemm_mx(x, w, bias, epilogue, out0, out1=None, out2=None, *, M=None, ldo=None, out_scale=None, gate=None, gate_rows=1, gate_ld=0,
            tokens=0, tok_pad=0, heads=0, head_dim=0, transpose_mask=0, head_dim_pad=0):
    """out = epi(deq(x)[M,K] @ deq(w)[N,K]^T + bias) on the MX-FP8 MFMA.  x, w: MX.  epilogue: EPI_F32, EPI_HEADS, EPI_GATE_RES or
    EPI_GELU_ERF, whose output is MXFP8 (out0 uint8 e4m3 [M, ldo], out_scale uint8 [M, N / 32])."""
    a = L.MxGemmArgs()
    K = w.q.shape[1]
    if x.q.shape[-1] != K:
        raise ValueError(f"gemm_mx: activation has {x.q.shape[-1]} input features, the weight expects {K}")
    a.Xq, a.Xs, a.ldx, a.ldxs = _p(x.q), _p(x.s), x.q.stride(0), x.s.stride(0)
    a.Wq, a.Ws, a.ldw, a.ldws = _p(w.q), _p(w.s), w.q.stride(0), w.s.stride(0)
    a.bias = _p(bias)
    a.M = int(M if M is not None else x.q.shape[0])
    a.N, a.K = w.q.shape[0], K
    a.epilogue = epilogue
    a.out0, a.out1, a.out2 = _p(out0), _p(out1), _p(out2)
    a.ldo = int(ldo if ldo is not None else w.q.shape[0])
    a.out_scale = _p(out_scale)
    a.ldos = int(out_scale.stride(0)) if out_scale is not None else 0
    a.gate, a.gate_rows, a.gate_ld = _p(gate), gate_rows, gate_ld
    a.tokens, a.tok_pad, a.heads, a.head_dim, a.transpose_mask, a.head_dim_pad = tokens, tok_pad, heads, head_dim, transpose_mask, head_dim_pad
    L.check(L.lib().ln3d_gemm_mxfp8(a, _stream()), "gemm_mx")


def heads_norm_fusable(M, N, tokens, head_dim, head_dim_pad=0):
    """True when ln3d_gemm_bf16's HEADS epilogue applies qk_norm itself for this problem - the library's own answer (it depends on
    the tile configuration it picks), not a copy of its heuristic."""
    return bool(L.lib().ln3d_gemm_heads_norm_fusable(int(M), int(N), int(tokens), int(head_dim), int(head_dim_pad)))


def attention(q, k, vt, out, B, H, Nq, Nq_pad, Nk, Nk_pad, Dh, scale=None, causal=False, dh_true=0):
    """dh_true: true head size when q / k / vt rows are zero-padded to Dh; the output is then compact [B, Nq, H * dh_true]."""
    a = L.AttnArgs()
    a.Q, a.K, a.Vt, a.O = _p(q), _p(k), _p(vt), _p(out)
    a.B, a.H, a.Nq, a.Nq_pad, a.Nk, a.Nk_pad, a.Dh = B, H, Nq, Nq_pad, Nk, Nk_pad, Dh
    a.Dh_true = int(dh_true)
    a.ldo = H * (dh_true if dh_true and dh_true != Dh else Dh)
    a.scale = float(scale if scale is not None else Dh ** -0.5)
    a.causal = causal
    L.check(L.lib().ln3d_attention_bf16(a, _stream()), "attention")


def rmsnorm_heads(x, w, rows, Dh, eps=1e-5, true_dim=0):
    """x rows of Dh (64 / 128) bf16 in place; true_dim < Dh when heads are zero-padded (w padded with zeros to Dh)."""
    L.check(L.lib().ln3d_rmsnorm_heads_bf16(_p(x), _p(w), rows, Dh, int(true_dim), eps, _stream()), "rmsnorm_heads")


def norm_modulate(x, y, rows, D, kind=0, eps=1e-6, weight=None, shift=None, scale=None, mod_rows=1, mod_ld=0,
                  shift_table=None, scale_table=None, rows_in=0, rows_out=0):
    a = L.NormArgs()
    a.x, a.y, a.rows, a.D, a.kind, a.eps, a.weight = _p(x), _p(y), rows, D, kind, eps, _p(weight)
    a.shift, a.scale, a.mod_rows, a.mod_ld = _p(shift), _p(scale), mod_rows, mod_ld
    a.shift_table, a.scale_table, a.rows_in, a.rows_out = _p(shift_table), _p(scale_table), rows_in, rows_out
    L.check(L.lib().ln3d_norm_modulate(a, _stream()), "norm_modulate")


def norm_modulate_mx(x, y, rows, D, kind=0, eps=1e-6, weight=None, shift=None, scale=None, mod_rows=1, mod_ld=0):
    """norm_modulate with an MXFP8 output: y MX [rows, D] (contiguous)."""
    a = L.NormArgs()
    a.x, a.y, a.rows, a.D, a.kind, a.eps, a.weight = _p(x), _p(y.q), rows, D, kind, eps, _p(weight)
    a.shift, a.scale, a.mod_rows, a.mod_ld = _p(shift), _p(scale), mod_rows, mod_ld
    L.check(L.lib().ln3d_norm_modulate_mx(a, _p(y.s), _stream()), "norm_modulate_mx")


def timestep_embedding(t, out, B, dim=256):
    L.check(L.lib().ln3d_timestep_embedding(_p(t), _p(out), B, dim, _stream()), "timestep_embedding")


def add_act_cast(a, b, y_bf16, sum_f32, n, act):
    L.check(L.lib().ln3d_add_act_cast(_p(a), _p(b), _p(y_bf16), _p(sum_f32), n, act, _stream()), "add_act_cast")


def cast_bf16(x, y):
    L.check(L.lib().ln3d_cast_f32_bf16(_p(x), _p(y), x.numel(), _stream()), "cast")


def patch_embed(x, in_scale, w, bias, pos, tokens, Bx, Bn, Cc, S, p, D):
    L.check(L.lib().ln3d_patch_embed(_p(x), _p(in_scale), _p(w), _p(bias), _p(pos), _p(tokens), Bx, Bn, Cc, S, p, D, _stream()),
            "patch_embed")


def final_layer(tokens, shift, scale, mod_ld, shift_table, scale_table, w, bias, out, Bn, Cc, S, p, D):
    L.check(L.lib().ln3d_final_layer(_p(tokens), _p(shift), _p(scale), mod_ld, _p(shift_table), _p(scale_table),
                                     _p(w), _p(bias), _p(out), Bn, Cc, S, p, D, _stream()), "final_layer")


def edm_euler_step(x, eps2, sigma, sigma_next, cfg_scale):
    L.check(L.lib().ln3d_edm_euler_step(_p(x), _p(eps2), sigma, sigma_next, cfg_scale, x.numel(), _stream()), "edm_euler_step")


def ddpm_step(x, eps, noise, a, b, c1, c2, sig, clip):
    L.check(L.lib().ln3d_ddpm_step(_p(x), _p(eps), _p(noise), a, b, c1, c2, sig, clip, x.numel(), _stream()), "ddpm_step")


def flow_euler_step(x2, v2, dt, cfg_scale):
    L.check(L.lib().ln3d_flow_euler_step(_p(x2), _p(v2), dt, cfg_scale, x2.numel() // 2, _stream()), "flow_euler_step")


def axpby(x, y, a, b):
    L.check(L.lib().ln3d_axpby(_p(x), _p(y), a, b, x.numel(), _stream()), "axpby")


def planes_to_channel_last(src, dst, NP, Cc, H, W):
    L.check(L.lib().ln3d_planes_to_channel_last(_p(src), _p(dst), NP, Cc, H, W, _stream()), "planes_to_channel_last")


def planes_to_channel_last_f16(src, dst, NP, Cc, H, W):
    """src [NP, 3 * Cc, H, W] f32 -> dst [NP, 3, H, W, Cc] torch.float16: round to nearest even, saturating at +-65504 (include/ln3d_planes16.h)."""
    if src.dtype != torch.float32 or dst.dtype != torch.float16:
        raise TypeError(f"planes_to_channel_last_f16: f32 source and f16 destination expected, got {src.dtype} -> {dst.dtype}")
    L.check(L.lib().ln3d_planes_to_channel_last_f16(_p(src), _p(dst), NP, Cc, H, W, _stream()), "planes_to_channel_last_f16")


def planes_f32_to_f16(src, dst):
    """contiguous f32 planes (any layout) -> torch.float16, element for element, by the rule of planes_to_channel_last_f16."""
    if src.dtype != torch.float32 or dst.dtype != torch.float16:
        raise TypeError(f"planes_f32_to_f16: f32 source and f16 destination expected, got {src.dtype} -> {dst.dtype}")
    L.check(L.lib().ln3d_planes_f32_to_f16(_p(src), _p(dst), src.numel(), _stream()), "planes_f32_to_f16")


def _plane_entry(planes, what):
    """the entry point for this texel type: f32 planes -> include/ln3d.h, f16 planes -> include/ln3d_planes16.h; nothing else exists"""
    if planes.dtype == torch.float32:
        return getattr(L.lib(), "ln3d_" + what)
    if planes.dtype == torch.float16:
        return getattr(L.lib(), "ln3d_" + what + "_f16")
    raise TypeError(f"{what}: tri-plane texels are torch.float32 or torch.float16, got {planes.dtype}")


def planes_to_nchw(src, dst, NP, Cc, H, W):
    L.check(L.lib().ln3d_planes_to_nchw(_p(src), _p(dst), NP, Cc, H, W, _stream()), "planes_to_nchw")


def render_triplane(planes_cl, H, W, plane_index, cams, res, dec, jitter, u_fine, rgb, depth, wsum, ray_limits, scalars,
                    box_warp=0.9, bbox_min=-0.45, bbox_max=0.45, white_back=True, coarse_sigma=None, fine_depths=None,
                    ray_o=None, ray_d=None, fine_sigma=None, coarse_coords=None, fine_coords=None, n_views=None, views_per_call=0,
                    rays_per_view=0, visibility=None, depth_resolution=0, depth_resolution_importance=0, ray_start='auto', ray_end='auto',
                    filter_out_of_bbox=True, weights=None, all_coords=None, feature_volume=None):
    """cams [V,25] (rays generated in-kernel) or explicit ray_o / ray_d [V, M, 3] (then cams may be None; rays_per_view = M).
    planes_cl: channel-last texels, torch.float32 or torch.float16 (ln3d_render_triplane_f16); any other dtype is a TypeError.
    views_per_call: how many consecutive views form one reference forward() call for the call-wide reductions (ray-limit fix-up,
    depth clamp range); 0 = all of them (include/ln3d.h).  ray_start / ray_end: both 'auto' or both numbers."""
    entry = _plane_entry(planes_cl, "render_triplane")
    a = L.RenderArgs()
    a.planes, a.H, a.W, a.plane_index, a.cams = _p(planes_cl), H, W, _p(plane_index), _p(cams)
    a.V, a.res = (cams.shape[0] if cams is not None else n_views), res
    a.dec_w0, a.dec_b0, a.dec_w1, a.dec_b1 = (_p(t) for t in dec)
    a.jitter, a.u_fine = _p(jitter), _p(u_fine)
    a.box_warp, a.bbox_min, a.bbox_max, a.white_back = box_warp, bbox_min, bbox_max, int(white_back)
    a.rgb, a.depth, a.wsum, a.ray_limits, a.scalars = _p(rgb), _p(depth), _p(wsum), _p(ray_limits), _p(scalars)
    a.coarse_sigma, a.fine_depths = _p(coarse_sigma), _p(fine_depths)
    a.ray_o, a.ray_d, a.fine_sigma, a.coarse_coords, a.fine_coords = _p(ray_o), _p(ray_d), _p(fine_sigma), _p(coarse_coords), _p(fine_coords)
    a.views_per_call = int(views_per_call)
    a.rays_per_view, a.visibility = int(rays_per_view), _p(visibility)
    a.depth_resolution, a.depth_resolution_importance = int(depth_resolution), int(depth_resolution_importance)
    if (ray_start == 'auto') != (ray_end == 'auto'):
        raise ValueError("ray_start / ray_end: both 'auto' or both numbers (renderer.py:145)")
    if ray_start == 'auto':
        a.ray_mode = 0
    else:
        a.ray_mode, a.ray_start, a.ray_end = 1, float(ray_start), float(ray_end)
    a.no_bbox_filter = 0 if filter_out_of_bbox else 1
    a.weights, a.all_coords, a.feature_volume = _p(weights), _p(all_coords), _p(feature_volume)
    L.check(entry(a, _stream()), "render_triplane")


def query_points(planes_cl, H, W, points, dec, box_warp, sigma, rgb, scalars):
    """scalars: caller-owned f32 scratch of _lib.RENDER_SCRATCH_FLOATS (no allocation inside the library).  planes_cl: torch.float32 or
    torch.float16 texels (ln3d_query_points_f16)."""
    L.check(_plane_entry(planes_cl, "query_points")(_p(planes_cl), H, W, _p(points), points.shape[0], *(_p(t) for t in dec),
                                      box_warp, _p(sigma), _p(rgb), _p(scalars), _stream()), "query_points")


def query_points_grad(planes_cl, H, W, points, dec, box_warp, sigma, grad):
    """sigma [P] and d sigma / d p [P, 3] of ONE tri-plane [3, H, W, 32] (torch.float32 or torch.float16 texels) at points [P, 3]
    (include/ln3d_normals.h)."""
    L.check(_plane_entry(planes_cl, "query_points_grad")(_p(planes_cl), H, W, _p(points), points.shape[0], *(_p(t) for t in dec),
                                                         box_warp, _p(sigma), _p(grad), _stream()), "query_points_grad")


NORMAL_SPACES = {'world': 0, 'camera': 1}
NORMAL_MODES = ('surface', 'composited')


def surface_normals(planes_cl, H, W, plane_index, dec, box_warp, depth, wsum, normal, cams=None, res=0, ray_o=None, ray_d=None, n_views=None,
                    rays_per_view=0, mask_threshold=0.5, space='world', points=None, mode='surface', weights=None, coords=None,
                    weight_floor=0.0, accum=None):
    """normal [V, 3, M] at the expected-depth surface point of every ray of a finished render (its depth / wsum [V, M]); the rays are
    cams [V, 25] + res (generated as the marcher generates them) or explicit ray_o / ray_d [V, M, 3].  space: 'world' or 'camera'
    (needs cams).  points: optional [V, M, 3] output, the surface points (include/ln3d_normals.h).
    mode 'composited': the per-sample normals at coords [V, M, T, 3] composited by weights [V, M, T - 1] (both outputs of a finished
    ops.render_triplane call over the same rays), samples with a weight <= weight_floor skipped; depth and the rays are not read
    (depth may be None; M = rays_per_view or res * res), points is not written, accum: optional [V, 3, M] output, the un-normalised
    sum."""
    if space not in NORMAL_SPACES:
        raise ValueError(f"normal space {space!r}: expected one of {sorted(NORMAL_SPACES)}")
    if mode not in NORMAL_MODES:
        raise ValueError(f"normal mode {mode!r}: expected one of {sorted(NORMAL_MODES)}")
    entry = _plane_entry(planes_cl, "surface_normals")
    a = L.NormalsArgs()
    if n_views is None and cams is None:
        raise ValueError("surface_normals: the number of views comes from cams [V, 25] or n_views; got neither")
    if mode == 'composited':
        V = n_views if n_views is not None else cams.shape[0]
        M = int(rays_per_view) if rays_per_view else int(res) * int(res)
        if weights is None or coords is None:
            raise ValueError("surface_normals(mode='composited') needs weights [V, M, T - 1] and coords [V, M, T, 3] of a finished render")
        if points is not None:
            raise ValueError("surface_normals(mode='composited') writes no points")
        T = coords.numel() // max(1, 3 * V * M)
        for name, t, n in (('weights', weights, V * M * (T - 1)), ('coords', coords, V * M * T * 3), ('wsum', wsum, V * M),
                           ('normal', normal, V * 3 * M), ('accum', accum, V * 3 * M)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"surface_normals(mode='composited'): {name} must be a contiguous torch.float32 tensor, got {t.dtype}"
                                f"{'' if t.is_contiguous() else ', not contiguous'}")
            if t.numel() < n or (name in ('weights', 'coords') and t.numel() != n):
                raise ValueError(f"surface_normals(mode='composited'): {name} has {t.numel()} elements, V = {V}, M = {M}, T = {T} need {n}")
        if not 2 <= T <= 256:
            raise ValueError(f"surface_normals(mode='composited'): 2 ... 256 samples per ray, got {T}")
        a.mode, a.samples, a.weights, a.coords, a.weight_floor, a.accum = 1, T, _p(weights), _p(coords), float(weight_floor), _p(accum)
    elif weights is not None or coords is not None or accum is not None or weight_floor != 0.0:
        raise ValueError("surface_normals: weights / coords / weight_floor / accum belong to mode='composited'")
    a.planes, a.H, a.W, a.plane_index, a.cams = _p(planes_cl), H, W, _p(plane_index), _p(cams)
    a.V, a.res = (n_views if n_views is not None else cams.shape[0]), int(res)
    a.ray_o, a.ray_d, a.rays_per_view = _p(ray_o), _p(ray_d), int(rays_per_view)
    a.dec_w0, a.dec_b0, a.dec_w1, a.dec_b1 = (_p(t) for t in dec)
    a.box_warp, a.depth, a.wsum, a.mask_threshold = box_warp, _p(depth), _p(wsum), float(mask_threshold)
    a.space, a.normal, a.points = NORMAL_SPACES[space], _p(normal), _p(points)
    L.check(entry(a, _stream()), "surface_normals")


def groupnorm_swish(x, w, b, y, stats, N, HW, Cc, groups=32, eps=1e-6, swish=True):
    L.check(L.lib().ln3d_groupnorm_swish(_p(x), _p(w), _p(b), _p(y), _p(stats), N, HW, Cc, groups, eps, swish,
                                         _stream()), "groupnorm_swish")


def im2col3x3(x, col, N, H, W, Cc, upsample, Kpad):
    L.check(L.lib().ln3d_im2col3x3(_p(x), _p(col), N, H, W, Cc, upsample, Kpad, _stream()), "im2col3x3")


def patch_embed_triplane(latent, w, bias, out_silu, out_raw, B, Cg, S, p, D):
    L.check(L.lib().ln3d_patch_embed_triplane(_p(latent), _p(w), _p(bias), _p(out_silu), _p(out_raw), B, Cg, S, p, D, _stream()),
            "patch_embed_triplane")


def tile_rows(x, y, per, reps):
    L.check(L.lib().ln3d_tile_rows(_p(x), _p(y), per, reps, _stream()), "tile_rows")


def add_table_rows(t0, tables, out, layers, B, W):
    L.check(L.lib().ln3d_add_table_rows(_p(t0), _p(tables), _p(out), layers, B, W, _stream()), "add_table_rows")


def cfg_combine_dup(v2, cfg_scale):
    L.check(L.lib().ln3d_cfg_combine_dup(_p(v2), cfg_scale, v2.numel() // 2, _stream()), "cfg_combine_dup")


def vt_key_order(n_pad, device=None):
    """Index map of the V^T layout consumed by ln3d_attention_bf16: position p of every 16-key group holds key
    perm(p) with bits 2 and 3 swapped ([0-3, 8-11, 4-7, 12-15]).  ln3d_gemm_bf16's HEADS epilogue writes this layout
    itself; this helper exists for callers (tests, op-level bindings) that build V^T by hand: vt_perm = vt[..., idx]."""
    t = torch.arange(n_pad, device=device)
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def ddim_step(x, eps_u, eps_c, noise, cfg_scale, a, b, sqrt_ab_prev, coef_eps, sigma, clip):
    L.check(L.lib().ln3d_ddim_step(_p(x), _p(eps_u), _p(eps_c), _p(noise), cfg_scale, a, b, sqrt_ab_prev, coef_eps, sigma, clip, x.numel(),
                                   _stream()), "ddim_step")


def mesh_count(sigma, G, thr, counts):
    L.check(L.lib().ln3d_mesh_count(_p(sigma), G, thr, _p(counts), _stream()), "mesh_count")


def mesh_emit(sigma, G, thr, offsets, tri_pos, tri_key):
    L.check(L.lib().ln3d_mesh_emit(_p(sigma), G, thr, _p(offsets), _p(tri_pos), _p(tri_key), _stream()), "mesh_emit")


def mcubes_count(sigma, G, thr, counts):
    L.check(L.lib().ln3d_mcubes_count(_p(sigma), G, thr, _p(counts), _stream()), "mcubes_count")


def mcubes_emit(sigma, G, thr, offsets, tri_pos, tri_key):
    L.check(L.lib().ln3d_mcubes_emit(_p(sigma), G, thr, _p(offsets), _p(tri_pos), _p(tri_key), _stream()), "mcubes_emit")


def check_index(t, n, what, shape=None):
    """include/ln3d_meshclean.h and include/ln3d_meshsimplify.h take the values of their index arrays in [0, n) as a precondition: a value
    outside that range must never reach a kernel.  A contiguous int64 tensor (of `shape`, when given) whose values all lie in that range,
    or ValueError (one read-back of the smallest and largest value); a host tensor that passes is refused like every other."""
    if t.dtype != torch.int64 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what}: expected a contiguous int64 tensor" + (f" of shape {tuple(shape)}" if shape is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)}")
    if t.numel():
        lo, hi = (int(x) for x in torch.aminmax(t))
        if lo < 0 or hi >= n:
            raise ValueError(f"{what}: values span [{lo}, {hi}], outside [0, {n})")
    if not t.is_cuda:
        raise RuntimeError(_NEED_DEVICE)


def check_faces(faces, nv):
    """check_index for faces [Nf, 3] of a mesh with nv vertices"""
    check_index(faces, nv, "faces", tuple(faces.shape[:1]) + (3,))


def mesh_components(faces, nv, label, check=True):
    """label [nv] int32 <- the smallest vertex index of every vertex's connected component (include/ln3d_meshclean.h).  check=False: the
    caller has already put these faces through check_faces."""
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_mesh_components(_p(faces), faces.shape[0], nv, _p(label), _stream()), "mesh_components")


def mesh_component_counts(faces, label, nvert, nface, best, check=True):
    """nvert, nface [nv] int32 per label, best int64[1] (the uint64 word (nface << 32) | (0x7fffffff - root) of the largest component)"""
    nv = label.shape[0]
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_mesh_component_counts(_p(faces), faces.shape[0], _p(label), nv, _p(nvert), _p(nface), _p(best),
                                               _stream()), "mesh_component_counts")


def mesh_mark(faces, label, nface, min_faces, largest_only, best, keep_v, keep_f, check=True):
    nv = label.shape[0]
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_mesh_mark(_p(faces), faces.shape[0], _p(label), _p(nface), nv, min_faces, largest_only, _p(best), _p(keep_v),
                                   _p(keep_f), _stream()), "mesh_mark")


def mesh_gather(verts, faces, keep_v, vprefix, keep_f, fprefix, verts_out, faces_out, check=True):
    """vprefix / fprefix: int64 inclusive prefix sums of the int32 masks; verts_out / faces_out: at least vprefix[-1] / fprefix[-1] rows"""
    nv = verts.shape[0]
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_mesh_gather(_p(verts), _p(faces), _p(keep_v), _p(vprefix), _p(keep_f), _p(fprefix), nv, faces.shape[0],
                                     _p(verts_out), _p(faces_out), _stream()), "mesh_gather")


def _buffer(t, dtype, shape, what):
    """the kernels of include/ln3d_meshsimplify.h and include/ln3d_meshbake.h write whole rows of the buffers they are given: a buffer of another dtype, a shorter one
    or a strided view would be written past its end, so it is refused here (metadata only: no read-back)"""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def simplify_keys(verts, origin, cell, key):
    """key [nv] int64 <- the packed lattice cell of every vertex (include/ln3d_meshsimplify.h); verts [nv,3] f32; origin: three floats.
    There is no index to check: the kernel clamps."""
    _buffer(verts, torch.float32, (verts.shape[0], 3), "verts")
    _buffer(key, torch.int64, (verts.shape[0],), "key")
    ox, oy, oz = (float(o) for o in origin)
    L.check(L.lib().ln3d_simplify_keys(_p(verts), verts.shape[0], ox, oy, oz, float(cell), _p(key), _stream()), "simplify_keys")


def simplify_mean(verts, order, start, rep, check=True):
    """rep [nc,3] f32 <- the mean of every cluster's members, summed in the order of its row of the CSR (order [nv], start [nc + 1] int64).
    check=False: the caller has made order and start itself (a stable sort and the prefix sum of its counts)."""
    nv, nc = verts.shape[0], start.shape[0] - 1
    _buffer(verts, torch.float32, (nv, 3), "verts")
    _buffer(order, torch.int64, (nv,), "order")
    _buffer(start, torch.int64, (nc + 1,), "start")
    _buffer(rep, torch.float32, (nc, 3), "rep")
    if check:
        check_index(order, nv, "order", (nv,))
        check_index(start, nv + 1, "start")
        if nc >= 1 and (int(start[0]) != 0 or int(start[-1]) != nv or bool((start[1:] < start[:-1]).any())):
            raise ValueError("start: expected an ascending row-pointer array from 0 to nv")
    L.check(L.lib().ln3d_simplify_mean(_p(verts), _p(order), _p(start), nv, nc, _p(rep), _stream()), "simplify_mean")


def simplify_faces(faces, cluster, nc, cfaces, fkey, check=True):
    """cfaces [nf,3] int64 <- cluster[faces]; fkey [nf] int64 <- -1 for a collapsed face, else its ascending corners packed 21 bits each"""
    nv, nf = cluster.shape[0], faces.shape[0]
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(cluster, torch.int64, (nv,), "cluster")
    _buffer(cfaces, torch.int64, (nf, 3), "cfaces")
    _buffer(fkey, torch.int64, (nf,), "fkey")
    if check:
        check_index(cluster, nc, "cluster")
        check_faces(faces, nv)
    L.check(L.lib().ln3d_simplify_faces(_p(faces), faces.shape[0], _p(cluster), nv, nc, _p(cfaces), _p(fkey), _stream()), "simplify_faces")


def simplify_first(sorted_key, perm, keep_f, check=True):
    """keep_f [nf] int32 <- 1 at the original index of every run head of the stably sorted keys whose key is not -1, 0 elsewhere"""
    nf = sorted_key.shape[0]
    _buffer(sorted_key, torch.int64, (nf,), "sorted_key")
    _buffer(perm, torch.int64, (nf,), "perm")
    _buffer(keep_f, torch.int32, (nf,), "keep_f")
    if check:
        check_index(perm, nf, "perm", (nf,))
    L.check(L.lib().ln3d_simplify_first(_p(sorted_key), _p(perm), nf, _p(keep_f), _stream()), "simplify_first")


def simplify_used(cfaces, keep_f, keep_v, check=True):
    """keep_v [nc] int32 <- 1 for the clusters that a kept face names, 0 for the others"""
    nc, nf = keep_v.shape[0], cfaces.shape[0]
    _buffer(cfaces, torch.int64, (nf, 3), "cfaces")
    _buffer(keep_f, torch.int32, (nf,), "keep_f")
    _buffer(keep_v, torch.int32, (nc,), "keep_v")
    if check:
        check_faces(cfaces, nc)
    L.check(L.lib().ln3d_simplify_used(_p(cfaces), _p(keep_f), cfaces.shape[0], nc, _p(keep_v), _stream()), "simplify_used")


def quadric_pairs(cfaces, nc, pair_key, check=True):
    """pair_key [3 nf] int64 <- cfaces[f][j] << 31 | f for every corner j of face f whose cluster differs from the corners before it,
    INT64_MAX for the others (include/ln3d_meshquadric.h); cfaces [nf,3] int64 with every value in [0, nc).  check=False: the caller
    has made cfaces itself (simplify_faces)."""
    nf = cfaces.shape[0]
    _buffer(cfaces, torch.int64, (nf, 3), "cfaces")
    _buffer(pair_key, torch.int64, (3 * nf,), "pair_key")
    if check:
        check_faces(cfaces, nc)
    L.check(L.lib().ln3d_quadric_pairs(_p(cfaces), nf, nc, _p(pair_key), _stream()), "quadric_pairs")


def quadric_place(verts, faces, sorted_pair_key, start, rep_mean, origin, cell, cluster_cell_key, eps, rep_out, placed, check=True):
    """rep_out [nc,3] f32, placed [nc] int32 <- the quadric-error placement of every cluster (include/ln3d_meshquadric.h): the
    minimiser of the summed squared distance to the planes of the cluster's faces, regularised with eps * trace, where it lies inside the
    cluster's lattice cell (placed 1), rep_mean's bits elsewhere (placed 0).  verts [nv,3] f32, faces [nf,3] int64, sorted_pair_key [3 nf]
    int64: quadric_pairs' keys in ascending order, start [nc + 1] int64: the row pointers into it, rep_mean [nc,3] f32, origin: three
    floats, cluster_cell_key [nc] int64.  rep_out may be rep_mean itself and may not overlap it otherwise.  check=False: the caller has
    put faces through check_faces and made the keys and start itself."""
    nv, nf, nc, npairs = verts.shape[0], faces.shape[0], rep_mean.shape[0], sorted_pair_key.shape[0]
    _buffer(verts, torch.float32, (nv, 3), "verts")
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(sorted_pair_key, torch.int64, (3 * nf,), "sorted_pair_key")
    _buffer(start, torch.int64, (nc + 1,), "start")
    _buffer(rep_mean, torch.float32, (nc, 3), "rep_mean")
    _buffer(cluster_cell_key, torch.int64, (nc,), "cluster_cell_key")
    _buffer(rep_out, torch.float32, (nc, 3), "rep_out")
    _buffer(placed, torch.int32, (nc,), "placed")
    try:
        e = float(np.float32(eps))
    except (TypeError, ValueError):
        e = math.nan
    if not 0.0 < e <= 1.0:
        raise ValueError(f"eps {eps!r}: expected a number in (0, 1] (in float32)")
    if check:
        check_faces(faces, nv)
        check_index(start, npairs + 1, "start")
        if nc >= 1 and bool((start[1:] < start[:-1]).any()):
            raise ValueError("start: expected an ascending row-pointer array")
    ox, oy, oz = (float(o) for o in origin)
    L.check(L.lib().ln3d_quadric_place(_p(verts), nv, _p(faces), nf, _p(sorted_pair_key), npairs, _p(start), nc, _p(rep_mean), ox, oy, oz,
                                       float(cell), _p(cluster_cell_key), e, _p(rep_out), _p(placed), _stream()), "quadric_place")


def bake_points(verts, faces, T, n, c, points, owner, check=True):
    """points [T*T,3] f32, owner [T*T] int32 <- the point on its face and the face of every texel of the per-face atlas (T, n, c:
    mesh.atlas_layout; include/ln3d_meshbake.h); verts [nv,3] f32, faces [nf,3] int64.  check=False: the caller has already put these
    faces through check_faces."""
    nv, nf = verts.shape[0], faces.shape[0]
    _buffer(verts, torch.float32, (nv, 3), "verts")
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(points, torch.float32, (T * T, 3), "points")
    _buffer(owner, torch.int32, (T * T,), "owner")
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_bake_points(_p(verts), nv, _p(faces), nf, T, n, c, _p(points), _p(owner), _stream()), "bake_points")


def bake_pack(rgb, owner, fill, tex):
    """tex [P,3] uint8 <- fill where owner [P] int32 is negative, elsewhere rgb [P,3] f32 clamped to [0, 1], times 255, truncated (NaN: 0)"""
    P = owner.shape[0]
    _buffer(rgb, torch.float32, (P, 3), "rgb")
    _buffer(owner, torch.int32, (P,), "owner")
    _buffer(tex, torch.uint8, (P, 3), "tex")
    L.check(L.lib().ln3d_bake_pack(_p(rgb), _p(owner), P, int(fill), _p(tex), _stream()), "bake_pack")


def smooth_edge_keys(faces, nv, key, check=True):
    """key [3 nf] int64 <- the undirected edge (lo << 32) | hi between corners j and (j + 1) % 3 of every face, -1 where they are equal
    (include/ln3d_meshsmooth.h); faces [nf,3] int64 of a mesh with nv vertices.  check=False: the caller has already put these faces
    through check_faces."""
    nf = faces.shape[0]
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(key, torch.int64, (3 * nf,), "key")
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_smooth_edge_keys(_p(faces), nf, _p(key), _stream()), "smooth_edge_keys")


def smooth_halfedges(edge, count, nv, dkey, pinned, check=True):
    """dkey [2 ne] int64 <- every distinct edge of edge [ne] int64 in both directions, (src << 32) | dst; pinned [nv] int32, ZEROED BY THE
    CALLER, <- 1 at both ends of every edge whose count [ne] int64 is 1.  check=False: the caller has made edge from smooth_edge_keys."""
    ne = edge.shape[0]
    _buffer(edge, torch.int64, (ne,), "edge")
    _buffer(count, torch.int64, (ne,), "count")
    _buffer(dkey, torch.int64, (2 * ne,), "dkey")
    _buffer(pinned, torch.int32, (nv,), "pinned")
    if check:
        check_index(torch.stack([edge >> 32, edge & 0xffffffff]), nv, "edge (both ends)")
    L.check(L.lib().ln3d_smooth_halfedges(_p(edge), _p(count), ne, nv, _p(dkey), _p(pinned), _stream()), "smooth_halfedges")


def smooth_step(verts_in, start, nbr, pinned, factor, verts_out, check=True):
    """verts_out [nv,3] f32 <- one smoothing pass of verts_in with `factor` over the CSR adjacency start [nv + 1] int64, nbr [nh] int32;
    a vertex whose pinned [nv] int32 is set, or whose row is empty, is copied.  verts_out may not overlap verts_in.  check=False: the caller
    has made start and nbr itself (mesh.mesh_adjacency)."""
    nv, nh = verts_in.shape[0], nbr.shape[0]
    _buffer(verts_in, torch.float32, (nv, 3), "verts_in")
    _buffer(start, torch.int64, (nv + 1,), "start")
    _buffer(nbr, torch.int32, (nh,), "nbr")
    _buffer(pinned, torch.int32, (nv,), "pinned")
    _buffer(verts_out, torch.float32, (nv, 3), "verts_out")
    if check:
        if int(start[0]) != 0 or int(start[-1]) != nh or bool((start[1:] < start[:-1]).any()):          # so every entry lies in [0, nh]
            raise ValueError("start: expected an ascending row-pointer array from 0 to the number of half-edges")
        check_index(nbr.long(), nv, "nbr")
    L.check(L.lib().ln3d_smooth_step(_p(verts_in), _p(start), _p(nbr), _p(pinned), nv, nh, float(factor), _p(verts_out), _stream()), "smooth_step")


# ------------------------------------------------------------------ binary mesh export (include/ln3d_meshpack.h)
def _pack_rows(xyz, normal, what="xyz"):
    """xyz [n,3] f32 and, when given, normal of the same shape -> n"""
    n = xyz.shape[0]
    _buffer(xyz, torch.float32, (n, 3), what)
    if normal is not None:
        _buffer(normal, torch.float32, (n, 3), "normal")
    return n


def _pack_bytes(out, nbytes, what="out"):
    """a uint8 buffer of exactly nbytes rounded up to a multiple of 4: the packers write whole words"""
    _buffer(out, torch.uint8, ((nbytes + 3) // 4 * 4,), what)


def pack_ply_vertices(xyz, normal, rgb, rot9, out):
    """out [ceil(nv * S / 4) * 4] uint8 <- the nv vertex records of a binary little-endian PLY, S = 15 bytes each (3 f32 rot9 @ xyz, 3 uint8
    colours) or 27 with normal (3 f32 rot9 @ normal between them); the pad bytes behind the last record are 0.  xyz, normal (or None), rgb
    [nv,3] f32, rot9 [9] f32: a row-major 3 x 3 matrix."""
    nv = _pack_rows(xyz, normal)
    _buffer(rgb, torch.float32, (nv, 3), "rgb")
    _buffer(rot9, torch.float32, (9,), "rot9")
    _pack_bytes(out, nv * (15 if normal is None else 27))
    L.check(L.lib().ln3d_pack_ply_vertices(_p(xyz), _p(normal), _p(rgb), _p(rot9), nv, _p(out), _stream()), "pack_ply_vertices")


def pack_ply_faces(faces, out):
    """out [ceil(nf * 13 / 4) * 4] uint8 <- the nf face records of a binary PLY: the byte 3 and three int32; faces [nf,3] int64.  Nothing is
    gathered, so there is no index to check: the values are narrowed to 32 bits."""
    nf = faces.shape[0]
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _pack_bytes(out, nf * 13)
    L.check(L.lib().ln3d_pack_ply_faces(_p(faces), nf, _p(out), _stream()), "pack_ply_faces")


def pack_gltf_vertices(xyz, normal, rgb, rot9, pos_out, nrm_out, rgba_out):
    """pos_out [nv,3] f32 <- rot9 @ xyz; nrm_out [nv,3] f32 <- rot9 @ normal (both None, or neither); rgba_out [nv,4] uint8 <- the colour
    bytes of rgb [nv,3] f32 and 255"""
    nv = _pack_rows(xyz, normal)
    if (normal is None) != (nrm_out is None):
        raise ValueError("normal and nrm_out: expected both or neither")
    _buffer(rgb, torch.float32, (nv, 3), "rgb")
    _buffer(rot9, torch.float32, (9,), "rot9")
    _buffer(pos_out, torch.float32, (nv, 3), "pos_out")
    if nrm_out is not None:
        _buffer(nrm_out, torch.float32, (nv, 3), "nrm_out")
    _buffer(rgba_out, torch.uint8, (nv, 4), "rgba_out")
    L.check(L.lib().ln3d_pack_gltf_vertices(_p(xyz), _p(normal), _p(rgb), _p(rot9), nv, _p(pos_out), _p(nrm_out), _p(rgba_out), _stream()),
            "pack_gltf_vertices")


def pack_gltf_indices(faces, idx_out):
    """idx_out [3 nf] int32 (read as uint32) <- faces [nf,3] int64, narrowed"""
    nf = faces.shape[0]
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(idx_out, torch.int32, (3 * nf,), "idx_out")
    L.check(L.lib().ln3d_pack_gltf_indices(_p(faces), nf, _p(idx_out), _stream()), "pack_gltf_indices")


def pack_gltf_corners(xyz, normal, faces, uv, rot9, pos_out, nrm_out, uv_out, check=True):
    """The per-corner vertex sections of a textured GLB: pos_out [3 nf,3] f32 <- rot9 @ xyz[faces[i][j]] at corner 3 i + j; nrm_out likewise
    from normal (both None, or neither); uv_out [3 nf,2] f32 <- (u, 1 - v) of uv [nf,3,2] f32.  check=False: the caller has already put these
    faces through check_faces."""
    nv, nf = _pack_rows(xyz, normal), faces.shape[0]
    if (normal is None) != (nrm_out is None):
        raise ValueError("normal and nrm_out: expected both or neither")
    _buffer(faces, torch.int64, (nf, 3), "faces")
    _buffer(uv, torch.float32, (nf, 3, 2), "uv")
    _buffer(rot9, torch.float32, (9,), "rot9")
    _buffer(pos_out, torch.float32, (3 * nf, 3), "pos_out")
    if nrm_out is not None:
        _buffer(nrm_out, torch.float32, (3 * nf, 3), "nrm_out")
    _buffer(uv_out, torch.float32, (3 * nf, 2), "uv_out")
    if check:
        check_faces(faces, nv)
    L.check(L.lib().ln3d_pack_gltf_corners(_p(xyz), _p(normal), _p(faces), _p(uv), _p(rot9), nv, nf, _p(pos_out), _p(nrm_out), _p(uv_out),
                                           _stream()), "pack_gltf_corners")


def position_bounds(pos, bounds6):
    """bounds6 [6] f32 <- the per-axis minimum, then maximum, of pos [n,3] f32, which the caller has found finite"""
    n = pos.shape[0]
    _buffer(pos, torch.float32, (n, 3), "pos")
    _buffer(bounds6, torch.float32, (6,), "bounds6")
    L.check(L.lib().ln3d_position_bounds(_p(pos), n, _p(bounds6), _stream()), "position_bounds")


SNAP_MAX_ITERS = 64


def snap_points(planes_cl, H, W, points_in, dec, box_warp, level, iters, tol, max_step, max_dist, points_out, residual, state, evals):
    """points_out [P,3] f32, residual [P] f32, state [P] int32, evals [P] int32 <- the damped Newton projection of points_in [P,3] f32 onto
    sigma = level of ONE tri-plane [3, H, W, 32] (torch.float32 or torch.float16 texels), at most `iters` iterations
    (include/ln3d_meshsnap.h).  points_out may not overlap points_in.  ValueError on a buffer of another dtype, shape or stride, iters
    not an integer in [0, 64], a level / tol / max_step / max_dist that is not finite (in float32), tol < 0, max_step <= 0, max_dist < 0."""
    P = points_in.shape[0]
    _buffer(points_in, torch.float32, (P, 3), "points_in")
    _buffer(points_out, torch.float32, (P, 3), "points_out")
    _buffer(residual, torch.float32, (P,), "residual")
    _buffer(state, torch.int32, (P,), "state")
    _buffer(evals, torch.int32, (P,), "evals")
    if planes_cl.dim() != 4 or tuple(planes_cl.shape) != (3, H, W, 32) or not planes_cl.is_contiguous():
        raise ValueError(f"planes: expected one contiguous channel-last tri-plane of shape {(3, H, W, 32)}, got {tuple(planes_cl.shape)}")
    if P < 1:
        raise ValueError("points_in: expected at least one point")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= SNAP_MAX_ITERS:
        raise ValueError(f"iters {iters!r}: expected an integer in [0, {SNAP_MAX_ITERS}]")
    vals = {}
    for name, v in (("level", level), ("tol", tol), ("max_step", max_step), ("max_dist", max_dist)):
        try:
            with np.errstate(over='ignore'):
                vals[name] = float(np.float32(v))
        except (TypeError, ValueError):
            vals[name] = math.nan
        if not math.isfinite(vals[name]):
            raise ValueError(f"{name} {v!r}: expected a finite number (in float32)")
    if vals["tol"] < 0 or vals["max_step"] <= 0 or vals["max_dist"] < 0:
        raise ValueError(f"expected tol >= 0, max_step > 0 and max_dist >= 0 (in float32), got {tol!r}, {max_step!r}, {max_dist!r}")
    if points_out.data_ptr() == points_in.data_ptr():
        raise ValueError("points_out: may not be the buffer of points_in")
    L.check(_plane_entry(planes_cl, "snap_points")(_p(planes_cl), H, W, _p(points_in), P, *(_p(t) for t in dec), box_warp, vals["level"],
                                                   int(iters), vals["tol"], vals["max_step"], vals["max_dist"], _p(points_out), _p(residual),
                                                   _p(state), _p(evals), _stream()), "snap_points")


def lincomb(y, ks, cs, out):
    n = len(ks)
    arr_k = (C.c_void_p * n)(*[_p(k) for k in ks])
    arr_c = (C.c_float * n)(*[float(c) for c in cs])
    L.check(L.lib().ln3d_lincomb(_p(y), arr_k, arr_c, n, _p(out), out.numel(), _stream()), "lincomb")


def err_ratio_sq(err, y0, y1, atol, rtol, acc):
    L.check(L.lib().ln3d_err_ratio_sq(_p(err), _p(y0), _p(y1), atol, rtol, _p(acc), err.numel(), _stream()), "err_ratio_sq")


def embed_tokens(ids, tok_emb, pos_emb, out, B, T, D):
    assert ids.dtype == torch.int32
    L.check(L.lib().ln3d_embed_tokens(_p(ids), _p(tok_emb), _p(pos_emb), _p(out), B, T, D, tok_emb.shape[0], _stream()), "embed_tokens")


def layernorm_f32(x, w, b, y, rows, D, eps=1e-5):
    L.check(L.lib().ln3d_layernorm_f32(_p(x), _p(w), _p(b), _p(y), rows, D, eps, _stream()), "layernorm_f32")


def image_preprocess(x, S, antialias, mean, std):
    """[N, C, H, W] f32 in [-1, 1] -> resized (kornia bicubic, align_corners, optional antialias blur) and normalised [N, C, S, S]"""
    N, Cc, H, W = x.shape
    x = x.contiguous().float()
    out = torch.empty(N, Cc, S, S, device=x.device, dtype=torch.float32)
    tmp = torch.empty(2 * x.numel(), device=x.device, dtype=torch.float32) if (antialias and (H > S or W > S)) else None
    m = (C.c_float * Cc)(*[float(v) for v in mean])
    sd = (C.c_float * Cc)(*[float(v) for v in std])
    L.check(L.lib().ln3d_image_preprocess(_p(x), _p(out), _p(tmp), N, Cc, H, W, S, antialias, m, sd, _stream()), "image_preprocess")
    return out


def vit_patchify(img, out, B, S, p, Kpad, C=3):
    L.check(L.lib().ln3d_vit_patchify(_p(img), _p(out), B, S, p, Kpad, C, _stream()), "vit_patchify")


def plucker_rays(c, S):
    """c f32 [V, 25] (c2w 4x4 + intrinsics 3x3) -> Pluecker maps f32 [V, 6, S, S] (o x d, d)."""
    V = c.shape[0]
    out = torch.empty(V, 6, S, S, device=c.device, dtype=torch.float32)
    c32 = c.contiguous().float()                     # kept alive across the launch (a temporary's block could be handed out again)
    L.check(L.lib().ln3d_plucker_rays(_p(c32), _p(out), V, S, _stream()), "plucker_rays")
    return out


def vit_assemble(patch, cls, reg, pos, x, B, Lp, R, D):
    L.check(L.lib().ln3d_vit_assemble(_p(patch), _p(cls), _p(reg), _p(pos), _p(x), B, Lp, R, D, _stream()), "vit_assemble")


def device_cus():
    return int(L.lib().ln3d_device_cus())


def probe_mfma(out, wgs, iters):
    """Diagnostic pure-MFMA stream (include/ln3d.h ln3d_probe_mfma_bf16); returns the flop it executes."""
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() >= wgs * 512
    L.check(L.lib().ln3d_probe_mfma_bf16(_p(out), int(wgs), int(iters), _stream()), "probe_mfma")
    return wgs * 8 * iters * 8 * 2.0 * 32 * 32 * 16


# ---------------------------------------------------------------- U-Net pieces (csrc/unet_ops.hip)
def groupnorm_any(x, w, b, y, N, HW, Cc, groups=32, eps=1e-5, swish=True, add_row=None, mod_scale=None, mod_shift=None):
    L.check(L.lib().ln3d_groupnorm_any(_p(x), _p(add_row), _p(w), _p(b), _p(mod_scale), _p(mod_shift), _p(y), N, HW, Cc, groups, eps,
                                       swish, _stream()), "groupnorm_any")


def im2col3x3_strided(x, col, N, H, W, Cc, stride, Kpad):
    L.check(L.lib().ln3d_im2col3x3_strided(_p(x), _p(col), N, H, W, Cc, stride, Kpad, _stream()), "im2col3x3_strided")


def geglu(x, y, rows, inner):
    L.check(L.lib().ln3d_geglu(_p(x), _p(y), rows, inner, _stream()), "geglu")


def attention_small(q, k, v, out, B, H, Nq, Nk, Dh, ldq, ldk, ldv, scale):
    """q / k / v: bf16 tensors (or views into wider projection outputs) whose data_ptr is column 0 of head 0; ld* = their row strides"""
    L.check(L.lib().ln3d_attention_small(_p(q), _p(k), _p(v), _p(out), B, H, Nq, Nk, Dh, ldq, ldk, ldv, scale, _stream()), "attention_small")


def nchw_to_cl_bf16(x, y, N, Cc, HW, Cpad):
    L.check(L.lib().ln3d_nchw_to_cl_bf16(_p(x), _p(y), N, Cc, HW, Cpad, _stream()), "nchw_to_cl_bf16")


def cl_to_nchw_f32(x, y, N, Cc, HW):
    L.check(L.lib().ln3d_cl_to_nchw_f32(_p(x), _p(y), N, Cc, HW, _stream()), "cl_to_nchw_f32")


def mix_prediction(eps, x, mixing_logit, sqrt_one_minus_ab, N, Cc, HW):
    L.check(L.lib().ln3d_mix_prediction(_p(eps), _p(x), _p(mixing_logit), sqrt_one_minus_ab, N, Cc, HW, _stream()), "mix_prediction")


# ---------------------------------------------------------------- multi-view VAE encoder (include/ln3d_encoder.h, csrc/conv_ops.hip)
def im2col3x3_pad01(x, col, N, H, W, Cc, Kpad):
    """Downsample of the encoder: F.pad(x, (0, 1, 0, 1)) + 3x3 conv stride 2 padding 0, as an im2col gather ([N*Ho*Wo, Kpad] bf16)."""
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    if x.numel() < N * H * W * Cc or col.numel() < N * Ho * Wo * Kpad:
        raise ValueError("im2col3x3_pad01: buffers smaller than the problem")
    L.check(L.lib().ln3d_im2col3x3_pad01(_p(x), _p(col), N, H, W, Cc, Kpad, _stream()), "im2col3x3_pad01")


def _channel_last_view(h):
    """h: [N, C, H, W] whose memory is channel-last ([N, H, W, C] contiguous) - what Encoder.forward_frames returns."""
    N, Cc, H, W = h.shape
    return h.stride() == (H * W * Cc, 1, W * Cc, Cc)


def frame_mean(h, out, B, F, HW, Cc):
    """h [B*F, C, H, W] (channel-last memory) -> out f32 [B, C, H, W] contiguous: mean over each object's F frames."""
    if h.dtype != torch.float32 or out.dtype != torch.float32 or not _channel_last_view(h) or not out.is_contiguous():
        raise ValueError("frame_mean: h must be an f32 channel-last [B*F, C, H, W] view, out a contiguous f32 tensor")
    if h.shape[0] != B * F or h.shape[1] != Cc or h.shape[2] * h.shape[3] != HW or out.numel() != B * Cc * HW:
        raise ValueError("frame_mean: shapes do not match (B, F, HW, C)")
    L.check(L.lib().ln3d_frame_mean(_p(h), _p(out), B, F, HW, Cc, _stream()), "frame_mean")


def mv_posterior(h, qw, qb, eps, B, F, E=4):
    """Fused posterior (ln3d_mv_posterior): h [B*F, 6E, H, W] f32 of any strides with a uniform pixel stride (the per-frame channel-last
    encoder output, or the pooled NCHW one with F = 1); qw [6E, 2E] / qb [6E] f32 (quant_conv); eps f32 [B, E, 3, H*W] or None (mode).
    Returns dict of f32 tensors: mean, logvar, z, log_q, entropy [B, E, 3, H*W] and latent_tok [B, 3*H*W, E] (E = ldm_embed_dim)."""
    N, Cm, H, W = h.shape
    HW = H * W
    if h.dtype != torch.float32 or N != B * F or Cm != 6 * E or h.stride(2) != W * h.stride(3):
        raise ValueError(f"mv_posterior: h {tuple(h.shape)} / strides {h.stride()}: expected f32 [{B * F}, {6 * E}, H, W] with a uniform pixel stride")
    if qw.dtype != torch.float32 or qw.numel() != 12 * E * E or not qw.is_contiguous() or qb.numel() != 6 * E or not qb.is_contiguous():
        raise ValueError("mv_posterior: quant_conv weight [6E, 2E] / bias [6E] must be contiguous f32")
    if eps is not None and (eps.dtype != torch.float32 or tuple(eps.shape) != (B, E, 3, HW) or not eps.is_contiguous()):
        raise ValueError(f"mv_posterior: eps must be a contiguous f32 [{B}, {E}, 3, {HW}] tensor")
    out = {k: torch.empty(B, E, 3, HW, device=h.device, dtype=torch.float32) for k in ('mean', 'logvar', 'z', 'log_q', 'entropy')}
    out['latent_tok'] = torch.empty(B, 3 * HW, E, device=h.device, dtype=torch.float32)
    L.check(L.lib().ln3d_mv_posterior(_p(h), h.stride(0), h.stride(3), h.stride(1), _p(qw), _p(qb), _p(eps),
                                      _p(out['mean']), _p(out['logvar']), _p(out['z']), _p(out['latent_tok']), _p(out['log_q']),
                                      _p(out['entropy']), B, F, HW, E, _stream()), "mv_posterior")
    return out


# ---------------------------------------------------------------- ShapeNet VAE decoder class (include/ln3d_shapenet.h, csrc/shapenet_ops.hip)
def _need(cond, msg):
    if not cond:
        raise ValueError(msg)


def triplane_axis_attention(qkv, out, B, p, H, scale=None):
    """qkv f32 [B*3*p*p, >= 3*H*64] ([q | k | v] columns) -> out bf16 [B*3*p*p, H*64]: plane i's query at (y, x) attends to row y of
    plane (i+1) % 3 and column x of plane (i+2) % 3 (Conv3DCrossAttentionBlockXformerMHANested)."""
    rows, D = B * 3 * p * p, H * 64
    _need(qkv.dtype == torch.float32 and qkv.stride(-1) == 1 and qkv.shape[0] == rows and qkv.shape[1] >= 3 * D,
          "triplane_axis_attention: qkv must be f32 [B*3*p*p, >= 3*H*64] with unit column stride")
    _need(out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == rows * D, "triplane_axis_attention: out bf16 [rows, H*64]")
    L.check(L.lib().ln3d_triplane_axis_attention(_p(qkv), qkv.stride(0), _p(out), B, p, H, scale or 64 ** -0.5,
                                                 _stream()), "triplane_axis_attention")


def sr_unpatchify(pred, planes, mixed, B, S, P, Cc):
    n = B * 3 * S * P * S * P * Cc
    _need(pred.dtype == torch.float32 and pred.is_contiguous() and pred.numel() == n, "sr_unpatchify: pred f32 [B, 3*S*S, P*P*C]")
    _need(planes.dtype == torch.float32 and planes.is_contiguous() and planes.numel() == n, "sr_unpatchify: planes f32 [B, 3, R, R, C]")
    _need(mixed.dtype == torch.bfloat16 and mixed.is_contiguous() and mixed.numel() == n, "sr_unpatchify: mixed bf16 [B, 3, R, R, C]")
    L.check(L.lib().ln3d_sr_unpatchify(_p(pred), _p(planes), _p(mixed), B, S, P, Cc, _stream()), "sr_unpatchify")


def resize_bilinear_cl(x, y, N, h, w, Ho, Wo, Cc, transpose=False):
    _need(x.dtype == torch.float32 and x.is_contiguous() and x.numel() == N * h * w * Cc, "resize_bilinear_cl: x f32 [N, h, w, C]")
    _need(y.dtype == torch.bfloat16 and y.is_contiguous() and y.numel() == N * Ho * Wo * Cc, "resize_bilinear_cl: y bf16 [N, Ho, Wo, C]")
    L.check(L.lib().ln3d_resize_bilinear_cl(_p(x), _p(y), N, h, w, Ho, Wo, Cc, transpose, _stream()), "resize_bilinear_cl")


def resize_add_lrelu(base, t, out, N, h, w, Ho, Wo, Cc, slope=0.01):
    _need(base.dtype == torch.float32 and base.is_contiguous() and base.numel() == N * h * w * Cc, "resize_add_lrelu: base f32 [N, h, w, C]")
    for z in (t, out):
        _need(z.dtype == torch.float32 and z.is_contiguous() and z.numel() == N * Ho * Wo * Cc, "resize_add_lrelu: t / out f32 [N, Ho, Wo, C]")
    L.check(L.lib().ln3d_resize_add_lrelu(_p(base), _p(t), _p(out), N, h, w, Ho, Wo, Cc, slope, _stream()), "resize_add_lrelu")


def rollout_means(x, rowmean, colmean, N, H, W, Cc):
    _need(x.is_contiguous() and x.numel() == N * H * W * Cc and rowmean.numel() == N * H * Cc and colmean.numel() == N * W * Cc,
          "rollout_means: x [N, H, W, C], rowmean [N, H, C], colmean [N, W, C] (f32, contiguous)")
    if x.dtype == torch.bfloat16:                # include/ln3d_ffhq.h: the same means of bf16 planes
        return L.check(L.lib().ln3d_rollout_means_bf16(_p(x), _p(rowmean), _p(colmean), N, H, W, Cc, _stream()), "rollout_means_bf16")
    L.check(L.lib().ln3d_rollout_means(_p(x), _p(rowmean), _p(colmean), N, H, W, Cc, _stream()), "rollout_means")


def im2col3x3_rollout(x, rowmean, colmean, col, plane, H, W, Cc, Kpad):
    """x f32 [3, H, W, C] (one object), rowmean [3, H, C], colmean [3, W, C] -> col bf16 [H*W, Kpad] of plane `plane`'s roll-out conv."""
    _need(x.dtype == torch.float32 and x.is_contiguous() and x.numel() == 3 * H * W * Cc, "im2col3x3_rollout: x f32 [3, H, W, C]")
    _need(rowmean.is_contiguous() and rowmean.numel() == 3 * H * Cc and colmean.is_contiguous() and colmean.numel() == 3 * W * Cc,
          "im2col3x3_rollout: rowmean [3, H, C] / colmean [3, W, C]")
    _need(col.dtype == torch.bfloat16 and col.is_contiguous() and col.numel() == H * W * Kpad, "im2col3x3_rollout: col bf16 [H*W, Kpad]")
    L.check(L.lib().ln3d_im2col3x3_rollout(_p(x), _p(rowmean), _p(colmean), _p(col), plane, H, W, Cc, Kpad, _stream()), "im2col3x3_rollout")


def conv3x3_rollout(x, rowmean, colmean, w, bias, base, out, H, W, Cc, Cout, slope=0.01):
    """Fused roll-out 3x3 conv of one object (include/ln3d_ffhq.h): x f32 / bf16 [3, H, W, C], rowmean [3, H, C], colmean [3, W, C],
    w bf16 [3, Cout, 27C], bias f32 [3, Cout], base f32 [3, h, w, Cout] (resized when h, w differ from H, W) -> out f32 [3, H, W, Cout]
    = base + leaky_relu(conv + bias)."""
    _need(x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous() and x.numel() == 3 * H * W * Cc, "conv3x3_rollout: x f32 / bf16 [3, H, W, C]")
    for z, n, what in ((rowmean, 3 * H * Cc, "rowmean f32 [3, H, C]"), (colmean, 3 * W * Cc, "colmean f32 [3, W, C]"), (bias, 3 * Cout, "bias f32 [3, Cout]"),
                       (out, 3 * H * W * Cout, "out f32 [3, H, W, Cout]")):
        _need(z.dtype == torch.float32 and z.is_contiguous() and z.numel() == n, "conv3x3_rollout: " + what)
    _need(w.dtype == torch.bfloat16 and w.is_contiguous() and w.numel() == 3 * Cout * 27 * Cc, "conv3x3_rollout: w bf16 [3, Cout, 27C]")
    _need(base.dtype == torch.float32 and base.is_contiguous() and base.dim() == 4 and base.shape[0] == 3 and base.shape[3] == Cout,
          "conv3x3_rollout: base f32 [3, h, w, Cout]")
    _need(out.data_ptr() != x.data_ptr(), "conv3x3_rollout: out must not be x")
    L.check(L.lib().ln3d_conv3x3_rollout_bf16(_p(x), x.dtype == torch.bfloat16, _p(rowmean), _p(colmean), _p(w), _p(bias), _p(base),
                                              base.shape[1], base.shape[2], _p(out), H, W, Cc, Cout, slope, _stream()), "conv3x3_rollout")
