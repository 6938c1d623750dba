"""C-ABI contract without a GPU: every entry point of include/ln3d.h and of the stage headers (ln3d_shapenet.h, ln3d_encoder.h,
ln3d_ffhq.h, ln3d_mx.h) rejects missing buffers with LN3D_ERR_BAD_ARG BEFORE it touches the device (argument validation is not a
compute call; nothing is launched here).  The tables must cover every `int ln3d_*(...)` declared in each header, so a new export
without validation shows up as a failing test.  The mesh simplification (ln3d_meshsimplify.h) is held to more: every entry point returns
LN3D_ERR_BAD_ARG for each null buffer, each zero, negative or oversize count and each bad cell / origin, and LN3D_ERR_UNSUPPORTED for
nc = 2^21 + 1, all on fake addresses that are never dereferenced."""
import ctypes as C
import os
import re

from abi_args import BAD_ARG, UNSUPPORTED, refuses_null_buffers_and_bad_counts, with_args as _with
from conftest import ROOT

N = None
F, I64 = C.c_float, C.c_int64
NULL_CALLS = {
    'ln3d_gemm_bf16': (N, N),
    'ln3d_attention_bf16': (N, N),
    'ln3d_norm_modulate': (N, N),
    'ln3d_render_triplane': (N, N),
    'ln3d_embed_tokens': (N, N, N, N, 1, 1, 4, 1, N),
    'ln3d_layernorm_f32': (N, N, N, N, I64(1), 128, F(1e-5), N),
    'ln3d_vit_patchify': (N, N, 1, 224, 14, 640, 3, N),
    'ln3d_plucker_rays': (N, N, 1, 224, N),
    'ln3d_vit_assemble': (N, N, N, N, N, 1, 1, 0, 128, N),
    'ln3d_image_preprocess': (N, N, N, 1, 3, 8, 8, 4, 1, N, N, N),
    'ln3d_rmsnorm_heads_bf16': (N, N, I64(1), 64, 64, F(1e-5), N),
    'ln3d_timestep_embedding': (N, N, 1, 256, N),
    'ln3d_add_act_cast': (N, N, N, N, I64(1), 0, N),
    'ln3d_cast_f32_bf16': (N, N, I64(1), N),
    'ln3d_patch_embed': (N, N, N, N, N, N, 1, 1, 4, 32, 2, 128, N),
    'ln3d_patch_embed_triplane': (N, N, N, N, N, 1, 4, 32, 2, 128, N),
    'ln3d_tile_rows': (N, N, I64(1), 1, N),
    'ln3d_final_layer': (N, N, N, I64(0), N, N, N, N, N, 1, 4, 32, 2, 128, N),
    'ln3d_edm_euler_step': (N, N, F(1), F(1), F(1), I64(1), N),
    'ln3d_ddpm_step': (N, N, N, F(1), F(1), F(1), F(1), F(1), 0, I64(1), N),
    'ln3d_ddim_step': (N, N, N, N, F(1), F(1), F(1), F(1), F(1), F(1), 0, I64(1), N),
    'ln3d_flow_euler_step': (N, N, F(1), F(1), I64(1), N),
    'ln3d_add_table_rows': (N, N, N, 1, 1, I64(4), N),
    'ln3d_cfg_combine_dup': (N, F(1), I64(1), N),
    'ln3d_lincomb': (N, N, N, 1, N, I64(1), N),
    'ln3d_err_ratio_sq': (N, N, N, F(1), F(1), N, I64(1), N),
    'ln3d_axpby': (N, N, F(1), F(1), I64(1), N),
    'ln3d_planes_to_channel_last': (N, N, 1, 32, 8, 8, N),
    'ln3d_planes_to_nchw': (N, N, 1, 32, 8, 8, N),
    'ln3d_query_points': (N, 8, 8, N, I64(1), N, N, N, N, F(0.9), N, N, N, N),
    'ln3d_mesh_count': (N, 8, F(1), N, N),
    'ln3d_mcubes_count': (N, 8, F(1), N, N),
    'ln3d_mcubes_emit': (N, 8, F(1), N, N, N, N),
    'ln3d_mesh_emit': (N, 8, F(1), N, N, N, N),
    'ln3d_groupnorm_swish': (N, N, N, N, N, 1, 64, 64, 32, F(1e-6), 1, N),
    'ln3d_im2col3x3': (N, N, 1, 8, 8, 64, 1, 576, N),
    'ln3d_probe_mfma_bf16': (N, 1, 1, N),
    'ln3d_groupnorm_any': (N, N, N, N, N, N, N, 1, 16, 64, 32, F(1e-5), 1, N),
    'ln3d_im2col3x3_strided': (N, N, 1, 8, 8, 64, 2, 576, N),
    'ln3d_geglu': (N, N, I64(1), 64, N),
    'ln3d_attention_small': (N, N, N, N, 1, 1, 16, 16, 40, I64(40), I64(40), I64(40), F(0.1), N),
    'ln3d_nchw_to_cl_bf16': (N, N, 1, 12, 64, 16, N),
    'ln3d_cl_to_nchw_f32': (N, N, 1, 12, 64, N),
    'ln3d_mix_prediction': (N, N, N, F(0.5), 1, 12, 64, N),
}
# the stage headers, walked the same way
STAGE_NULL_CALLS = {
    'ln3d_shapenet.h': {
        'ln3d_triplane_axis_attention': (N, I64(192), N, 1, 4, 1, F(0.125), N),
        'ln3d_sr_unpatchify': (N, N, N, 1, 2, 2, 4, N),
        'ln3d_resize_bilinear_cl': (N, N, 1, 4, 4, 8, 8, 4, 0, N),
        'ln3d_resize_add_lrelu': (N, N, N, 1, 4, 4, 8, 8, 4, F(0.01), N),
        'ln3d_rollout_means': (N, N, N, 1, 4, 4, 4, N),
        'ln3d_im2col3x3_rollout': (N, N, N, N, 0, 4, 4, 4, 108, N),
    },
    'ln3d_encoder.h': {
        'ln3d_im2col3x3_pad01': (N, N, 1, 8, 8, 8, 72, N),
        'ln3d_frame_mean': (N, N, 1, 1, 4, 24, N),
        'ln3d_mv_posterior': (N, I64(96), I64(1), I64(4), N, N, N, N, N, N, N, N, N, 1, 1, 4, 4, N),
    },
    'ln3d_ffhq.h': {
        'ln3d_conv3x3_rollout_bf16': (N, 0, N, N, N, N, N, 8, 8, N, 8, 8, 16, 32, F(0.01), N),
        'ln3d_rollout_means_bf16': (N, N, N, 1, 4, 4, 4, N),
    },
    'ln3d_mx.h': {
        'ln3d_quantize_mx': (N, 0, I64(32), 1, 32, N, I64(32), N, I64(1), N),
        'ln3d_gemm_mxfp8': (N, N),
        'ln3d_norm_modulate_mx': (N, N, N),
    },
}
NOT_A_KERNEL = {'ln3d_abi_version', 'ln3d_gemm_heads_norm_fusable', 'ln3d_device_cus'}      # pure host queries

# Sizes <= 0 are bad arguments too, not zero-sized grids: every buffer below is a fake, never dereferenced address, so on a correct
# library nothing is launched
P = C.c_void_p(0x10000)
ZERO_CALLS = [
    ('ln3d_tile_rows', (P, P, I64(4), 0, N)),
    ('ln3d_tile_rows', (P, P, I64(0), 3, N)),
    ('ln3d_add_table_rows', (P, P, P, 0, 1, I64(4), N)),
    ('ln3d_add_table_rows', (P, P, P, 1, 0, I64(4), N)),
    ('ln3d_add_table_rows', (P, P, P, 1, 1, I64(0), N)),
    ('ln3d_timestep_embedding', (P, P, 0, 256, N)),
    ('ln3d_cast_f32_bf16', (P, P, I64(0), N)),
    ('ln3d_groupnorm_swish', (P, P, P, P, P, 0, 64, 64, 32, F(1e-6), 1, N)),
    ('ln3d_groupnorm_swish', (P, P, P, P, P, 1, 0, 64, 32, F(1e-6), 1, N)),
    ('ln3d_groupnorm_swish', (P, P, P, P, P, 1, 64, 64, 0, F(1e-6), 1, N)),
    ('ln3d_im2col3x3', (P, P, 0, 8, 8, 64, 1, 576, N)),
    ('ln3d_im2col3x3', (P, P, 1, 0, 8, 64, 1, 576, N)),
    ('ln3d_im2col3x3', (P, P, 1, 8, 0, 64, 1, 576, N)),
    ('ln3d_planes_to_channel_last', (P, P, 0, 32, 8, 8, N)),
    ('ln3d_planes_to_channel_last', (P, P, 1, 32, 0, 8, N)),
    ('ln3d_planes_to_nchw', (P, P, 0, 32, 8, 8, N)),
    ('ln3d_planes_to_nchw', (P, P, 1, 32, 8, 0, N)),
    ('ln3d_patch_embed_triplane', (P, P, P, P, P, 0, 4, 32, 2, 128, N)),
    ('ln3d_patch_embed_triplane', (P, P, P, P, P, 1, 4, 32, 0, 128, N)),
]
# the iso-surface passes: 2 <= G <= LN3D_MESH_MAX_GRID = 1448 (a vertex key is gid[a] * G^3 + gid[b] < G^6, and 1449^6 > 2^63)
for _name, _args in [('ln3d_mesh_count', (P, 8, F(1), P, N)), ('ln3d_mcubes_count', (P, 8, F(1), P, N)),
                     ('ln3d_mcubes_emit', (P, 8, F(1), P, P, P, N)), ('ln3d_mesh_emit', (P, 8, F(1), P, P, P, N))]:
    ZERO_CALLS += [(_name, _args[:1] + (g,) + _args[2:]) for g in (1449, 2048, 1 << 30, 1, 0, -1)]


def _sizes_zeroed(name, args, positions):
    """one row per size argument at `positions` of the otherwise valid call `args`, set to 0 and to -1 (keeping its C type)"""
    for i in positions:
        for bad in (0, -1):
            a = list(args)
            a[i] = type(a[i])(bad) if not isinstance(a[i], int) else bad
            yield (name, tuple(a))


# every size argument of the U-Net, VAE-decoder, encoder and DiT-boundary glue kernels (tests/test_stage_kernels_gpu.py)
for _name, _args, _pos in [
    ('ln3d_attention_small', (P, P, P, P, 1, 1, 16, 16, 40, I64(40), I64(40), I64(40), F(0.1), N), (4, 5, 6, 7, 8)),
    ('ln3d_triplane_axis_attention', (P, I64(192), P, 1, 4, 1, F(0.125), N), (3, 4, 5)),
    ('ln3d_geglu', (P, P, I64(1), 64, N), (2, 3)),
    ('ln3d_mix_prediction', (P, P, P, F(0.5), 1, 12, 64, N), (4, 5, 6)),
    ('ln3d_im2col3x3_strided', (P, P, 1, 8, 8, 64, 2, 576, N), (2, 3, 4, 5, 6)),
    ('ln3d_im2col3x3_pad01', (P, P, 1, 8, 8, 8, 72, N), (2, 3, 4, 5)),
    ('ln3d_im2col3x3_rollout', (P, P, P, P, 0, 4, 4, 4, 108, N), (5, 6, 7)),
    ('ln3d_nchw_to_cl_bf16', (P, P, 1, 12, 64, 16, N), (2, 3, 4)),
    ('ln3d_cl_to_nchw_f32', (P, P, 1, 12, 64, N), (2, 3, 4)),
    ('ln3d_sr_unpatchify', (P, P, P, 1, 2, 2, 4, N), (3, 4, 5, 6)),
    ('ln3d_resize_bilinear_cl', (P, P, 1, 4, 4, 8, 8, 4, 0, N), (2, 3, 4, 5, 6, 7)),
    ('ln3d_resize_add_lrelu', (P, P, P, 1, 4, 4, 8, 8, 4, F(0.01), N), (3, 4, 5, 6, 7, 8)),
    ('ln3d_rollout_means', (P, P, P, 1, 4, 4, 4, N), (3, 4, 5, 6)),
    ('ln3d_rollout_means_bf16', (P, P, P, 1, 4, 4, 4, N), (3, 4, 5, 6)),
    ('ln3d_frame_mean', (P, P, 1, 1, 4, 24, N), (2, 3, 4, 5)),
    ('ln3d_mv_posterior', (P, I64(96), I64(1), I64(4), P, P, P, P, P, P, P, P, P, 1, 1, 4, 4, N), (13, 14, 15, 16)),
    ('ln3d_patch_embed', (P, P, P, P, P, P, 1, 1, 4, 32, 2, 128, N), (6, 7, 8, 9, 10, 11)),
    ('ln3d_final_layer', (P, P, P, I64(256), P, P, P, P, P, 1, 4, 32, 2, 128, N), (9, 10, 11, 12, 13)),
    ('ln3d_rmsnorm_heads_bf16', (P, P, I64(1), 64, 64, F(1e-5), N), (2, 3)),
]:
    ZERO_CALLS += list(_sizes_zeroed(_name, _args, _pos))
ZERO_CALLS += [
    ('ln3d_final_layer', (P, P, P, I64(256), P, P, P, P, P, 1, 4, 33, 2, 128, N)),           # S % p != 0
    ('ln3d_patch_embed', (P, P, P, P, P, P, 1, 1, 4, 33, 2, 128, N)),
]


# ---- the ray-marcher: every size or scale csrc/render.hip indexes with or divides by.  (field, value) rows on an otherwise valid
# ln3d_render_args (fake, never dereferenced addresses) and the code each must return before any launch.
def _render_args(**kw):
    from ln3diff_amd._lib import RenderArgs
    a = RenderArgs()
    for k in ('planes', 'plane_index', 'cams', 'dec_w0', 'dec_b0', 'dec_w1', 'dec_b1', 'jitter', 'u_fine', 'rgb', 'depth', 'wsum', 'ray_limits',
              'scalars'):
        setattr(a, k, 0x10000)
    a.H, a.W, a.V, a.res, a.box_warp, a.bbox_min, a.bbox_max = 8, 8, 1, 4, 0.9, -0.45, 0.45
    for k, v in kw.items():
        setattr(a, k, v)
    return a


RENDER_ROWS = [
    (dict(H=0), BAD_ARG), (dict(H=-1), BAD_ARG), (dict(W=0), BAD_ARG), (dict(W=-8), BAD_ARG),
    (dict(H=1 << 15, W=1 << 15), BAD_ARG),                                        # 32-bit tap offsets
    (dict(box_warp=0.0), BAD_ARG), (dict(box_warp=-0.9), BAD_ARG), (dict(box_warp=float('nan')), BAD_ARG), (dict(box_warp=float('inf')), BAD_ARG),
    (dict(V=0), BAD_ARG), (dict(V=-1), BAD_ARG),
    (dict(res=0), BAD_ARG), (dict(res=-2), BAD_ARG), (dict(res=-2, rays_per_view=4), BAD_ARG), (dict(res=0, rays_per_view=16), BAD_ARG),
    (dict(res=1 << 16), BAD_ARG),                                                 # res * res is an int
    (dict(rays_per_view=-1), BAD_ARG), (dict(rays_per_view=15), BAD_ARG),         # camera rays are a res x res image
    (dict(cams=None), BAD_ARG), (dict(ray_o=0x10000), BAD_ARG), (dict(ray_d=0x10000), BAD_ARG),
    (dict(cams=None, ray_o=0x10000, ray_d=0x10000, res=0, rays_per_view=0), BAD_ARG),
    (dict(cams=None, ray_o=0x10000, ray_d=0x10000, res=0, rays_per_view=-5), BAD_ARG),
    (dict(depth_resolution=3), UNSUPPORTED), (dict(depth_resolution=129), UNSUPPORTED), (dict(depth_resolution=-64), UNSUPPORTED),
    (dict(depth_resolution_importance=129), UNSUPPORTED), (dict(depth_resolution_importance=-1), UNSUPPORTED),
    (dict(ray_mode=1, ray_start=1.0, ray_end=1.0), BAD_ARG), (dict(ray_mode=1, ray_start=1.8, ray_end=0.6), BAD_ARG),
    (dict(ray_mode=1, ray_start=0.6, ray_end=float('nan')), BAD_ARG),
    (dict(V=2000, views_per_call=1), BAD_ARG),                                    # more call groups than the scratch holds
]
QUERY_OK = (P, 8, 8, P, I64(4), P, P, P, P, F(0.9), P, P, P, N)
QUERY_ROWS = [{1: 0}, {1: -1}, {2: 0}, {2: -3}, {1: 1 << 15, 2: 1 << 15}, {4: I64(0)}, {4: I64(-1)}, {9: F(0.0)}, {9: F(-1.0)},
              {9: F(float('nan'))}, {9: F(float('inf'))}, {5: N}, {6: N}, {7: N}, {8: N}, {10: N}, {11: N}, {12: N}]


def test_render_and_query_arguments_are_validated(hip_lib):
    """H, W <= 0 and box_warp <= 0 or non-finite were accepted by both entry points (H = 0 clamps tap coordinates to -1, box_warp = 0
    makes coord_scale infinite), so were res < 0 with rays_per_view = res^2, rays_per_view < 0, negative sample counts (silently 64)
    and, in ln3d_query_points, missing decoder weights (dereferenced by the init kernel)."""
    from ln3diff_amd._lib import RENDER_MAX_CALLS
    assert RENDER_MAX_CALLS < 2000
    for kw, code in RENDER_ROWS:
        assert hip_lib.ln3d_render_triplane(C.byref(_render_args(**kw)), None) == code, (kw, code)
    for row in QUERY_ROWS:
        a = list(QUERY_OK)
        for i, v in row.items():
            a[i] = v
        assert hip_lib.ln3d_query_points(*a) == BAD_ARG, row


def test_every_entry_point_rejects_missing_buffers(hip_lib):
    hdr = open(os.path.join(ROOT, 'include', 'ln3d.h')).read()
    declared = set(re.findall(r'^int (ln3d_[a-z0-9_]+)\(', hdr, re.M))
    assert declared - NOT_A_KERNEL == set(NULL_CALLS), (declared - NOT_A_KERNEL) ^ set(NULL_CALLS)
    for name, args in NULL_CALLS.items():
        rc = getattr(hip_lib, name)(*args)
        assert rc == -1, (name, rc)                                       # LN3D_ERR_BAD_ARG
    assert b'bad argument' in hip_lib.ln3d_strerror(-1)


def test_every_stage_entry_point_rejects_missing_buffers(hip_lib):
    for header, calls in STAGE_NULL_CALLS.items():
        hdr = open(os.path.join(ROOT, 'include', header)).read()
        declared = set(re.findall(r'^int (ln3d_[a-z0-9_]+)\(', hdr, re.M))
        assert declared == set(calls), (header, declared ^ set(calls))
        for name, args in calls.items():
            rc = getattr(hip_lib, name)(*args)
            assert rc == -1, (header, name, rc)                               # LN3D_ERR_BAD_ARG


def test_host_queries(hip_lib):
    assert hip_lib.ln3d_abi_version() == 10
    # the fused qk-norm epilogue needs head-aligned tiles: 64-wide heads yes, 72-in-128 padded heads no
    assert hip_lib.ln3d_gemm_heads_norm_fusable(12288, 3072, 768, 64, 64) == 1
    assert hip_lib.ln3d_gemm_heads_norm_fusable(12288, 3 * 16 * 128, 768, 72, 128) == 0


def test_gate_residual_row_arguments_are_validated(hip_lib):
    """the GATE_RES epilogue reads float4 quads at gate / res_bias + (row / gate_rows) * ld + feature - a leading dimension
    that is not a multiple of 4, a misaligned pointer or gate_rows left at 0 next to a per-sample buffer is a bad argument, not an
    out-of-bounds read.  Validation happens before anything touches the device (fake, never dereferenced addresses)."""
    from ln3diff_amd._lib import GemmArgs, EPI_GATE_RES
    base = dict(X=0x10000, ldx=64, W=0x20000, ldw=64, M=192, N=256, K=64, epilogue=EPI_GATE_RES, out0=0x30000, ldo=256)
    bad = [dict(gate=0x40000, gate_rows=96, gate_ld=258),              # ld % 4
           dict(gate=0x40004, gate_rows=96, gate_ld=256),              # pointer not 16-byte aligned
           dict(gate=0x40000, gate_rows=0, gate_ld=256),               # rows per sample missing
           dict(res_bias=0x50000, res_bias_ld=255, gate_rows=96),
           dict(res_bias=0x50008, res_bias_ld=256, gate_rows=96),
           dict(res_bias=0x50000, res_bias_ld=256, gate_rows=0)]
    for extra in bad:
        a = GemmArgs(**dict(base, **extra))
        assert hip_lib.ln3d_gemm_bf16(C.byref(a), None) == -1, extra


def test_zero_sizes_are_bad_arguments(hip_lib):
    for name, args in ZERO_CALLS:
        assert getattr(hip_lib, name)(*args) == -1, (name, args)              # LN3D_ERR_BAD_ARG, before any launch


def test_merged_glue_kernels_keep_every_front_refusal(hip_lib):
    """One kernel serves the three im2col fronts, both plane layouts and both roll-out means: each front still refuses what only it
    refuses, and the f32 entry points refuse the grid limits their f16 / bf16 twins always did.  Fake addresses: nothing launches."""
    assert hip_lib.ln3d_im2col3x3(P, P, 1, 8, 8, 64, 3, 576, N) == -1                     # upsample in {1, 2}
    assert hip_lib.ln3d_im2col3x3_strided(P, P, 1, 8, 8, 64, 3, 576, N) == -1             # stride in {1, 2}
    assert hip_lib.ln3d_im2col3x3_pad01(P, P, 1, 1, 8, 64, 576, N) == -1                  # H >= 2
    for entry in (hip_lib.ln3d_planes_to_channel_last, hip_lib.ln3d_planes_to_channel_last_f16):
        assert entry(P, P, 21846, 32, 8, 8, N) == -1                                      # NP * 3 > 65535, the grid's y extent
        assert entry(P, P, 1, 32, 46341, 46341, N) == -1                                  # H * W + 31 is no int
    for entry in (hip_lib.ln3d_rollout_means, hip_lib.ln3d_rollout_means_bf16):
        assert entry(P, P, P, 65536, 8, 8, 32, N) == -1                                   # N > 65535, the grid's y extent


# ---- the mesh simplification (include/ln3d_meshsimplify.h): name -> (a valid argument list on fake addresses, indices of its buffers,
# indices of its counts)
A = 0x10000                                  # a fake device address
NAN, INF = float('nan'), float('inf')
VALID = {
    'ln3d_simplify_keys': ([A, 5, 0.0, -1.0, 2.0, 0.5, A, None], (0, 6), (1,)),
    'ln3d_simplify_mean': ([A, A, A, 9, 4, A, None], (0, 1, 2, 5), (3, 4)),
    'ln3d_simplify_faces': ([A, 7, A, 9, 4, A, A, None], (0, 2, 5, 6), (1, 3, 4)),
    'ln3d_simplify_first': ([A, A, 7, A, None], (0, 1, 3), (2,)),
    'ln3d_simplify_used': ([A, A, 7, 4, A, None], (0, 1, 4), (2, 3)),
}
NC_AT = {'ln3d_simplify_mean': 4, 'ln3d_simplify_faces': 4, 'ln3d_simplify_used': 3}          # where nc stands
NV_AT = {'ln3d_simplify_mean': 3, 'ln3d_simplify_faces': 3}                                   # nc <= nv is checked: raise nv with it


def test_every_entry_point_validates_before_it_launches(hip_lib):
    assert set(VALID) == {'ln3d_simplify_faces', 'ln3d_simplify_first', 'ln3d_simplify_keys', 'ln3d_simplify_mean', 'ln3d_simplify_used'}
    for name, (args, buffers, counts) in VALID.items():
        refuses_null_buffers_and_bad_counts(getattr(hip_lib, name), name, args, buffers, counts)
    keys, kargs = hip_lib.ln3d_simplify_keys, VALID['ln3d_simplify_keys'][0]
    for cell in (0.0, -0.0, -1.0, NAN, INF, -INF):
        assert keys(*_with(kargs, i5=cell)) == BAD_ARG, cell
    for i in (2, 3, 4):
        for o in (NAN, INF, -INF):
            assert keys(*_with(kargs, **{'i%d' % i: o})) == BAD_ARG, (i, o)
    # more clusters than vertices cannot be
    assert hip_lib.ln3d_simplify_mean(*_with(VALID['ln3d_simplify_mean'][0], i3=4, i4=5)) == BAD_ARG
    assert hip_lib.ln3d_simplify_faces(*_with(VALID['ln3d_simplify_faces'][0], i3=4, i4=5)) == BAD_ARG
    # nc = 2^21 + 1: three cluster numbers no longer fit a face key; a null buffer still comes first
    for name, at in NC_AT.items():
        big = {'i%d' % at: (1 << 21) + 1}
        if name in NV_AT:
            big['i%d' % NV_AT[name]] = 1 << 22
        assert getattr(hip_lib, name)(*_with(VALID[name][0], **big)) == UNSUPPORTED, name
        assert getattr(hip_lib, name)(*_with(VALID[name][0], i0=None, **big)) == BAD_ARG, name
    assert b'bad argument' in hip_lib.ln3d_strerror(BAD_ARG) and hip_lib.ln3d_strerror(UNSUPPORTED)
