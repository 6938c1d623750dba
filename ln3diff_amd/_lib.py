"""ctypes binding of libln3d_hip.so (the C ABI of include/ln3d.h, include/ln3d_encoder.h, include/ln3d_shapenet.h, include/ln3d_mx.h, include/ln3d_ffhq.h,
include/ln3d_planes16.h, include/ln3d_normals.h and the include/ln3d_mesh*.h of the mesh post-processing: every header of include/).

Every export is declared once, in PROTOTYPES: name -> (restype, argtypes), which lib() applies, so a call site passes plain Python values
and a value of the wrong kind is a ctypes.ArgumentError.  One rule maps a C parameter to its argtype:
    const ln3d_*_args*  (one of the six argument structs)  -> POINTER(<its Structure below>)   (takes the Structure itself: ctypes passes
                                                              its address, and that is cheaper per call than byref(...) at the call site)
    any other pointer, device or host                      -> c_void_p   (takes an int address, None, a ctypes array, byref(...))
    int64_t -> c_int64        int -> c_int        float -> c_float        (void) -> no arguments
Results are c_int (0 or a negative LN3D_ERR_*), except ln3d_strerror (c_char_p) and ln3d_reload_env (void: None).
The headers are not read here: tests/test_abi_types_cpu.py parses them and compares the table, the six Structure layouts (against a
compiled offsetof probe) and the constants below with what they declare.

There is NO fallback: if the library is missing or a kernel launch fails the product raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libln3d_hip.so")

ABI_VERSION = 10
EPI_F32, EPI_BF16, EPI_GELU_ERF, EPI_GELU_TANH, EPI_SILU, EPI_GATE_RES, EPI_HEADS, EPI_F32_SILU, EPI_QUICK_GELU, EPI_CROSS_ATTN = range(10)
RENDER_SCRATCH_FLOATS = 16384
RENDER_MAX_CALLS = (RENDER_SCRATCH_FLOATS - 2644) // 8      # per-call range records after the decoder image (csrc/render.hip)

vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float


class GemmArgs(C.Structure):
    _fields_ = [("X", vp), ("ldx", i64), ("W", vp), ("ldw", i64), ("bias", vp),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32),
                ("out0", vp), ("out1", vp), ("out2", vp), ("ldo", i64),
                ("gate", vp), ("gate_rows", i32), ("gate_ld", i64),
                ("tokens", i32), ("tok_pad", i32), ("heads", i32), ("head_dim", i32),
                ("transpose_mask", i32), ("ctx_keys", i32), ("ctx_pad", i32), ("ctx_scale", f32), ("head_dim_pad", i32),
                ("head_norm0", vp), ("head_norm1", vp), ("head_norm_eps", f32),
                ("res_bias", vp), ("res_bias_ld", i64)]


class MxGemmArgs(C.Structure):          # ln3d_gemm_mx_args (include/ln3d_mx.h)
    _fields_ = [("Xq", vp), ("Xs", vp), ("ldx", i64), ("ldxs", i64),
                ("Wq", vp), ("Ws", vp), ("ldw", i64), ("ldws", i64), ("bias", vp),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32),
                ("out0", vp), ("out1", vp), ("out2", vp), ("ldo", i64), ("out_scale", vp), ("ldos", i64),
                ("gate", vp), ("gate_rows", i32), ("gate_ld", i64),
                ("tokens", i32), ("tok_pad", i32), ("heads", i32), ("head_dim", i32), ("transpose_mask", i32), ("head_dim_pad", i32)]


class AttnArgs(C.Structure):
    _fields_ = [("Q", vp), ("K", vp), ("Vt", vp), ("O", vp),
                ("B", i32), ("H", i32), ("Nq", i32), ("Nq_pad", i32), ("Nk", i32), ("Nk_pad", i32),
                ("Dh", i32), ("ldo", i64), ("scale", f32), ("causal", i32), ("Dh_true", i32)]


class NormArgs(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("rows", i64), ("D", i32), ("kind", i32), ("eps", f32),
                ("weight", vp), ("shift", vp), ("scale", vp), ("mod_rows", i32), ("mod_ld", i64),
                ("shift_table", vp), ("scale_table", vp), ("rows_in", i32), ("rows_out", i32)]


class RenderArgs(C.Structure):
    _fields_ = [("planes", vp), ("H", i32), ("W", i32), ("plane_index", vp), ("cams", vp),
                ("V", i32), ("res", i32), ("dec_w0", vp), ("dec_b0", vp), ("dec_w1", vp), ("dec_b1", vp),
                ("jitter", vp), ("u_fine", vp), ("box_warp", f32), ("bbox_min", f32), ("bbox_max", f32),
                ("white_back", i32), ("rgb", vp), ("depth", vp), ("wsum", vp), ("ray_limits", vp),
                ("scalars", vp), ("coarse_sigma", vp), ("fine_depths", vp), ("ray_o", vp), ("ray_d", vp),
                ("fine_sigma", vp), ("coarse_coords", vp), ("fine_coords", vp), ("views_per_call", i32),
                ("rays_per_view", i32), ("visibility", vp), ("depth_resolution", i32), ("depth_resolution_importance", i32),
                ("ray_mode", i32), ("ray_start", f32), ("ray_end", f32), ("no_bbox_filter", i32),
                ("weights", vp), ("all_coords", vp), ("feature_volume", vp)]


class NormalsArgs(C.Structure):         # ln3d_normals_args (include/ln3d_normals.h)
    _fields_ = [("planes", vp), ("H", i32), ("W", i32), ("plane_index", vp), ("cams", vp), ("V", i32), ("res", i32),
                ("ray_o", vp), ("ray_d", vp), ("rays_per_view", i32), ("dec_w0", vp), ("dec_b0", vp), ("dec_w1", vp), ("dec_b1", vp),
                ("box_warp", f32), ("depth", vp), ("wsum", vp), ("mask_threshold", f32), ("space", i32), ("normal", vp), ("points", vp),
                ("mode", i32), ("samples", i32), ("weights", vp), ("coords", vp), ("weight_floor", f32), ("accum", vp)]


def _int(*argtypes):
    return (C.c_int, argtypes)


_gemm, _gemm_mx, _attn, _norm = C.POINTER(GemmArgs), C.POINTER(MxGemmArgs), C.POINTER(AttnArgs), C.POINTER(NormArgs)
_render, _normals = C.POINTER(RenderArgs), C.POINTER(NormalsArgs)

PROTOTYPES = {
    # include/ln3d.h
    "ln3d_strerror": (C.c_char_p, (i32,)),
    "ln3d_abi_version": _int(),
    "ln3d_reload_env": (None, ()),
    "ln3d_device_cus": _int(),
    "ln3d_probe_mfma_bf16": _int(vp, i32, i32, vp),
    "ln3d_gemm_bf16": _int(_gemm, vp),
    "ln3d_gemm_heads_norm_fusable": _int(i32, i32, i32, i32, i32),
    "ln3d_attention_bf16": _int(_attn, vp),
    "ln3d_embed_tokens": _int(vp, vp, vp, vp, i32, i32, i32, i32, vp),
    "ln3d_layernorm_f32": _int(vp, vp, vp, vp, i64, i32, f32, vp),
    "ln3d_vit_patchify": _int(vp, vp, i32, i32, i32, i32, i32, vp),
    "ln3d_plucker_rays": _int(vp, vp, i32, i32, vp),
    "ln3d_vit_assemble": _int(vp, vp, vp, vp, vp, i32, i32, i32, i32, vp),
    "ln3d_image_preprocess": _int(vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp),
    "ln3d_rmsnorm_heads_bf16": _int(vp, vp, i64, i32, i32, f32, vp),
    "ln3d_norm_modulate": _int(_norm, vp),
    "ln3d_timestep_embedding": _int(vp, vp, i32, i32, vp),
    "ln3d_add_act_cast": _int(vp, vp, vp, vp, i64, i32, vp),
    "ln3d_cast_f32_bf16": _int(vp, vp, i64, vp),
    "ln3d_patch_embed": _int(vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp),
    "ln3d_patch_embed_triplane": _int(vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp),
    "ln3d_tile_rows": _int(vp, vp, i64, i32, vp),
    "ln3d_final_layer": _int(vp, vp, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp),
    "ln3d_edm_euler_step": _int(vp, vp, f32, f32, f32, i64, vp),
    "ln3d_ddpm_step": _int(vp, vp, vp, f32, f32, f32, f32, f32, i32, i64, vp),
    "ln3d_ddim_step": _int(vp, vp, vp, vp, f32, f32, f32, f32, f32, f32, i32, i64, vp),
    "ln3d_flow_euler_step": _int(vp, vp, f32, f32, i64, vp),
    "ln3d_add_table_rows": _int(vp, vp, vp, i32, i32, i64, vp),
    "ln3d_cfg_combine_dup": _int(vp, f32, i64, vp),
    "ln3d_lincomb": _int(vp, vp, vp, i32, vp, i64, vp),                    # ks, cs: host arrays
    "ln3d_err_ratio_sq": _int(vp, vp, vp, f32, f32, vp, i64, vp),
    "ln3d_axpby": _int(vp, vp, f32, f32, i64, vp),
    "ln3d_planes_to_channel_last": _int(vp, vp, i32, i32, i32, i32, vp),
    "ln3d_planes_to_nchw": _int(vp, vp, i32, i32, i32, i32, vp),
    "ln3d_render_triplane": _int(_render, vp),
    "ln3d_query_points": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, vp, vp, vp, vp),
    "ln3d_mesh_count": _int(vp, i32, f32, vp, vp),
    "ln3d_mcubes_count": _int(vp, i32, f32, vp, vp),
    "ln3d_mcubes_emit": _int(vp, i32, f32, vp, vp, vp, vp),
    "ln3d_mesh_emit": _int(vp, i32, f32, vp, vp, vp, vp),
    "ln3d_groupnorm_swish": _int(vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, vp),
    "ln3d_im2col3x3": _int(vp, vp, i32, i32, i32, i32, i32, i32, vp),
    "ln3d_groupnorm_any": _int(vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, vp),
    "ln3d_im2col3x3_strided": _int(vp, vp, i32, i32, i32, i32, i32, i32, vp),
    "ln3d_geglu": _int(vp, vp, i64, i32, vp),
    "ln3d_attention_small": _int(vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, f32, vp),
    "ln3d_nchw_to_cl_bf16": _int(vp, vp, i32, i32, i32, i32, vp),
    "ln3d_cl_to_nchw_f32": _int(vp, vp, i32, i32, i32, vp),
    "ln3d_mix_prediction": _int(vp, vp, vp, f32, i32, i32, i32, vp),
    # include/ln3d_encoder.h (the multi-view VAE encoder)
    "ln3d_im2col3x3_pad01": _int(vp, vp, i32, i32, i32, i32, i32, vp),
    "ln3d_frame_mean": _int(vp, vp, i32, i32, i32, i32, vp),
    "ln3d_mv_posterior": _int(vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp),
    # include/ln3d_shapenet.h (the ShapeNet VAE decoder class)
    "ln3d_triplane_axis_attention": _int(vp, i64, vp, i32, i32, i32, f32, vp),
    "ln3d_sr_unpatchify": _int(vp, vp, vp, i32, i32, i32, i32, vp),
    "ln3d_resize_bilinear_cl": _int(vp, vp, i32, i32, i32, i32, i32, i32, i32, vp),
    "ln3d_resize_add_lrelu": _int(vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp),
    "ln3d_rollout_means": _int(vp, vp, vp, i32, i32, i32, i32, vp),
    "ln3d_im2col3x3_rollout": _int(vp, vp, vp, vp, i32, i32, i32, i32, i32, vp),
    # include/ln3d_mx.h (the opt-in MX-FP8 GEMMs of the T23D DiT)
    "ln3d_quantize_mx": _int(vp, i32, i64, i32, i32, vp, i64, vp, i64, vp),
    "ln3d_gemm_mxfp8": _int(_gemm_mx, vp),
    "ln3d_norm_modulate_mx": _int(_norm, vp, vp),
    # include/ln3d_ffhq.h (the FFHQ VAE decoder class)
    "ln3d_conv3x3_rollout_bf16": _int(vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, i32, f32, vp),
    "ln3d_rollout_means_bf16": _int(vp, vp, vp, i32, i32, i32, i32, vp),
    # include/ln3d_planes16.h (the opt-in fp16 tri-plane texels of the ray-marcher and the point query)
    "ln3d_planes_to_channel_last_f16": _int(vp, vp, i32, i32, i32, i32, vp),
    "ln3d_planes_f32_to_f16": _int(vp, vp, i64, vp),
    "ln3d_render_triplane_f16": _int(_render, vp),
    "ln3d_query_points_f16": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, vp, vp, vp, vp),
    # include/ln3d_normals.h (sigma gradient at points, surface normals per ray)
    "ln3d_query_points_grad": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, vp, vp, vp),
    "ln3d_query_points_grad_f16": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, vp, vp, vp),
    "ln3d_surface_normals": _int(_normals, vp),
    "ln3d_surface_normals_f16": _int(_normals, vp),
    # include/ln3d_meshclean.h (connected components of the extracted mesh, floater removal)
    "ln3d_mesh_components": _int(vp, i64, i64, vp, vp),
    "ln3d_mesh_component_counts": _int(vp, i64, vp, i64, vp, vp, vp, vp),
    "ln3d_mesh_mark": _int(vp, i64, vp, vp, i64, i64, i32, vp, vp, vp, vp),
    "ln3d_mesh_gather": _int(vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp),
    # include/ln3d_meshsimplify.h (mesh simplification by vertex clustering)
    "ln3d_simplify_keys": _int(vp, i64, f32, f32, f32, f32, vp, vp),
    "ln3d_simplify_mean": _int(vp, vp, vp, i64, i64, vp, vp),
    "ln3d_simplify_faces": _int(vp, i64, vp, i64, i64, vp, vp, vp),
    "ln3d_simplify_first": _int(vp, vp, i64, vp, vp),
    "ln3d_simplify_used": _int(vp, vp, i64, i64, vp, vp),
    # include/ln3d_meshbake.h (texture baking of an exported mesh: per-face atlas)
    "ln3d_bake_points": _int(vp, i64, vp, i64, i32, i32, i32, vp, vp, vp),
    "ln3d_bake_pack": _int(vp, vp, i64, i32, vp, vp),
    # include/ln3d_meshpack.h (the records of a binary PLY and the buffer sections of a GLB, packed on the device)
    "ln3d_pack_ply_vertices": _int(vp, vp, vp, vp, i64, vp, vp),
    "ln3d_pack_ply_faces": _int(vp, i64, vp, vp),
    "ln3d_pack_gltf_vertices": _int(vp, vp, vp, vp, i64, vp, vp, vp, vp),
    "ln3d_pack_gltf_indices": _int(vp, i64, vp, vp),
    "ln3d_pack_gltf_corners": _int(vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp),
    "ln3d_position_bounds": _int(vp, i64, vp, vp),
    # include/ln3d_meshquadric.h (quadric-error placement of the simplification's representatives)
    "ln3d_quadric_pairs": _int(vp, i64, i64, vp, vp),
    "ln3d_quadric_place": _int(vp, i64, vp, i64, vp, i64, vp, i64, vp, f32, f32, f32, f32, vp, f32, vp, vp, vp),
    # include/ln3d_meshsmooth.h (Taubin smoothing of an exported mesh)
    "ln3d_smooth_edge_keys": _int(vp, i64, vp, vp),
    "ln3d_smooth_halfedges": _int(vp, vp, i64, i64, vp, vp, vp),
    "ln3d_smooth_step": _int(vp, vp, vp, vp, i64, i64, f32, vp, vp),
    # include/ln3d_meshsnap.h (Newton projection of points onto a level set of the density field)
    "ln3d_snap_points": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, f32, i32, f32, f32, f32, vp, vp, vp, vp, vp),
    "ln3d_snap_points_f16": _int(vp, i32, i32, vp, i64, vp, vp, vp, vp, f32, f32, i32, f32, f32, f32, vp, vp, vp, vp, vp),
}
SYMBOLS = list(PROTOTYPES)


_lib = None


def lib():
    """dlopen the HIP library; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python __graft_entry__.py`).  ln3diff_amd has no CPU/eager fallback.")
        # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  It must be in the process BEFORE this library is
        # loaded, so that our NEEDED libamdhip64.so.7 resolves to the same runtime; loaded the other way round (build() then
        # smoke() in one process) /opt/rocm's copy comes in first, torch then loads its own, and launches on torch's streams
        # fail with "HIP kernel launch failed".
        import torch  # noqa: F401
        _lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _lib


def check_symbols():
    L = lib()
    missing = [s for s in PROTOTYPES if not hasattr(L, s)]
    if missing:
        raise RuntimeError(f"libln3d_hip.so lacks symbols: {missing}")
    assert L.ln3d_abi_version() == ABI_VERSION
    return True


def check(code, what=""):
    if code != 0:
        raise RuntimeError(f"ln3d {what} failed: {lib().ln3d_strerror(code).decode()} ({code})")
