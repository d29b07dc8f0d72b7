"""ctypes loader for libvt355.so (the C-ABI declared in include/vt355.h).

The product path has NO fallback: if the HIP library is missing or a call fails, we raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class VtError(RuntimeError):
    pass


def lib_path() -> str:
    # VT355_LIB: an alternative build of the same ABI (compiler-flag experiments, tools/); default = the in-tree library
    return os.environ.get("VT355_LIB") or os.path.join(_HERE, "libvt355.so")


# name -> argtypes ; all return int unless listed in _RESTYPE
_vp, _i, _ll, _f, _fp = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_void_p
PROTOTYPES = {
    "vt_version": [],
    "vt_arch": [],
    "vt_error_string": [_i],
    "vt_gemm_bf16": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _i, _fp, _fp, _i, _i, _i,
                     _vp, _i, _vp, _i, _vp],
    "vt_gemm_set_tile": [_i],
    "vt_gemm_set_big_loop": [_i],
    "vt_gemm_big_last_wide": [],
    "vt_gemm_bf16_kernel": [_i, _i, _i],
    "vt_gemm_bf16_tile": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _i, _fp, _fp, _i, _i, _i,
                          _vp, _i, _vp, _i, _i, _vp],
    "vt_gemm_bf16_block_tile": [_i, _i, _i],
    "vt_conv_set_tile": [_i],
    "vt_conv_set_slots": [_i],
    "vt_conv_plan": [_ll, _ll] + [_i] * 13 + [C.POINTER(C.c_int)] * 4,
    "vt_conv_dw_plan": [_ll, _ll] + [_i] * 13 + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_longlong)],
    "vt_transpose_bf16": [_vp, _ll, _ll, _vp, _ll, _ll, _i, _i, _i, _vp],
    "vt_transpose_multi_bf16": [_vp, _i, _ll, _vp],
    "vt_gemm_nt_bf16": [_vp, _i, _vp, _i, _fp, _i, _i, _i, _i, _f, _i, _vp],
    "vt_gemm_nt_bf16_unpad": [_vp, _i, _vp, _i, _fp, _i, _i, _i, _i, _f, _i, _i, _i, _i, _i, _vp],
    "vt_group_colsum": [_vp, _i, _vp, _i, _fp, _fp, _fp, _fp, _ll, _i, _i, _i, _i, _ll, _ll, _vp],
    "vt_qk_ln_param_grads": [_fp, _i, _vp, _i, _vp, _i, _fp, _fp, _fp, _ll, _i, _fp, _fp, _i, _i, _vp],
    "vt_ln_param_combine": [_fp, _fp, _i, _i, _vp, _vp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _vp],
    "vt_small_linear_bwd": [_fp, _i, _vp, _i, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _vp],
    "vt_silu_bwd": [_fp, _vp, _fp, _ll, _vp],
    "vt_attn_fwd_hd64": [_vp, _vp, _vp, _vp, _fp, _i, _i, _i, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _f, _i, _vp],
    "vt_attn_fwd_bias_hd64": [_vp, _vp, _vp, _fp, _vp, _fp, _i, _i, _i, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _f, _vp],
    "vt_gemm_splitk_f32": [_vp, _i, _vp, _i, _fp, _i, _i, _i, _i, _i, _vp],
    "vt_residual_cast_bf16": [_fp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _vp],
    "vt_groupnorm_ws_bytes": [_i, _i],
    "vt_groupnorm_silu_cl": [_vp, _ll, _vp, _vp, _vp, _ll, _i, _ll, _i, _i, _f, _i, _fp, _ll, _vp],
    "vt_causal_conv3d_cl": [_vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp],
    "vt_causal_conv3d_in8_cl": [_vp, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _vp],
    "vt_downsample_conv2d_cl": [_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp],
    "vt_downsample_conv2d_res_cl": [_vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp],
    "vt_conv3d_set_kernel": [_i, _i],
    "vt_conv3d_plan": [_ll] + [_i] * 8 + [C.POINTER(C.c_int)] * 4,
    "vt_temporal_pool_cl": [_vp, _ll, _vp, _ll, _i, _i, _ll, _i, _i, _vp],
    "vt_spatialnorm_silu_cl": [_vp, _ll, _vp, _vp, _vp, _vp, _ll] + [_i] * 9 + [_f, _i, _fp, _ll, _vp],
    "vt_upsample_conv2d_cl": [_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp],
    "vt_rmsnorm_bf16": [_vp, _ll, _vp, _vp, _ll, _ll, _i, _f, _vp],
    "vt_gated_gelu_bf16": [_vp, _ll, _vp, _ll, _ll, _i, _vp],
    "vt_attn_bwd_hd64": [_vp, _vp, _vp, _vp, _vp, _fp, _fp, _fp, _vp, _vp, _i, _i, _i,
                         _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _ll, _f, _i, _vp, _ll, _vp],
    "vt_attn_bwd_chain_ws_bytes": [_i, _i, _i],
    "vt_attn_bwd_set_chain": [_i, _i],
    "vt_attn_bwd_chain_plan": [_i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "vt_ln_modulate_fwd": [_vp, _i, _vp, _i, _vp, _vp, _fp, _fp, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _f, _vp],
    "vt_ln_modulate_bwd": [_vp, _i, _vp, _i, _fp, _fp, _vp, _fp, _fp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp],
    "vt_qk_layernorm_fwd": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _fp, _fp, _ll, _i, _f, _f, _fp, _fp, _i, _i, _vp],
    "vt_qk_layernorm_bwd": [_fp, _i, _vp, _i, _vp, _i, _fp, _fp, _vp, _vp, _vp, _i, _ll, _i, _fp, _fp, _i, _i, _vp],
    "vt_gate_mul": [_vp, _i, _vp, _i, _fp, _fp, _i, _ll, _i, _i, _i, _vp],
    "vt_silu_bf16": [_vp, _vp, _ll, _vp],
    "vt_cast_f32_bf16": [_fp, _vp, _ll, _vp],
    "vt_timestep_embedding": [_vp, _vp, _i, _i, _i, _f, _vp],
    "vt_patchify": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "vt_unpatchify": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "vt_add_noise": [_fp, _fp, _fp, _fp, _vp, _ll, _i, _vp],
    # sampler (csrc/sampler.hip): Philox normals under the header's noise convention; guidance combine + one DPM-Solver++ step
    "vt_philox_normal": [_vp, _i, _ll, _i, C.c_ulonglong, _i, _vp],
    "vt_dpm_step": [_vp, _vp, _fp, _fp, _vp, _fp, _ll, _i, _i] + [_f] * 8 + [_i, C.c_ulonglong, _i, _vp],
    "vt_diffusion_loss": [_vp, _vp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _ll, _i, _f, _vp],
    "vt_diffusion_loss_bwd": [_vp, _vp, _fp, _fp, _fp, _fp, _fp, _vp, _ll, _i, _vp],
    "vt_adamw": [_fp, _fp, _fp, _fp, _vp, _ll, _f, _f, _f, _f, _f, _i, _f, _vp, _vp],
    "vt_grad_sqnorm_partials": [],
    "vt_grad_sqnorm": [_fp, _ll, _fp, _i, _vp],
    "vt_clip_finalize": [_fp, _i, _f, _f, _fp, _vp],
    "vt_adamw_clip": [_fp, _fp, _fp, _fp, _vp, _ll, _f, _f, _f, _f, _f, _i, _f, _vp, _fp, _f, _vp],
    "vt_lora_down": [_vp, _i, _vp, _i, _i, _vp, _i, _ll, _i, _i, _vp],
    "vt_skinny_tn": [_vp, _i, _vp, _i, _i, _fp, _ll, _ll, _f, _ll, _i, _fp, _vp],
    "vt_skinny_tn_workspace_bytes": [_i],
    "vt_lora_up_add": [_vp, _i, _vp, _i, _vp, _i, _i, _ll, _i, _vp],
    "vt_lora_pack_b": [_fp, _vp, _i, _i, _i, _i, _f, _vp],
    "vt_lora_pack_bt": [_fp, _vp, _i, _i, _i, _i, _f, _vp],
    "vt_lora_down_wide": [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _i, _ll, _i, _vp],
    "vt_lora_tn_wide": [_vp, _i, _vp, _i, _i, _fp, _ll, _ll, _f, _ll, _i, _vp],
    "vt_lora_up_add_wide": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _ll, _i, _vp],
    "vt_lora_pack_b_wide": [_fp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "vt_lora_pack_bt_wide": [_fp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    # lora_dropout > 0: the same products under recomputed Philox keep masks (p, seed, site0 after the sibling's arguments)
    "vt_lora_down_drop": [_vp, _i, _vp, _i, _i, _i, _vp, _i, _ll, _i, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_skinny_tn_drop": [_vp, _i, _vp, _i, _i, _i, _fp, _ll, _ll, _f, _ll, _i, _fp, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_up_add_drop": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_down_wide_drop_fits": [_i, _i],
    "vt_lora_down_wide_drop": [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _i, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_tn_wide_drop": [_vp, _i, _vp, _i, _i, _fp, _ll, _ll, _f, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_up_add_wide_drop": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_up_add_dgelu_drop": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    "vt_lora_up_add_wide_dgelu_drop": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _ll, _i, _f, C.c_ulonglong, _i, _vp],
    # _at: the wide _drop products with an origin map (seg_local, seg_global, n_first, off_first, off_rest, k0, K_log) before the stream
    "vt_lora_down_wide_drop_at": [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _i, _ll, _i, _f, C.c_ulonglong, _i] + [_ll] * 5 + [_i, _i, _vp],
    "vt_lora_tn_wide_drop_at": [_vp, _i, _vp, _i, _i, _fp, _ll, _ll, _f, _ll, _i, _f, C.c_ulonglong, _i] + [_ll] * 5 + [_i, _i, _vp],
    "vt_lora_up_add_wide_drop_at": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _ll, _i, _f, C.c_ulonglong, _i] + [_ll] * 5 + [_i, _i, _vp],
    "vt_lora_up_add_wide_dgelu_drop_at": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _ll, _i, _f, C.c_ulonglong, _i] + [_ll] * 5
                                         + [_i, _i, _vp],
    # DoRA (use_dora): row norms / c = m / norm, the scaled operand refresh, the dB and dm finishes (csrc/dora.hip)
    "vt_dora_norm": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _f, _fp, _fp, _vp],
    "vt_dora_scale": [_vp, _ll, _vp, _ll, _fp, _i, _i, _i, _vp],
    "vt_dora_transpose_scale": [_vp, _ll, _vp, _ll, _fp, _i, _i, _vp],
    "vt_dora_db_add": [_fp, _fp, _fp, _i, _i, _vp],
    "vt_dora_dm": [_fp, _fp, _vp, _fp, _fp, _i, _vp],
    # ---- VideoCrafter2 UNet path ----
    "vt_conv_cl": [_vp, _ll, _vp, _vp, _fp, _i, _vp, _ll, _vp, _ll] + [_i] * 13 + [_vp],
    "vt_conv_dw_cl": [_vp, _ll, _vp, _ll, _fp] + [_i] * 13 + [_i, _vp],
    "vt_conv_dw_bias_cl": [_vp, _ll, _vp, _ll, _fp, _fp] + [_i] * 13 + [_i, _vp],
    "vt_conv_desc_extents": [_ll, _ll] + [_i] * 11 + [C.POINTER(C.c_longlong)] * 3,
    "vt_groupnorm_silu_bwd_cl": [_vp, _ll, _vp, _ll, _vp, _fp, _fp, _ll, _vp, _ll, _fp, _fp, _i, _ll, _i, _i, _i, _i, _vp],
    "vt_geglu_fwd": [_vp, _ll, _vp, _ll, _ll, _i, _vp],
    "vt_geglu_bwd": [_vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _vp],
    "vt_add_rows_bf16": [_vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _vp],
    "vt_dropout_bf16": [_vp, _ll, _vp, _ll, _ll, _i, _f, C.c_ulonglong, C.c_ulonglong, _vp, _vp],
    "vt_row_map_bf16": [_vp, _ll, _vp, _ll, _i, _ll, _i, _i, _i, _i, _vp],
    "vt_q_sample": [_fp, _fp, _fp, _fp, _fp, _vp, _ll, _i, _vp],
    "vt_mse_loss": [_vp, _fp, _fp, _vp, _ll, _f, _vp],
    "vt_attn_small_fwd": [_vp, _vp, _vp, _vp, _fp, _i, _i, _i, _i] + [_ll] * 8 + [_f, _i, _vp],
    "vt_qk_rmsnorm_rope128_fwd": [_vp, _ll, _vp, _ll, _vp, _vp, _fp, _fp, _fp, _ll, _i, _i, _i, _i, _i, _f, _vp],
    "vt_qk_rmsnorm_rope128_bwd": [_vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _fp, _fp, _fp, _fp, _fp, _ll, _i, _i, _i, _i, _i, _vp],
    "vt_attn128_fwd": [_vp, _vp, _vp, _vp, _fp, _vp, _i, _i, _i] + [_ll] * 8 + [_f, _vp],
    "vt_attn128_bwd": [_vp, _vp, _vp, _vp, _vp, _fp, _vp, _fp, _fp, _vp, _vp, _vp, _i, _i, _i] + [_ll] * 18 + [_f, _vp],
    "vt_gemm_fp8": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _fp, _fp, _vp],
    "vt_quantize_fp8": [_vp, _ll, _vp, _ll, _ll, _i, _fp, _vp, _i, _vp],
    "vt_gemm_mxfp8": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _fp, _fp, _i, _vp, _i, _fp, _fp, _i, _i, _i, _vp, _i,
                      _vp, _i, _vp, _i, _i, _vp, _i, _fp, _vp, _vp],
    "vt_cast_fp8_scaled": [_vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _i, _i, _i, _fp, _vp, _vp],
    "vt_ln_modulate_fwd_fp8": [_vp, _i, _vp, _i, _vp, _vp, _fp, _fp, _fp, _fp, _i, _fp, _fp, _i, _i, _i, _i, _f, _vp, _i, _fp, _vp, _vp],
    "vt_fp8_scale_update": [_vp, _fp, _fp, _i, _i, _vp],
    "vt_gemm_mxfp8_dx": [_vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _fp, _fp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i,
                         _vp, _i, _i, _fp, _vp, _vp],
    "vt_cast_fp8_fmt": [_vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _i, _i, _i, _i, _fp, _vp, _vp],
    "vt_gate_mul_fp8": [_vp, _i, _vp, _i, _fp, _fp, _i, _ll, _i, _i, _i, _vp, _i, _i, _fp, _vp, _vp],
    "vt_fp8_scale_update_fmax": [_vp, _fp, _fp, _i, _i, _f, _vp],
    "vt_opensora_loss": [_fp, _fp, _fp, _vp, _vp, _fp, _ll, _i, _i, _f, _vp],
    "vt_attn_gen_fwd": [_vp, _vp, _vp, _vp, _fp, _vp, _i, _i, _i, _i, _i, _i] + [_ll] * 8 + [_f, _i, _vp],
    "vt_attn_gen_bwd": [_vp, _vp, _vp, _vp, _vp, _fp, _vp, _vp, _vp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _i] + [_ll] * 14 + [_f, _i, _vp],
    "vt_attn_small_bwd": [_vp, _vp, _vp, _vp, _vp, _fp, _vp, _vp, _vp, _fp, _fp, _i, _i, _i, _i] + [_ll] * 14 + [_f, _i, _vp],
    # ---- DynamiCrafter: dual-context (text + per-frame image) cross-attention ----
    "vt_attn_dual_ws_floats": [_i] * 6,
    "vt_attn_dual_fwd": [_vp] * 6 + [_fp] + [_i] * 6 + [_ll] * 12 + [_f, _f, _vp],
    "vt_attn_dual_bwd": [_vp] * 6 + [_fp, _vp] + [_fp] * 5 + [_ll] + [_i] * 6 + [_ll] * 14 + [_f, _f, _vp],
    # ---- VideoCrafter1: temporal attention with relative-position tables ----
    "vt_attn_relpos_workspace_bytes": [],
    "vt_attn_relpos_fwd": [_vp] * 6 + [_fp] + [_i] * 4 + [_ll] * 4 + [_f, _vp],
    "vt_attn_relpos_bwd": [_vp] * 7 + [_fp] + [_vp] * 3 + [_fp, _fp, _vp] + [_i] * 4 + [_ll] * 8 + [_f, _vp],
}
_RESTYPE = {"vt_arch": C.c_char_p, "vt_error_string": C.c_char_p, "vt_skinny_tn_workspace_bytes": C.c_longlong,
             "vt_attn_bwd_chain_ws_bytes": C.c_longlong, "vt_groupnorm_ws_bytes": C.c_longlong,
             "vt_attn_dual_ws_floats": C.c_longlong, "vt_attn_relpos_workspace_bytes": C.c_longlong}


def load_library():
    """Load libvt355.so once; raise VtError (never fall back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch-ROCm ships its own libamdhip64; it must be the HIP runtime of this process BEFORE libvt355.so is mapped,
    # otherwise the kernels register with a second runtime and every launch on a torch stream fails.
    import torch  # noqa: F401
    path = lib_path()
    if not os.path.exists(path):
        raise VtError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(videotuna-dev_amd/csrc/build.sh). There is no CPU / eager fallback.")
    lib = C.CDLL(path)
    for name, args in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError here means header and library disagree
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, C.c_int)
    _LIB = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        lib = load_library()
        raise VtError(f"{what} failed: {lib.vt_error_string(code).decode()} (code {code})")
