"""CPU: every symbol the C-ABI library exports names the test that holds it to a reference (compute entry points: an op-level comparison
with plain PyTorch; path-level, profiling, communicator and error entry points: the test that drives them).  An export added without an
entry here -- or an entry whose test was renamed away -- fails this file, so a new kernel cannot ship covered by model goldens alone."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_OPS = "tests/test_ops_gpu.py::"
_ABWD = "tests/test_attention_bwd_gpu.py::"
_LLAMA = "tests/test_llama_ops_gpu.py::"
_MEND = "tests/test_mend_train_ops_gpu.py::"
_TP = "tests/test_tp_neuron_ops_gpu.py::"
_PATH = "tests/test_path_abi_gpu.py::"
_PATH_LLAMA = "tests/test_path_abi_llama_gpu.py::"
_SEAM = "tests/test_ft_seam_gpu.py::"
_VAR = "tests/test_gemm_variants_gpu.py::"
_CABI = "tests/test_cabi_exports.py::"

COVERED_BY = {
    # ---- op level ----
    "devqa_gemm_bf16": _OPS + "test_gemm",
    "devqa_gemm_bf16_swiglu_supported": _OPS + "test_gemm_fused_swiglu",
    "devqa_gemm_bf16_splitk": "tests/test_splitk_gpu.py::test_splitk",
    "devqa_gemm_f32": _VAR + "test_gemm_f32_exact_and_splitk",
    "devqa_gemm_set_mode": _VAR + "test_gemm_variants",
    "devqa_gemm_grouped_supported": _SEAM + "test_grouped_tail_equals_the_per_edit_loop",
    "devqa_gemm_grouped_bf16": _SEAM + "test_grouped_tail_equals_the_per_edit_loop",
    "devqa_gemm_grouped_f32": _SEAM + "test_grouped_tail_equals_the_per_edit_loop",
    "devqa_gather_cols_grouped_f32": _SEAM + "test_grouped_tail_equals_the_per_edit_loop",
    "devqa_gather_cols_grouped_bf16": _SEAM + "test_grouped_tail_equals_the_per_edit_loop",
    "devqa_layernorm": _OPS + "test_layernorm_fwd_bwd",
    "devqa_layernorm_bwd_dx": _OPS + "test_layernorm_fwd_bwd",
    "devqa_layernorm_bwd_params": _OPS + "test_layernorm_param_grads_and_colsum",
    "devqa_colsum_f32": _OPS + "test_layernorm_param_grads_and_colsum",
    "devqa_attention": _OPS + "test_attention",
    "devqa_attention_f32": _OPS + "test_attention_f32",
    "devqa_attention_reload_env": _OPS + "test_attention",
    "devqa_attention_bwd": _ABWD + "test_head_dims",
    "devqa_attention_bwd_f32": _ABWD + "test_head_dims",
    "devqa_im2col_patches": _OPS + "test_patch_embed_and_assemble",
    "devqa_im2col_patches_f32": _OPS + "test_patch_embed_and_assemble",
    "devqa_vit_assemble": _OPS + "test_patch_embed_and_assemble",
    "devqa_embed_rows": _OPS + "test_embed_rows_and_gather",
    "devqa_embed_rows_f32": _OPS + "test_embed_rows_and_gather",
    "devqa_gather_rows": _OPS + "test_embed_rows_and_gather",
    "devqa_cast_f32_bf16": _OPS + "test_embed_rows_and_gather",
    "devqa_split_f32_bf16x2": _OPS + "test_split_f32_bf16x2",
    "devqa_act_cast": _MEND + "test_act_cast",
    "devqa_vocab_rows": _OPS + "test_vocab_rows",
    "devqa_vocab_rows_f32": _OPS + "test_vocab_rows",
    "devqa_ft_adamw_step": _OPS + "test_ft_adamw_step_matches_torch_adamw",
    "devqa_ft_adamw_step_fm": _OPS + "test_ft_adamw_step_matches_torch_adamw",
    "devqa_rows_matvec_f32": _OPS + "test_rows_matvec_delta_and_control",
    "devqa_delta_op": _OPS + "test_rows_matvec_delta_and_control",
    "devqa_ft_step_control": _OPS + "test_rows_matvec_delta_and_control",
    "devqa_active_columns": _OPS + "test_column_compaction",
    "devqa_gather_cols_f32": _OPS + "test_column_compaction",
    "devqa_gather_cols_bf16": _OPS + "test_column_compaction",
    "devqa_scatter_cols_add_f32": _OPS + "test_column_compaction",
    "devqa_row_inv_norm": _OPS + "test_cosine_topk_few_queries_one_launch",
    "devqa_cosine_topk_workspace": _OPS + "test_cosine_topk_exact_indices",
    "devqa_cosine_topk": _OPS + "test_cosine_topk_exact_indices",
    "devqa_cosine_topk_cached": _OPS + "test_cosine_topk_few_queries_one_launch",
    "devqa_gelu_f32": _OPS + "test_gelu_forward_and_backward",
    "devqa_gelu_bwd_f32": _OPS + "test_gelu_forward_and_backward",
    # ---- LLaMA row ops ----
    "devqa_rmsnorm": _LLAMA + "test_rmsnorm_fwd",
    "devqa_rmsnorm_bwd_dx": _LLAMA + "test_rmsnorm_bwd_dx",
    "devqa_rope_f32": _LLAMA + "test_rope_f32",
    "devqa_rope_bf16": _LLAMA + "test_rope_bf16",
    "devqa_swiglu_f32": _LLAMA + "test_swiglu_f32",
    "devqa_swiglu_bf16": _LLAMA + "test_swiglu_bf16",
    "devqa_swiglu_bwd_bf16": _LLAMA + "test_swiglu_bwd",
    "devqa_swiglu_bwd_f32": _LLAMA + "test_swiglu_bwd",
    # ---- MEND / LTE training row ops ----
    "devqa_relu_bwd": _MEND + "test_relu_bwd",
    "devqa_relu_bwd_f32": _MEND + "test_relu_bwd",
    "devqa_mend_normalize_concat": _MEND + "test_mend_normalize_concat",
    "devqa_mend_lrlinear_epilogue": _MEND + "test_mend_lrlinear_epilogue",
    "devqa_mend_lrlinear_bwd": _MEND + "test_mend_lrlinear_bwd",
    "devqa_logit_kl_rows": _MEND + "test_kl_rows_and_dlogits",
    "devqa_kl_dlogits": _MEND + "test_kl_rows_and_dlogits",
    "devqa_welford_rows": _MEND + "test_welford_rows",
    "devqa_sumsq_f32": _MEND + "test_sumsq",
    "devqa_adam_step": _MEND + "test_adam_step",
    # ---- T-Patcher neuron ops ----
    "devqa_tp_neuron_fwd": _TP + "test_tp_neuron_fwd_bwd",
    "devqa_tp_neuron_bwd": _TP + "test_tp_neuron_fwd_bwd",
    "devqa_tp_gated_neuron_fwd": _TP + "test_tp_neuron_fwd_bwd",
    "devqa_tp_gated_neuron_bwd": _TP + "test_tp_neuron_fwd_bwd",
    # ---- path level: the model context and the launch schedules behind it ----
    "devqa_ctx_create": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_ctx_destroy": _PATH + "test_path_level_error_behaviour",
    "devqa_ctx_set_weight": _PATH + "test_ctx_set_weight_repoints_one_entry",
    "devqa_ctx_bind_edit_target": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_vision_encode_workspace": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_vision_encode": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_prefix_workspace": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_prefix": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_prefix_rows_workspace": _SEAM + "test_kept_rows_equal_all_rows_on_the_tiny_models",
    "devqa_llm_prefix_rows": _SEAM + "test_kept_rows_equal_all_rows_on_the_tiny_models",
    "devqa_llm_layers_workspace": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_layers": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_layers_ex": _SEAM + "test_kept_rows_equal_all_rows_on_the_tiny_models",
    "devqa_llm_forward_workspace": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_llm_forward": _PATH + "test_llm_forward_short_form",
    "devqa_llm_forward_ex": _PATH_LLAMA + "test_llava_forward_through_path_level_calls_only",
    "devqa_llm_head_workspace": _PATH + "test_engine_over_the_context_equals_python_schedule",
    "devqa_llm_head": _PATH + "test_engine_over_the_context_equals_python_schedule",
    "devqa_ft_edit_workspace": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_ft_edit": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_apply_delta": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_restore": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_token_acc": _PATH + "test_one_cycle_through_path_level_calls_only",
    "devqa_mend_transform_workspace": _PATH + "test_mend_transform_and_apply_entry_points",
    "devqa_mend_transform": _PATH + "test_mend_transform_and_apply_entry_points",
    "devqa_mend_apply_workspace": _PATH + "test_mend_transform_and_apply_entry_points",
    "devqa_mend_apply": _PATH + "test_mend_transform_and_apply_entry_points",
    # ---- communicator, profiling, errors ----
    "devqa_comm_unique_id": _PATH + "test_gather_scores_single_rank",
    "devqa_comm_create": _PATH + "test_gather_scores_single_rank",
    "devqa_comm_destroy": _PATH + "test_gather_scores_single_rank",
    "devqa_gather_scores": _PATH + "test_gather_scores_single_rank",
    "devqa_profile": _OPS + "test_profile_slots_count_launches",
    "devqa_profile_read": _OPS + "test_profile_slots_count_launches",
    "devqa_profile_dropped": _OPS + "test_profile_slots_count_launches",
    "devqa_profile_gemm": _OPS + "test_profile_slots_count_launches",
    "devqa_profile_gemm_read": _OPS + "test_profile_slots_count_launches",
    "devqa_last_error": _CABI + "test_argument_validation_without_gpu",
    "devqa_abi_version": _CABI + "test_header_symbols_exported",
}


def test_every_export_names_its_test():
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    exports = set(lib.EXPORTS)
    assert len(exports) == len(lib.EXPORTS), "duplicate names in lib.EXPORTS"
    missing, stale = sorted(exports - set(COVERED_BY)), sorted(set(COVERED_BY) - exports)
    assert not missing, "exported without a test named in COVERED_BY: %s" % missing
    assert not stale, "COVERED_BY names symbols the library does not export: %s" % stale


def test_named_tests_exist():
    defined = {}
    for sym, where in sorted(COVERED_BY.items()):
        path, _, func = where.partition("::")
        assert path.startswith("tests/test_") and path.endswith(".py") and func.startswith("test_"), (sym, where)
        full = os.path.join(ROOT, *path.split("/"))
        assert os.path.isfile(full), "%s: no file %s" % (sym, path)
        if path not in defined:
            with open(full) as f:
                defined[path] = {n.name for n in ast.parse(f.read()).body if isinstance(n, ast.FunctionDef)}
        assert func in defined[path], "%s: %s defines no %s" % (sym, path, func)
