"""ctypes signatures of the C ABI exported by rocalphago_amd/_hipkernels.so: one row per
prototype in csrc/hip/rag_api.h (tests/test_native_symbols.py compares the two)."""
import ctypes as C

P = C.c_void_p
I = C.c_int
F = C.c_float
I64 = C.c_int64
SZ = C.c_size_t

SIGNATURES = {
    # conv.hip
    "rag_conv_igemm": [P] * 6 + [I] * 10 + [P, P, I, P, P, P, P],
    "rag_conv_wgrad_workspace": [I, I, I, I, I, P],
    "rag_conv_wgrad": [P] * 5 + [I] * 11 + [P, P, P],
    "rag_conv_bn_stat_blocks": [I, I, I],
    "rag_conv_bn_fusable": [I, I, I, I, I, I],
    "rag_wgrad_flush": [P, P],
    "rag_wgrad_pending_bytes": [],
    "rag_wgrad_pending_init": [P],
    "rag_wgrad_pending_free": [P],
    "rag_pack_weights": [P, P, P, I, I, I, I, I, P],
    "rag_pack_trunk": [P, I, I, I64, P, I64, F, F, I],
    # conv_wino.hip (+ the pending-handle entries in conv.hip)
    "rag_conv_wino_ok": [I, I, I, I, I],
    "rag_conv_wino": [P] * 5 + [I] * 8 + [P, P, I],
    "rag_wino_pack": [P, I, I, P, I64, F, F, I],
    "rag_pack_step": [P, I, P, I, I, I, I, P, I64, F, F, I, P, I64, I64, I64, I64],
    "rag_conv_wino_mode": [I, I, I, I],
    "rag_conv_wino_bn_ok": [I, I, I, I],
    "rag_conv_wino_bn": [P] * 6 + [I] * 8 + [P] * 6,
    "rag_conv_wino_bn_ch": [P] * 5 + [I] * 7 + [P] * 3,
    "rag_conv_wino_chain": [P, I, I, I, P, I],
    "rag_pack_input_u8": [P, P, P, P, I, I, I, I, I, I, P],
    "rag_pack_input_f32": [P, P, P, P, I, I, I, I, I, I, P],
    "rag_pack_input_bits": [P, P, P, P, I, I, I, I, I, P],
    "rag_unpack": [P, P, I, I, I, I, I, P],
    "rag_pack_nchw": [P, P, I, I, I, I, I, P],
    # head.hip
    "rag_policy_head_fwd": [P] * 16 + [I, I, I, I, I, F, P],
    "rag_policy_head_soft": [P] * 15 + [I, I, I, I, F, P],
    "rag_head_bwd": [P] * 8 + [I] * 5 + [P] * 5,
    "rag_head_bwd_workspace": [I, I, I],
    "rag_policy_head_dual": [P] * 15 + [I, I, I, I, I, F, P],
    "rag_head_bwd2": [P] * 12 + [I] * 5 + [P] * 5,
    "rag_head_bwd2_workspace": [I, I, I],
    "rag_policy_head_dual_relu": [P] * 15 + [I, I, I, I, I, F, P],
    "rag_head_bwd2_relu": [P] * 12 + [I] * 4 + [P] * 5,
    "rag_head_linear": [P, P, P, P, I, I, I, I, P],
    "rag_value_mlp_fwd": [P, P, P, P, P, P, P, P, I, I, I, I, P],
    "rag_value_mlp_workspace": [I, I],
    "rag_value_mlp_bwd": [P] * 16 + [I, I, I, I, P],
    "rag_sl_batch": [P, P, P, I, P, I, C.c_uint, C.c_uint, P, P, I, P],
    "rag_sl_batch_soft": [P, P, I, P, I, P, I, C.c_uint, C.c_uint, P, P, I, I, P],
    "rag_value_batch": [P, P, P, I, C.c_uint, C.c_uint, P, P, I, P],
    "rag_value_mlp_bwd_workspace": [I, I],
    # optim.hip
    "rag_sgd": [P, P, P, I64, F, F, F, I, P],
    # rollout.hip
    "rag_rollouts": [P, P, I, I, I, F, I, P, P, C.c_uint, P, P, P, P, P, I],
    "rag_rollout_park_bytes": [I],
    # bn.hip
    "rag_bn_workspace": [I, I],
    "rag_bn_train_fwd": [P, I, I, I, I, I, P, P, P, P, F, F, P, P, P, P],
    "rag_bn_infer_coef": [P, P, P, P, F, I, P, P],
    "rag_bn_bwd_coef": [P, I, P, I, I, I, I, I, P, P, P, P, P, P, P],
    "rag_bn_apply": [P, I, P, I, P, I, P, I, P, I, I, I, I, I, P],
    "rag_bn_apply_bwd_part": [P, I, P, P, P, P, P, I, P, I, P, I, P, I, I, I, I, I, P],
    "rag_bn_finalize_fwd": [P, I, I, I, I, P, P, P, P, F, F, P, P, P],
    "rag_bn_finalize_bwd": [P, I, I, I, I, P, P, P, P, P, P],
    "rag_bn_ch_finalize_fwd": [P, I, I, I, I, I, P, P, P, P, F, F, P, P, P],
    "rag_bn_ch_workspace": [I, I, I],
    "rag_bn_ch_train_fwd": [P, I, I, I, I, I, P, P, P, P, F, F, P, P, P, P],
    "rag_bn_ch_infer_coef": [P, P, P, P, F, I, I, P, P],
    "rag_bn_ch_bwd_coef": [P, I, P, I, I, I, I, I, P, P, P, P, P, P, P],
    "rag_bn_ch_apply": [P, I, P, I, P, I, P, I, P, I, I, I, I, I, P],
    # sample.hip
    "rag_sample_moves": [P, P, I, P, I, I, F, C.c_uint64, P, P, P],
    # features.hip
    "rag_pass_grads": [P, P, P, P, I, I, P],
    "rag_features": [P, P, P, P, P, I, I, P, I, I, P, P, P],
    # ladder.hip
    "rag_ladder_workspace": [I, I],
    "rag_ladders": [P, P, I, I, P, P, P],
    # conv_tap.hip, wgrad_slab.hip (A/B setters the tests drive)
    "rag_conv_tap_mode": [I],
    "rag_wgrad_slab_part_bf16": [I],
    "rag_wgrad_slab_map": [I],
    "rag_wgrad_slab_chunks": [I, I, I, I, P],
}

RESTYPES = {"rag_conv_wgrad_workspace": SZ, "rag_head_bwd_workspace": SZ,
            "rag_head_bwd2_workspace": SZ,
            "rag_ladder_workspace": SZ, "rag_wgrad_pending_bytes": SZ,
            "rag_value_mlp_workspace": SZ, "rag_value_mlp_bwd_workspace": SZ,
            "rag_rollout_park_bytes": C.c_long}


def declare(lib):
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError: the library lacks a listed symbol
        fn.argtypes = args
        fn.restype = RESTYPES.get(name, I)
