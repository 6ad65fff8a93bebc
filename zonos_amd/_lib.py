"""ctypes binding of libzonos_hip.so (the C ABI declared in include/zonos_hip.h).

The product path has no fallback: if the library is missing or fails to load, every
entry point raises. Device buffers are torch tensors; only their data_ptr() crosses the
ABI together with plain ints/floats and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C  # noqa: N812
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZK_LIB_PATH") or os.path.join(_HERE, "lib", "libzonos_hip.so")

P = C.c_void_p
I = C.c_int
L = C.c_long
F = C.c_float
U64 = C.c_uint64
I64 = C.c_int64


class SamplingParams(C.Structure):
    _fields_ = [("temperature", F), ("top_p", F), ("min_p", F), ("linear", F), ("conf", F), ("quad", F),
                ("top_k", C.c_int32), ("rp_window", C.c_int32), ("cfg_scale", F),
                ("force_full_length", C.c_int32)]


class GenState(C.Structure):
    _fields_ = [("scal", P), ("eos_mode", P), ("steps_after", P), ("remaining", P), ("stopping", P),
                ("act", P), ("rp", P), ("tok0", P), ("tok1", P), ("delayed", P),
                ("B", C.c_int32), ("K", C.c_int32), ("Ld", C.c_int32), ("V", C.c_int32),
                ("seed", U64), ("row_base", C.c_int32), ("noise_mode", C.c_int32), ("noise_offset", U64),
                ("noise_stride", C.c_int32), ("noise_incr", C.c_int32)]


class RowParams(C.Structure):
    """zk_row_params: one utterance of a request batch (its sampling parameters, keyed-noise seed and key)."""
    _fields_ = [("sp", SamplingParams), ("seed", U64), ("key", C.c_int32), ("reserved", C.c_int32)]


class StepLayer(C.Structure):
    _fields_ = [("ln1_w", P), ("ln1_b", P), ("wqkv", P), ("wo", P), ("ln2_w", P), ("ln2_b", P), ("fc1", P),
                ("fc2", P), ("k_cache", P), ("vt_cache", P), ("k_scale", P), ("v_scale", P),
                ("wqkv8", P), ("wo8", P), ("fc18", P), ("fc28", P), ("wqkv_scale", P), ("wo_scale", P),
                ("fc1_scale", P), ("fc2_scale", P)]


class StepDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "n_layer", "d_model", "n_heads", "n_kv", "head_dim", "d_ff", "smax",
                                         "split_qkv", "split_o", "split_fc2", "split_heads", "attn_splits",
                                         "attn_merge", "rope_neox", "small")] + \
              [("eps", F), ("kv_fp8", C.c_int32), ("layers", P), ("emb", P), ("heads", P), ("lnf_w", P), ("lnf_b", P),
               ("freqs", P), ("x", P), ("xn", P), ("y", P), ("h", P), ("part", P), ("attn_work", P), ("attn_cnt", P),
               ("dbg", P), ("st", GenState), ("sp", SamplingParams), ("pre_k", P), ("pre_vt", P),
               ("pre_smax", C.c_int32), ("w_fp8", C.c_int32), ("rows", P)]


class HybridLayer(C.Structure):
    _fields_ = [("type", C.c_int32), ("d_mlp", C.c_int32), ("ln1_w", P), ("ln1_b", P), ("wqkv", P), ("wo", P),
                ("ln2_w", P), ("ln2_b", P), ("fc1", P), ("fc2", P), ("k_cache", P), ("vt_cache", P), ("w_in", P),
                ("conv_w", P), ("conv_b", P), ("A", P), ("dt_bias", P), ("Dskip", P), ("norm_w", P), ("w_out", P),
                ("conv_state", P * 2), ("ssm_state", P * 2)]


class HybridDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "n_layer", "d_model", "n_heads", "n_kv", "head_dim", "d_ff", "smax",
                                         "d_inner", "nheads_ssm", "headdim_ssm", "d_state", "split_qkv", "split_o",
                                         "split_fc2", "split_heads", "split_inp", "split_out", "attn_splits",
                                         "norm_flags")] + \
              [("eps", F), ("gate_eps", F), ("layers", P), ("emb", P), ("heads", P), ("lnf_w", P), ("lnf_b", P),
               ("freqs", P), ("x", P), ("xn", P), ("y", P), ("h", P), ("part", P), ("attn_work", P), ("yz", P),
               ("ym", P), ("xc", P), ("dbg", P), ("st", GenState), ("sp", SamplingParams), ("xf", P), ("rows", P)]


class DacResUnit(C.Structure):
    _fields_ = [("dil", C.c_int32), ("a1", P), ("w1", P), ("b1", P), ("a2", P), ("w2", P), ("b2", P)]


DAC_MAXB, DAC_MAXR = 6, 3


class DacBlock(C.Structure):
    _fields_ = [("stride", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("nres", C.c_int32),
                ("alpha", P), ("wt", P), ("bt", P), ("res", DacResUnit * DAC_MAXR)]


class DacDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nblocks", "ncb", "codebook_size", "hidden", "cin0", "c0")] + \
              [("tables", P), ("conv1_w", P), ("conv1_b", P), ("final_alpha", P), ("conv2_w", P), ("conv2_b", P),
               ("blocks", DacBlock * DAC_MAXB)]


class StreamDesc(C.Structure):
    _fields_ = [("dac", C.POINTER(DacDesc)), ("delayed", P), ("B", C.c_int32), ("K", C.c_int32), ("Ld", C.c_int32),
                ("P", C.c_int32)]


class SpkBlock(C.Structure):
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("stride", C.c_int32), ("pad_", C.c_int32),
                ("w1", P), ("scale1", P), ("shift1", P), ("w2", P), ("scale2", P), ("shift2", P),
                ("wd", P), ("scaled", P), ("shiftd", P)]


class SpkDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "c0", "nblocks", "pool_dim", "att_dim", "emb_dim", "lda_dim",
                                         "pad_")] + \
              [(n, P) for n in ("window", "twiddle", "melfb", "stem_w", "stem_scale", "stem_shift", "blocks",
                                "asp_w1", "asp_b1", "asp_bn_scale", "asp_bn_shift", "asp_w2", "asp_b2",
                                "bott_w", "bott_b", "lda_w", "lda_b")]


# name -> argtypes (all return int status)
_SIGS = {
    "zk_version": [],
    "zk_device_sync": [],
    "zk_sample_logits": [P, I, I, I, P, I, I, P, C.POINTER(SamplingParams), U64, I, I, I, P, P],
    "zk_sample_logits_torch": [P, I, I, I, P, I, I, P, C.POINTER(SamplingParams), U64, U64, I, P, P],
    "zk_torch_exponential": [P, L, U64, U64, I, P],
    "zk_delay_apply": [P, I, I, I, I64, P, P],
    "zk_delay_revert": [P, I, I, I, P, P],
    "zk_embed_codes": [P, I, I, I, L, L, P, I, P, I, I, I, P, I, I, P, P, F, P, P, P],
    "zk_layernorm": [P, P, P, F, I, I, P, P],
    "zk_resid_ln": [P, I, P, P, P, F, I, I, P, P, I, P, P],
    "zk_gemm_bf16": [P, L, P, I, I, I, I, I, P, P, P, P],
    "zk_gemv_fused": [P, L, P, I, I, I, I, P, P, F, P, P, P, P],
    "zk_permute_fc1": [P, I, I, P, P],
    "zk_pack_weights": [P, I, I, P, P],
    "zk_pack_weights_e4m3": [P, I, I, P, P, P],
    "zk_gemv_fused_w8": [P, L, P, P, I, I, I, I, P, P, F, P, P, P, P],
    "zk_gemv_qkv_rope_w8": [P, P, P, I, I, I, I, P, P, F, P, P, P, I, P, P, P, P],
    "zk_gemv_attn_out_w8": [P, I, I, P, P, I, I, I, P, P, P],
    "zk_qkv_rope": [P, I, I, I, I, I, I, P, I, P, P, P, P, I, P, I, P, P],
    "zk_attn_decode": [P, P, P, I, I, I, I, I, I, P, P, I, P, P, P],
    "zk_attn_decode_qkv": [P, I, P, P, P, I, I, I, I, I, I, P, P, I, P, I, P, P],
    "zk_attn_decode_qkv_sc": [P, I, P, P, P, I, I, I, I, I, I, P, P, I, P, P, I, P, P],
    "zk_attn_decode_qkv_part": [P, I, P, P, P, I, I, I, I, I, I, P, P, I, I, P, P],
    "zk_attn_decode_qkv_sc_rows": [P, I, P, P, P, I, I, I, I, I, I, P, P, P, I, P, P, P, P],
    "zk_attn_decode_qkv_f8_rows": [P, I, P, P, P, P, P, I, I, I, I, I, I, P, P, P, I, P, P, P, P],
    "zk_embed_codes_rows": [P, I, I, I, L, L, P, I, I, I, P, I, I, P, P],
    "zk_gather_last_rows": [P, I, I, I, P, P, P],
    "zk_kv_quantize_e4m3": [P, P, I, I, I, I, I, P, P, P, P, I, P],
    "zk_attn_decode_f8": [P, P, P, P, P, I, I, I, I, I, I, P, P, I, P, P, P],
    "zk_attn_decode_qkv_f8": [P, I, P, P, P, P, P, I, I, I, I, I, I, P, P, I, P, P, P, P],
    "zk_gemv_attn_out": [P, I, I, P, I, I, I, P, P, P],
    "zk_gemv_qkv_rope": [P, P, I, I, I, I, P, P, F, P, P, P, I, P, P, P, P],
    "zk_attn_decode_q_part": [P, P, P, I, I, I, I, I, I, P, P, I, P, P],
    "zk_decode_step": [C.POINTER(StepDesc), P],
    "zk_decode_step_rows": [C.POINTER(StepDesc), P, P],
    "zk_prefill": [C.POINTER(StepDesc), P, I, I, P, P],
    "zk_prefill_rows": [C.POINTER(StepDesc), P, I, I, P, P, P],
    "zk_hybrid_decode_step": [C.POINTER(HybridDesc), P],
    "zk_hybrid_prefill": [C.POINTER(HybridDesc), P, I, I, P, P],
    "zk_dac_decode": [C.POINTER(DacDesc), P, I, I, P, P, C.c_size_t, P, P],
    "zk_stream_window": [P, I, I, I, I, I, I, I, P, P, P, P],
    "zk_stream_crop": [P, I, I, I, I, I, I, P, P, P, P],
    "zk_stream_chunk": [C.POINTER(StreamDesc), I, I, I, I, I, P, C.c_size_t, P, P, P, P],
    "zk_mamba_step": [P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "zk_mamba_step_per_head": [P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "zk_mamba_prefill": [P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P],
    "zk_gated_rmsnorm": [P, I, I, P, F, P, P, P],
    "zk_attn_prefill": [P, P, P, I, I, I, I, I, I, P, P],
    "zk_sample_heads": [P, I, C.POINTER(GenState), C.POINTER(SamplingParams), I, I, P, P],
    "zk_eos_step": [C.POINTER(GenState), I, I, P],
    "zk_sample_heads_rows": [P, I, C.POINTER(GenState), P, I, I, P, P],
    "zk_eos_step_rows": [C.POINTER(GenState), I, I, P],
    "zk_graph_begin": [P],
    "zk_graph_end": [P, C.POINTER(P)],
    "zk_graph_launch": [P, I, P],
    "zk_graph_destroy": [P],
    "zk_event_create": [C.POINTER(P)],
    "zk_event_record": [P, P],
    "zk_event_elapsed_ms": [P, P, C.POINTER(F)],
    "zk_event_destroy": [P],
    "zk_dac_rvq_tables": [P, P, P, I, I, I, I, P, P],
    "zk_dac_rvq_decode": [P, I, I, I, L, P, I, I, P, I, P, P],
    "zk_dac_conv": [P, I, I, I, P, P, P, I, I, I, I, I, I, I, P, I, P, I, P, I, I, P],
    "zk_dac_prep_convt": [P, I, I, I, P, P],
    "zk_dac_prep_w16": [P, I, I, I, I, I, P, P, P],
    "zk_dac_conv16": [P, I, I, I, P, P, P, P, I, I, I, I, I, I, I, P, I, P, I, P, I, I, I, P],
    "zk_dac_tail": [P, I, I, I, P, P, P, P, P, I, P],
    "zk_dac_rvq_decode_cl": [P, I, I, I, L, P, I, I, I, P, P, P],
    "zk_dac_conv_cl": [P, I, I, I, P, L, P, I, I, I, I, I, I, I, I, I, P, P, P, P, I, P, I, I, P],
    "zk_dac_conv_plan": [I, I, I, I, I, I, I, I, I, I, P],
    "zk_gemm_plan": [I, I, I, I, I, P],
    "zk_gemv_plan": [I, I, I, I, I, P],
    "zk_dac_tail_cl": [P, I, I, I, P, P, P, P, I, P],
    "zk_dac_resunit_cl": [P, I, I, I, P, P, I, P, P, P, P, P, P, I, P, I, P],
    "zk_dac_enc_conv1": [P, I, I, P, P, P, I, I, P, P, P],
    "zk_dac_rvq_encode": [P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P],
    "zk_resample": [P, I, L, P, I, I, I, I, P, L, P],
    "zk_prefix_cond": [P, I, P, P],
    "zk_loudness_gains": [P, I, L, P, I, C.c_double, P, P, P, P],
    "zk_spk_logfbank": [P, I, I, P, P, P, I, P, P],
    "zk_spk_stem": [P, I, I, I, P, P, P, I, P, P, P],
    "zk_spk_conv2d_cl": [P, I, I, I, I, P, I, I, I, P, P, I, P, P, P, P],
    "zk_spk_simam": [P, I, I, I, I, P, P, P, P, P, P],
    "zk_spk_asp": [P, I, I, I, I, P, P, P, P, P, P, I, P, P, P],
    "zk_spk_head": [P, I, I, P, P, I, P, P, I, P, P, P],
    "zk_speaker_embed": [C.POINTER(SpkDesc), P, I, I, P, C.c_size_t, P, P, P],
}

_lib = None


class ZonosHipError(RuntimeError):
    pass


def load():
    """Load (and type) the library. Raises ZonosHipError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZonosHipError(f"{LIB_PATH} not found: build it with `python -m zonos_amd.build` "
                            "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.zk_last_error.restype = C.c_char_p
    lib.zk_last_error.argtypes = []
    lib.zk_loudness_max_blocks.restype = C.c_int
    lib.zk_loudness_max_blocks.argtypes = [L, I]
    lib.zk_abi_size.restype = C.c_long
    lib.zk_abi_size.argtypes = [I]
    lib.zk_dac_decode_workspace.restype = C.c_size_t
    lib.zk_dac_decode_workspace.argtypes = [C.POINTER(DacDesc), I, I]
    lib.zk_stream_workspace.restype = C.c_size_t
    lib.zk_stream_workspace.argtypes = [C.POINTER(StreamDesc), I]
    lib.zk_dac_resunit_supported.restype = C.c_int
    lib.zk_dac_resunit_supported.argtypes = [I]
    lib.zk_gemm_warm_tiles.restype = C.c_int
    lib.zk_gemm_warm_tiles.argtypes = [I, I, I, I, I, I]
    lib.zk_torch_noise_policy.restype = C.c_int
    lib.zk_torch_noise_policy.argtypes = [L, I, I, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    lib.zk_spk_conv_tiles.restype = C.c_int
    lib.zk_spk_conv_tiles.argtypes = [I, I]
    lib.zk_speaker_workspace_bytes.restype = C.c_size_t
    lib.zk_speaker_workspace_bytes.argtypes = [C.POINTER(SpkDesc), I, I]
    _lib = lib
    return lib


def exported_symbols() -> list[str]:
    return list(_SIGS) + ["zk_last_error", "zk_loudness_max_blocks", "zk_abi_size",
                          "zk_dac_decode_workspace", "zk_stream_workspace", "zk_dac_resunit_supported", "zk_gemm_warm_tiles",
                          "zk_torch_noise_policy", "zk_spk_conv_tiles", "zk_speaker_workspace_bytes"]


def call(name: str, *args):
    lib = load()
    if len(args) != len(_SIGS[name]):
        raise TypeError(f"{name}: {len(args)} arguments given, the C ABI takes {len(_SIGS[name])}")
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise ZonosHipError(f"{name} failed ({rc}): {lib.zk_last_error().decode()}")
    return rc


DAC_PLAN_FIELDS = ("shape", "fm", "tile", "dx", "nx", "lds", "nq", "tiles", "wg_per_cu")   # ZK_DAC_PLAN_N = 9


def dac_conv_plan(B, Cin, Cout, ks, dil, Qn, nphase=1, resid=False, s_f32=False, fused=False) -> dict:
    """zk_dac_conv_plan: how zk_dac_conv_cl (fused: zk_dac_resunit_cl, C = Cout, T = Qn) launches a shape. No GPU."""
    plan = (C.c_int32 * len(DAC_PLAN_FIELDS))()
    call("zk_dac_conv_plan", int(fused), B, Cin, Cout, ks, dil, Qn, nphase, int(resid), int(s_f32), plan)
    return dict(zip(DAC_PLAN_FIELDS, plan))


GEMM_FAMILIES = ("rk", "ws", "pf", "tile")       # k_gemv_rk, k_gemm_ws, k_gemm_pf, k_gemm
GEMM_PLAN_FIELDS = ("family", "ks", "pf", "nchunks", "mt", "ncw", "u", "ntw", "gx", "gy", "gz", "block", "lds",
                    "pf_cols")                   # ZK_GEMM_PLAN_N = 14
GEMV_PLAN_FIELDS = ("lay", "ksw", "xr", "grid", "block", "ntw", "half", "nw", "ks", "pf")   # ZK_GEMV_PLAN_N = 10


def gemm_plan(M, N, K, nsplit=1, mode=0) -> dict:
    """zk_gemm_plan: the kernel family (a name of GEMM_FAMILIES), its template selectors and the grid
    zk_gemm_bf16 launches a shape with. No GPU."""
    plan = (C.c_int32 * len(GEMM_PLAN_FIELDS))()
    call("zk_gemm_plan", M, N, K, nsplit, mode, plan)
    d = dict(zip(GEMM_PLAN_FIELDS, plan))
    d["family"] = GEMM_FAMILIES[d["family"]]
    return d


def gemv_plan(M, N, K, mode=0, ln=False) -> dict:
    """zk_gemv_plan: the layout, template selectors and grid zk_gemv_fused launches a shape with. No GPU."""
    plan = (C.c_int32 * len(GEMV_PLAN_FIELDS))()
    call("zk_gemv_plan", M, N, K, mode, int(ln), plan)
    return dict(zip(GEMV_PLAN_FIELDS, plan))


def ptr(t) -> int | None:
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def device_index(device) -> int:
    """The GPU index a (possibly unindexed) cuda device means: torch.device("cuda") is the current
    device (torch.cuda.set_device), not GPU 0 -- the index of the generator torch itself would use."""
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def require_gpu(t: torch.Tensor, name: str = "tensor"):
    if not t.is_cuda:
        raise ZonosHipError(f"{name} must be a GPU tensor (the HIP engine has no CPU path)")
