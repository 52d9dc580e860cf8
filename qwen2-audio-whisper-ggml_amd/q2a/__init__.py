"""Python host mirror of the MI355X encoder path (ctypes over the C ABI in include/q2a_encoder.h).

The product is lib/libq2a.so (HIP kernels for gfx950). This module only marshals arguments; there is no
CPU fallback: if the library or a GPU is missing every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("Q2A_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libq2a.so")   # override: A/B builds
HOST_LIB_PATH = os.path.join(PKG_DIR, "lib", "libq2a_host.so")
TOOL_PATH = os.path.join(PKG_DIR, "bin", "q2a_tool")

EXPORTS = (
    "q2a_last_error", "q2a_open", "q2a_pack_model", "q2a_free_host_blob", "q2a_open_device_blob", "q2a_close",
    "q2a_get_info", "q2a_reserve", "q2a_encode_device", "q2a_encode_host", "q2a_pcm_to_mel",
    "q2a_encode_host_ex", "q2a_test_linear", "q2a_test_block", "q2a_test_block_taps", "q2a_test_attention", "q2a_test_fc1_path",
    "q2a_test_frontend", "q2a_test_pool_ln",
    "q2a_projector_open", "q2a_projector_close", "q2a_projector_get_dims", "q2a_projector_apply",
    "q2a_pack_model_compact", "q2a_blob_device_size", "q2a_expand_blob",
    "q2a_device_count", "q2a_group_open", "q2a_group_close", "q2a_group_size", "q2a_group_engine", "q2a_group_split",
    "q2a_group_encode_host", "q2a_group_setup_times", "q2a_group_open_with", "q2a_whisper_context_engine",
    "q2a_valid_lengths", "q2a_encode_device_padded", "q2a_encode_host_padded", "q2a_test_attention_len",
    "q2a_test_block_len",
    "q2a_varlen_rows", "q2a_encode_device_varlen", "q2a_encode_host_varlen", "q2a_test_attention_varlen",
    "q2a_test_block_varlen", "q2a_test_operand", "q2a_test_gemm_epi", "q2a_test_gemm_regime",
    "q2a_mel_valid_lengths", "q2a_encode_device_mel", "q2a_encode_host_mel", "q2a_test_frontend_mel",
    "whisper_set_mel", "whisper_set_mel_with_state",
    "q2a_packed_out_rows", "q2a_audio_features_device", "q2a_audio_features_device_mel", "q2a_audio_features_host",
    "q2a_audio_features_host_mel", "q2a_test_pool_operand",
    "q2a_feat_rows", "q2a_projector_apply_to", "q2a_projector_regime", "q2a_audio_features_device_to",
    "q2a_audio_features_device_mel_to",
    "q2a_audio_token_rows", "q2a_projector_apply_ids", "q2a_inputs_embeds_device", "q2a_inputs_embeds_device_mel",
    "q2a_test_audio_token_rows", "q2a_test_embed_gather",
)

# per-clip status of the encode calls (include/q2a_encoder.h): FAILED = the host call returned an error before this
# clip's output reached the caller
CLIP_ENCODED, CLIP_SKIPPED, CLIP_FAILED = 0, 1, 2


class Q2AError(RuntimeError):
    pass


class Info(C.Structure):
    _fields_ = [("n_audio_ctx", C.c_int32), ("n_audio_state", C.c_int32), ("n_audio_head", C.c_int32),
                ("n_audio_layer", C.c_int32), ("n_mels", C.c_int32), ("wtype", C.c_int32), ("n_out", C.c_int32),
                ("device", C.c_int32), ("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64),
                ("act", C.c_int32), ("reserved", C.c_int32)]


# producers of q2a_test_operand (include/q2a_encoder.h)
OPERAND_LN, OPERAND_QUANT_F32, OPERAND_QUANT_H16, OPERAND_GELU_Q8K = 0, 1, 2, 3

# epilogues of q2a_test_gemm_epi and the launcher's tile regimes (include/q2a_encoder.h)
EPI_QKV, EPI_RESID, EPI_GELU_H, EPI_GELU_Q8K, EPI_PRE_H = 0, 1, 2, 6, 7
(REGIME_NARROW, REGIME_128, REGIME_128x256, REGIME_256, REGIME_PIPE8, REGIME_PIPE8_PERSISTENT, REGIME_PIPE8_TAIL,
 REGIME_FIXED) = range(8)

# kinds of the log-mel entry points (include/q2a_encoder.h): all keys / per-clip key lengths / the packed valid rows
ENCODE_PLAIN, ENCODE_PADDED, ENCODE_VARLEN = 0, 1, 2
_KINDS = {"plain": ENCODE_PLAIN, "padded": ENCODE_PADDED, "varlen": ENCODE_VARLEN}

# activation contracts (include/q2a_encoder.h)
ACT_REFERENCE = 0
ACT_BF16 = 1

# element types of a feature destination (include/q2a_encoder.h, q2a_feat_dst)
DT_F32, DT_F16, DT_BF16 = 0, 1, 2


class FeatDst(C.Structure):
    """q2a_feat_dst: rows of the caller's on the device that the q2a_*_to calls store features into."""
    _fields_ = [("base", C.c_void_p), ("ld", C.c_int64), ("n_rows", C.c_int64), ("dtype", C.c_int32), ("reserved", C.c_int32)]


def feat_dst(base_ptr: int, ld: int, n_rows: int, dtype: int) -> FeatDst:
    return FeatDst(C.c_void_p(base_ptr) if base_ptr else None, ld, n_rows, dtype, 0)


class EmbedsSrc(C.Structure):
    """q2a_embeds_src: input_ids on the device, the audio token id, and the embedding table the text rows come from."""
    _fields_ = [("input_ids", C.c_void_p), ("ids_width", C.c_int32), ("reserved", C.c_int32), ("n_tokens", C.c_int64),
                ("audio_token_id", C.c_int64), ("embed_table", C.c_void_p), ("vocab", C.c_int64), ("table_ld", C.c_int64),
                ("report_dev", C.c_void_p)]


def embeds_src(ids_ptr: int, ids_width: int, n_tokens: int, audio_token_id: int, table_ptr: int = 0, vocab: int = 0,
               table_ld: int = 0, report_ptr: int = 0) -> EmbedsSrc:
    p = lambda a: C.c_void_p(a) if a else None   # noqa: E731
    return EmbedsSrc(p(ids_ptr), ids_width, 0, n_tokens, audio_token_id, p(table_ptr), vocab, table_ld, p(report_ptr))


_lib = None


def lib() -> C.CDLL:
    """Load libq2a.so (raises if it was not built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Q2AError(f"{LIB_PATH} not built; run `make -C {PKG_DIR}` (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIB_PATH)
        vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
        L.q2a_last_error.restype = C.c_char_p
        L.q2a_open.restype = vp
        L.q2a_open.argtypes = [C.c_char_p, C.c_int]
        L.q2a_open_ex.restype = vp
        L.q2a_open_ex.argtypes = [C.c_char_p, C.c_int, C.c_int]
        L.q2a_pack_model.restype = C.c_int64
        L.q2a_pack_model.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.q2a_pack_model_ex.restype = C.c_int64
        L.q2a_pack_model_ex.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.q2a_free_host_blob.argtypes = [vp]
        if hasattr(L, "q2a_pack_model_compact"):   # round 4 (optional: earlier diagnostic builds load too)
            L.q2a_pack_model_compact.restype = C.c_int64
            L.q2a_pack_model_compact.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
            L.q2a_blob_device_size.restype = C.c_int64
            L.q2a_blob_device_size.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64)]
            L.q2a_expand_blob.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int, vp]
        L.q2a_open_device_blob.restype = vp
        L.q2a_open_device_blob.argtypes = [vp, C.c_int64, C.c_int]
        L.q2a_close.argtypes = [vp]
        L.q2a_get_info.argtypes = [vp, C.POINTER(Info)]
        L.q2a_reserve.argtypes = [vp, C.c_int, C.c_int64]
        L.q2a_encode_device.argtypes = [vp, vp, C.c_int64, i32p, C.c_int, C.c_int, vp, i32p, vp]
        L.q2a_encode_host.argtypes = [vp, C.POINTER(vp), i32p, C.c_int, C.c_int, vp, i32p]
        L.q2a_encode_host_ex.argtypes = [vp, C.POINTER(vp), i32p, i32p, C.c_int, C.c_int, vp, i32p]
        L.q2a_pcm_to_mel.argtypes = [vp, vp, C.c_int, vp, C.c_int64, i32p]
        L.q2a_test_linear.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
        L.q2a_test_block.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        L.q2a_test_block_taps.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(vp), vp]
        L.q2a_test_attention.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
        # test hooks added in round 3: optional, so a diagnostic library of an earlier revision (diag/build_rev_lib.sh,
        # A/B runs) still loads; the shipped library exports them (tests/test_library_abi.py checks EXPORTS)
        for name, at in (("q2a_test_fc1_path", [vp, C.c_int]), ("q2a_test_frontend", [vp, vp, C.c_int64, i32p, C.c_int, vp, vp]),
                         ("q2a_test_pool_ln", [vp, vp, C.c_int, vp, vp])):
            if hasattr(L, name):
                getattr(L, name).argtypes = at
        if hasattr(L, "q2a_group_open"):   # round 5 (optional: earlier diagnostic builds load too)
            L.q2a_group_open.restype = vp
            L.q2a_group_open.argtypes = [C.c_char_p, i32p, C.c_int, C.c_int]
            L.q2a_group_open_with.restype = vp
            L.q2a_group_open_with.argtypes = [vp, i32p, C.c_int]
            L.q2a_group_close.argtypes = [vp]
            L.q2a_group_size.argtypes = [vp]
            L.q2a_group_engine.restype = vp
            L.q2a_group_engine.argtypes = [vp, C.c_int]
            L.q2a_group_split.argtypes = [C.c_int, C.c_int, C.c_int, i32p, i32p]
            L.q2a_group_encode_host.argtypes = [vp, C.POINTER(vp), i32p, i32p, C.c_int, C.c_int, vp, i32p]
            L.q2a_group_setup_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        # padding-aware encode (optional like the hooks above: an earlier diagnostic library still loads)
        for name, at in (("q2a_encode_device_padded", [vp, vp, C.c_int64, i32p, i32p, i32p, C.c_int, vp, i32p, i32p, vp]),
                         ("q2a_encode_host_padded", [vp, C.POINTER(vp), i32p, i32p, i32p, C.c_int, vp, i32p, i32p]),
                         ("q2a_test_attention_len", [vp, vp, vp, vp, C.c_int, i32p, vp, vp]),
                         ("q2a_test_block_len", [vp, C.c_int, vp, C.c_int, i32p, vp]),
                         # the variable-length family: the padded family's argument lists
                         ("q2a_encode_device_varlen", [vp, vp, C.c_int64, i32p, i32p, i32p, C.c_int, vp, i32p, i32p, vp]),
                         ("q2a_encode_host_varlen", [vp, C.POINTER(vp), i32p, i32p, i32p, C.c_int, vp, i32p, i32p]),
                         ("q2a_test_attention_varlen", [vp, vp, vp, vp, C.c_int, i32p, vp, vp]),
                         ("q2a_test_block_varlen", [vp, C.c_int, vp, C.c_int, i32p, vp])):
            if hasattr(L, name):
                getattr(L, name).argtypes = at
        if hasattr(L, "q2a_test_operand"):   # (optional like the hooks above)
            L.q2a_test_operand.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
        if hasattr(L, "q2a_test_gemm_epi"):   # (optional like the hooks above)
            L.q2a_test_gemm_epi.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp), C.c_int, vp]
            L.q2a_test_gemm_regime.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "q2a_encode_device_mel"):   # log-mel input (optional like the hooks above)
            L.q2a_mel_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, i32p, i32p]
            L.q2a_encode_device_mel.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int64, i32p, i32p, i32p, C.c_int, vp, i32p, i32p, vp]
            L.q2a_encode_host_mel.argtypes = [vp, C.c_int, C.POINTER(vp), i32p, i32p, i32p, C.c_int, vp, i32p, i32p]
            L.q2a_test_frontend_mel.argtypes = [vp, vp, C.c_int64, C.c_int64, i32p, i32p, C.c_int, vp, vp]
        if hasattr(L, "q2a_varlen_rows"):
            L.q2a_varlen_rows.restype = C.c_int64
            L.q2a_varlen_rows.argtypes = [i32p, C.c_int, C.c_int, i32p]
        if hasattr(L, "q2a_audio_features_device"):   # packed audio features (optional like the hooks above)
            L.q2a_packed_out_rows.restype = C.c_int64
            L.q2a_packed_out_rows.argtypes = [i32p, C.c_int, C.c_int, i32p]
            L.q2a_audio_features_device.argtypes = [vp, vp, vp, C.c_int64, i32p, i32p, i32p, C.c_int, vp, vp, C.c_int64,
                                                    i32p, i32p, vp]
            L.q2a_audio_features_device_mel.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, i32p, i32p, i32p, C.c_int, vp, vp,
                                                        C.c_int64, i32p, i32p, vp]
            L.q2a_audio_features_host.argtypes = [vp, vp, C.POINTER(vp), i32p, i32p, i32p, C.c_int, vp, vp, C.c_int64, i32p, i32p]
            L.q2a_audio_features_host_mel.argtypes = [vp, vp, C.POINTER(vp), i32p, i32p, i32p, C.c_int, vp, vp, C.c_int64, i32p,
                                                      i32p]
            L.q2a_test_pool_operand.argtypes = [vp, C.c_int, vp, C.c_int, i32p, vp, vp, vp, vp, C.c_int, vp]
        if hasattr(L, "q2a_audio_features_device_to"):   # 16-bit / in-place feature output (optional like the hooks above)
            dstp = C.POINTER(FeatDst)
            L.q2a_feat_rows.restype = C.c_int64
            L.q2a_feat_rows.argtypes = [i32p, i32p, C.c_int, C.c_int64, i32p]
            L.q2a_projector_apply_to.argtypes = [vp, vp, C.c_int64, dstp, vp, vp]
            L.q2a_projector_regime.argtypes = [vp, C.c_int64]
            L.q2a_audio_features_device_to.argtypes = [vp, vp, vp, C.c_int64, i32p, i32p, i32p, C.c_int, dstp, i32p, vp,
                                                       C.c_int64, i32p, i32p, vp]
            L.q2a_audio_features_device_mel_to.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, i32p, i32p, i32p, C.c_int, dstp,
                                                           i32p, vp, C.c_int64, i32p, i32p, vp]
        if hasattr(L, "q2a_inputs_embeds_device"):   # inputs_embeds from input_ids on the device
            dstp, srcp = C.POINTER(FeatDst), C.POINTER(EmbedsSrc)
            L.q2a_audio_token_rows.restype = C.c_int64
            L.q2a_audio_token_rows.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, i32p, C.c_int64]
            L.q2a_projector_apply_ids.argtypes = [vp, vp, C.c_int64, dstp, srcp, vp]
            L.q2a_inputs_embeds_device.argtypes = [vp, vp, vp, C.c_int64, i32p, i32p, i32p, C.c_int, dstp, srcp, vp, C.c_int64,
                                                   i32p, i32p, vp]
            L.q2a_inputs_embeds_device_mel.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, i32p, i32p, i32p, C.c_int, dstp, srcp,
                                                       vp, C.c_int64, i32p, i32p, vp]
            L.q2a_test_audio_token_rows.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp]
            L.q2a_test_embed_gather.argtypes = [srcp, dstp, C.c_int32, vp]
        L.q2a_projector_open.restype = vp
        L.q2a_projector_open.argtypes = [C.c_char_p, C.c_int]
        L.q2a_projector_close.argtypes = [vp]
        L.q2a_projector_get_dims.argtypes = [vp, i32p, i32p, i32p]
        L.q2a_projector_apply.argtypes = [vp, vp, C.c_int64, vp, vp]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        err = Q2AError(f"q2a error {rc}: {lib().q2a_last_error().decode()}")
        err.rc = rc   # the q2a_status code (include/q2a_encoder.h)
        raise err


class Engine:
    """One encoder engine on one HIP device (the analogue of a whisper_context + whisper_state)."""

    def __init__(self, model_path: str | None = None, device: int = 0, device_blob: int | None = None,
                 blob_size: int | None = None, act: int = ACT_REFERENCE):
        L = lib()
        if device_blob is not None:   # the blob carries its own activation contract
            h = L.q2a_open_device_blob(C.c_void_p(device_blob), C.c_int64(blob_size), device)
        else:
            h = L.q2a_open_ex(model_path.encode(), device, act)
        if not h:
            raise Q2AError(L.q2a_last_error().decode())
        self.h = h
        self.info = Info()
        _check(L.q2a_get_info(self.h, C.byref(self.info)))

    def close(self):
        if self.h:
            lib().q2a_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def out_shape(self):
        return (self.info.n_out, self.info.n_audio_state)

    def reserve(self, n_clips: int, max_samples: int = 0):
        _check(lib().q2a_reserve(self.h, n_clips, max_samples))
        _check(lib().q2a_get_info(self.h, C.byref(self.info)))

    def encode_device(self, pcm_ptr: int, pcm_stride: int, n_samples, out_ptr: int, offset_ms: int = 0,
                      stream: int | None = None):
        ns = np.ascontiguousarray(n_samples, dtype=np.int32)
        st = np.zeros(len(ns), dtype=np.int32)
        _check(lib().q2a_encode_device(self.h, C.c_void_p(pcm_ptr), C.c_int64(pcm_stride),
                                       ns.ctypes.data_as(C.POINTER(C.c_int32)), len(ns), offset_ms,
                                       C.c_void_p(out_ptr), st.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.c_void_p(stream) if stream else None))
        return st

    def encode_host(self, clips, offset_ms: int = 0, out: np.ndarray | None = None, offsets_ms=None,
                    raise_on_error: bool = True):
        """Encode host PCM clips. offsets_ms: per-clip window offsets (q2a_encode_host_ex). With raise_on_error=False a
        failing call returns (out, status, rc) instead of raising: status then marks every clip whose output never
        reached `out` as CLIP_FAILED."""
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        n = len(clips)
        if out is None:
            out = np.zeros((n,) + self.out_shape, dtype=np.float32)
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in clips])
        ns = np.array([len(c) for c in clips], dtype=np.int32)
        st = np.full(n, -1, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        if offsets_ms is None:
            rc = lib().q2a_encode_host(self.h, ptrs, ns.ctypes.data_as(i32p), n, offset_ms,
                                       C.c_void_p(out.ctypes.data), st.ctypes.data_as(i32p))
        else:
            offs = np.ascontiguousarray(offsets_ms, dtype=np.int32)
            assert len(offs) == n
            rc = lib().q2a_encode_host_ex(self.h, ptrs, ns.ctypes.data_as(i32p), offs.ctypes.data_as(i32p), n, offset_ms,
                                          C.c_void_p(out.ctypes.data), st.ctypes.data_as(i32p))
        if not raise_on_error:
            return out, st, rc
        _check(rc)
        return out, st

    def encode_device_padded(self, pcm_ptr: int, pcm_stride: int, n_samples, out_ptr: int, offsets_ms=None, key_len=None,
                             stream: int | None = None, _fn: str = "q2a_encode_device_padded"):
        """q2a_encode_device_padded: per-clip key lengths in every block's attention (key_len=None: valid_lengths'
        enc_len of each clip), output rows >= out_len written as zeros. Returns (out_len, status)."""
        i32p = C.POINTER(C.c_int32)
        ns = np.ascontiguousarray(n_samples, dtype=np.int32)
        n = len(ns)
        offs = None if offsets_ms is None else np.ascontiguousarray(offsets_ms, dtype=np.int32)
        kl = None if key_len is None else np.ascontiguousarray(key_len, dtype=np.int32)
        if (offs is not None and len(offs) != n) or (kl is not None and len(kl) != n):
            raise ValueError(f"offsets_ms / key_len need {n} entries")
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        _check(getattr(lib(), _fn)(self.h, C.c_void_p(pcm_ptr), C.c_int64(pcm_stride), ns.ctypes.data_as(i32p),
                                   offs.ctypes.data_as(i32p) if offs is not None else None,
                                   kl.ctypes.data_as(i32p) if kl is not None else None, n,
                                   C.c_void_p(out_ptr), ol.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
                                   C.c_void_p(stream) if stream else None))
        return ol, st

    def encode_device_varlen(self, pcm_ptr: int, pcm_stride: int, n_samples, out_ptr: int, offsets_ms=None, key_len=None,
                             stream: int | None = None):
        """q2a_encode_device_varlen: encode_device_padded's arguments, results and output bytes, with the encoder
        blocks run on the clips' valid rows only (packed per varlen_rows). Returns (out_len, status)."""
        return self.encode_device_padded(pcm_ptr, pcm_stride, n_samples, out_ptr, offsets_ms=offsets_ms, key_len=key_len,
                                         stream=stream, _fn="q2a_encode_device_varlen")

    def encode_host_padded(self, clips, offsets_ms=None, key_len=None, out: np.ndarray | None = None,
                           return_status: bool = False, _fn: str = "q2a_encode_host_padded"):
        """q2a_encode_host_padded over host PCM clips -> (out, out_len) (with return_status: (out, out_len, status))."""
        i32p = C.POINTER(C.c_int32)
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        n = len(clips)
        if out is None:
            out = np.zeros((n,) + self.out_shape, dtype=np.float32)
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in clips])
        ns = np.array([len(c) for c in clips], dtype=np.int32)
        offs = None if offsets_ms is None else np.ascontiguousarray(offsets_ms, dtype=np.int32)
        kl = None if key_len is None else np.ascontiguousarray(key_len, dtype=np.int32)
        if (offs is not None and len(offs) != n) or (kl is not None and len(kl) != n):
            raise ValueError(f"offsets_ms / key_len need {n} entries")
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        _check(getattr(lib(), _fn)(self.h, ptrs, ns.ctypes.data_as(i32p),
                                   offs.ctypes.data_as(i32p) if offs is not None else None,
                                   kl.ctypes.data_as(i32p) if kl is not None else None, n,
                                   C.c_void_p(out.ctypes.data), ol.ctypes.data_as(i32p), st.ctypes.data_as(i32p)))
        return (out, ol, st) if return_status else (out, ol)

    def encode_host_varlen(self, clips, offsets_ms=None, key_len=None, out: np.ndarray | None = None,
                           return_status: bool = False):
        """q2a_encode_host_varlen: encode_host_padded's arguments, results and output bytes on the packed rows."""
        return self.encode_host_padded(clips, offsets_ms=offsets_ms, key_len=key_len, out=out, return_status=return_status,
                                       _fn="q2a_encode_host_varlen")

    # ---- log-mel input (q2a_encode_device_mel / q2a_encode_host_mel): the caller's normalised f32 mel, zeros past n_len
    @staticmethod
    def _i32(a, n, what):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.int32)
        if len(a) != n:
            raise ValueError(f"{what} needs {n} entries")
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    def encode_device_mel(self, mel_ptr: int, clip_stride: int, ld: int, n_len, out_ptr: int, kind: int = ENCODE_PLAIN,
                          seek=None, key_len=None, stream: int | None = None):
        """q2a_encode_device_mel: clip c is [n_mels][ld] f32 at mel_ptr + 4 * c * clip_stride (clip_stride 0: one array
        for every clip) with n_len[c] frames, encoded from frame seek[c] (None: 0). kind ENCODE_*; key_len=None:
        mel_valid_lengths' enc_len. Returns (out_len, status); out_len is not written for ENCODE_PLAIN (zeros)."""
        i32p = C.POINTER(C.c_int32)
        nl = np.ascontiguousarray(n_len, dtype=np.int32)
        n = len(nl)
        _sk, skp = self._i32(seek, n, "seek")
        _kl, klp = self._i32(key_len, n, "key_len")
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        _check(lib().q2a_encode_device_mel(self.h, kind, C.c_void_p(mel_ptr), C.c_int64(clip_stride), C.c_int64(ld),
                                           nl.ctypes.data_as(i32p), skp, klp, n, C.c_void_p(out_ptr),
                                           ol.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
                                           C.c_void_p(stream) if stream else None))
        return ol, st

    def encode_host_mel(self, mels, kind: int = ENCODE_PLAIN, seek=None, key_len=None, out: np.ndarray | None = None,
                        raise_on_error: bool = True):
        """q2a_encode_host_mel over host arrays mels[c] = [n_mels][n_len[c]] f32 -> (out, out_len, status); with
        raise_on_error=False a failing call returns (out, out_len, status, rc)."""
        i32p = C.POINTER(C.c_int32)
        mels = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        n = len(mels)
        for m in mels:
            if m.ndim != 2 or m.shape[0] != self.info.n_mels:
                raise ValueError(f"mel arrays must be [{self.info.n_mels}][n_len]")
        if out is None:
            out = np.zeros((n,) + self.out_shape, dtype=np.float32)
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in mels])
        nl = np.array([m.shape[1] for m in mels], dtype=np.int32)
        _sk, skp = self._i32(seek, n, "seek")
        _kl, klp = self._i32(key_len, n, "key_len")
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        rc = lib().q2a_encode_host_mel(self.h, kind, ptrs, nl.ctypes.data_as(i32p), skp, klp, n, C.c_void_p(out.ctypes.data),
                                       ol.ctypes.data_as(i32p), st.ctypes.data_as(i32p))
        if not raise_on_error:
            return out, ol, st, rc
        _check(rc)
        return out, ol, st

    def test_frontend_mel(self, mel_ptr, clip_stride, ld, n_len, x_ptr, seek=None, stream=None):
        nl = np.ascontiguousarray(n_len, dtype=np.int32)
        _sk, skp = self._i32(seek, len(nl), "seek")
        _check(lib().q2a_test_frontend_mel(self.h, C.c_void_p(mel_ptr), C.c_int64(clip_stride), C.c_int64(ld),
                                           nl.ctypes.data_as(C.POINTER(C.c_int32)), skp, len(nl), C.c_void_p(x_ptr),
                                           C.c_void_p(stream) if stream else None))

    def encode_features(self, input_features, feature_attention_mask=None, kind: str = "varlen"):
        """Encode what transformers' Qwen2AudioProcessor hands the model: input_features [B][n_mels][L] f32 (a torch
        CUDA tensor: device entry point on torch's current stream, the result a tensor on that device; or a numpy
        array: host entry point) and optionally feature_attention_mask [B][L]. With a mask the key lengths are
        features_key_len(mask.sum(-1)); without one mel_valid_lengths' enc_len of L frames. kind "plain", "padded" or
        "varlen". Returns (out [B][n_out][n_audio_state], out_len [B]): rows >= out_len[c] are zeros for the
        key-length kinds, for "plain" every row is computed and out_len is n_out."""
        k = _KINDS[kind]
        shape = tuple(input_features.shape)
        if len(shape) != 3 or shape[1] != self.info.n_mels:
            raise ValueError(f"input_features must be [B][{self.info.n_mels}][L]")
        B, _, L = shape
        kl = None
        if feature_attention_mask is not None and k != ENCODE_PLAIN:
            m = feature_attention_mask
            m = m.detach().cpu().numpy() if hasattr(m, "detach") else np.asarray(m)
            if m.shape != (B, L):
                raise ValueError(f"feature_attention_mask must be [{B}][{L}]")
            kl = features_key_len(m.astype(np.int64).sum(-1))
        if hasattr(input_features, "is_cuda"):
            import torch
            if not input_features.is_cuda or input_features.dtype != torch.float32:
                raise ValueError("input_features: a float32 CUDA tensor (or a numpy array)")
            x = input_features.contiguous()
            out = torch.empty((B,) + self.out_shape, dtype=torch.float32, device=x.device)
            ol, _ = self.encode_device_mel(x.data_ptr(), self.info.n_mels * L, L, [L] * B, out.data_ptr(), kind=k, key_len=kl,
                                           stream=torch.cuda.current_stream(x.device).cuda_stream)
        else:
            x = np.ascontiguousarray(input_features, dtype=np.float32)
            out, ol, _ = self.encode_host_mel(list(x), kind=k, key_len=kl)
        if k == ENCODE_PLAIN:
            ol = np.full(B, self.info.n_out, dtype=np.int32)
        return out, ol

    # ---- audio features (q2a_audio_features_*): the valid output rows of all clips packed, through the projector
    def _features_device(self, fn, projector, data_ptr, strides, lens, second, what, key_len, sink, stream):
        """One device feature call: fn(engine, projector, data, *strides, lens, second, key_len, n, *sink, out_len,
        status, stream). second: offsets_ms or seek (named by `what`); a 0 pointer goes as NULL. Returns (out_len, status)."""
        i32p = C.POINTER(C.c_int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = len(lens)
        _sd, sdp = self._i32(second, n, what)
        _kl, klp = self._i32(key_len, n, "key_len")
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        p = lambda a: C.c_void_p(a) if a else None   # noqa: E731
        _check(fn(self.h, projector.h if projector is not None else None, p(data_ptr), *[C.c_int64(v) for v in strides],
                  lens.ctypes.data_as(i32p), sdp, klp, n, *[p(a) if isinstance(a, int) else a for a in sink],
                  ol.ctypes.data_as(i32p), st.ctypes.data_as(i32p), p(stream)))
        return ol, st

    @staticmethod
    def _ref(struct):
        return C.byref(struct) if struct is not None else None

    def audio_features_device(self, pcm_ptr: int, pcm_stride: int, n_samples, feat_ptr: int, embd_ptr: int, rows_cap: int,
                              projector=None, offsets_ms=None, key_len=None, stream: int | None = None):
        """q2a_audio_features_device: encode_device_varlen's inputs; feat_ptr [rows_cap][d_out] (0 without a projector)
        and embd_ptr [rows_cap][n_audio_state] (0: not written) receive clip c's out_len[c] rows at the prefix sum of
        out_len (packed_out_rows). Returns (out_len, status)."""
        return self._features_device(lib().q2a_audio_features_device, projector, pcm_ptr, (pcm_stride,), n_samples, offsets_ms,
                                     "offsets_ms", key_len, (feat_ptr, embd_ptr, C.c_int64(rows_cap)), stream)

    def audio_features_device_mel(self, mel_ptr: int, clip_stride: int, ld: int, n_len, feat_ptr: int, embd_ptr: int,
                                  rows_cap: int, projector=None, seek=None, key_len=None, stream: int | None = None):
        """q2a_audio_features_device_mel: encode_device_mel's inputs (kind ENCODE_VARLEN), audio_features_device's
        outputs. Returns (out_len, status)."""
        return self._features_device(lib().q2a_audio_features_device_mel, projector, mel_ptr, (clip_stride, ld), n_len, seek,
                                     "seek", key_len, (feat_ptr, embd_ptr, C.c_int64(rows_cap)), stream)

    def audio_features_device_to(self, pcm_ptr: int, pcm_stride: int, n_samples, dst: FeatDst, projector, clip_rows=None,
                                 embd_ptr: int = 0, embd_rows_cap: int = 0, offsets_ms=None, key_len=None,
                                 stream: int | None = None):
        """q2a_audio_features_device_to: audio_features_device with the features stored as dst's type into dst's rows,
        clip c's out_len[c] rows from row clip_rows[c] on (None: packed); embd_ptr [embd_rows_cap][n_audio_state] still
        receives the packed f32 rows (0: not written). Returns (out_len, status)."""
        _cr, crp = self._i32(clip_rows, len(n_samples), "clip_rows")
        return self._features_device(lib().q2a_audio_features_device_to, projector, pcm_ptr, (pcm_stride,), n_samples, offsets_ms,
                                     "offsets_ms", key_len, (self._ref(dst), crp, embd_ptr, C.c_int64(embd_rows_cap)), stream)

    def audio_features_device_mel_to(self, mel_ptr: int, clip_stride: int, ld: int, n_len, dst: FeatDst, projector,
                                     clip_rows=None, embd_ptr: int = 0, embd_rows_cap: int = 0, seek=None, key_len=None,
                                     stream: int | None = None):
        """q2a_audio_features_device_mel_to: audio_features_device_mel's inputs, audio_features_device_to's outputs."""
        _cr, crp = self._i32(clip_rows, len(n_len), "clip_rows")
        return self._features_device(lib().q2a_audio_features_device_mel_to, projector, mel_ptr, (clip_stride, ld), n_len, seek,
                                     "seek", key_len, (self._ref(dst), crp, embd_ptr, C.c_int64(embd_rows_cap)), stream)

    def inputs_embeds_device(self, pcm_ptr: int, pcm_stride: int, n_samples, dst: FeatDst, src: EmbedsSrc, projector,
                             embd_ptr: int = 0, embd_rows_cap: int = 0, offsets_ms=None, key_len=None,
                             stream: int | None = None):
        """q2a_inputs_embeds_device: audio_features_device_to with the rows placed by src's input_ids (the k-th feature
        row at the k-th audio token) and the text rows gathered from src's embedding table. Returns (out_len, status)."""
        return self._features_device(lib().q2a_inputs_embeds_device, projector, pcm_ptr, (pcm_stride,), n_samples, offsets_ms,
                                     "offsets_ms", key_len, (self._ref(dst), self._ref(src), embd_ptr, C.c_int64(embd_rows_cap)), stream)

    def inputs_embeds_device_mel(self, mel_ptr: int, clip_stride: int, ld: int, n_len, dst: FeatDst, src: EmbedsSrc, projector,
                                 embd_ptr: int = 0, embd_rows_cap: int = 0, seek=None, key_len=None,
                                 stream: int | None = None):
        """q2a_inputs_embeds_device_mel: audio_features_device_mel's inputs, inputs_embeds_device's outputs."""
        return self._features_device(lib().q2a_inputs_embeds_device_mel, projector, mel_ptr, (clip_stride, ld), n_len, seek,
                                     "seek", key_len, (self._ref(dst), self._ref(src), embd_ptr, C.c_int64(embd_rows_cap)), stream)

    def _features_host(self, fn, ptrs, lens, n, second, key_len, projector, embd, rows_cap, raise_on_error):
        i32p = C.POINTER(C.c_int32)
        _kl, klp = self._i32(key_len, n, "key_len")
        if rows_cap is None:   # the key lengths bound the rows; without them a full window per clip
            rows_cap = int((_kl // 2).sum()) if _kl is not None else n * self.info.n_out
        feat = np.zeros((rows_cap, projector.d_out), dtype=np.float32) if projector is not None else None
        emb = np.zeros((rows_cap, self.info.n_audio_state), dtype=np.float32) if embd else None
        st = np.full(n, -1, dtype=np.int32)
        ol = np.zeros(n, dtype=np.int32)
        rc = fn(self.h, projector.h if projector is not None else None, ptrs, lens.ctypes.data_as(i32p), second, klp, n,
                C.c_void_p(feat.ctypes.data) if feat is not None else None,
                C.c_void_p(emb.ctypes.data) if emb is not None else None, C.c_int64(rows_cap), ol.ctypes.data_as(i32p),
                st.ctypes.data_as(i32p))
        if raise_on_error:
            _check(rc)
        n_tot = int(ol.sum())
        res = (feat[:n_tot] if feat is not None else None, emb[:n_tot] if emb is not None else None, ol, st)
        return res if raise_on_error else res + (rc,)

    def audio_features_host(self, clips, projector=None, offsets_ms=None, key_len=None, embd: bool = True,
                            rows_cap: int | None = None, raise_on_error: bool = True):
        """q2a_audio_features_host over host PCM clips -> (feat [N_tot][d_out] or None without a projector, embd
        [N_tot][n_audio_state] or None with embd=False, out_len, status); with raise_on_error=False also rc."""
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        n = len(clips)
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in clips])
        ns = np.array([len(c) for c in clips], dtype=np.int32)
        _of, ofp = self._i32(offsets_ms, n, "offsets_ms")
        return self._features_host(lib().q2a_audio_features_host, ptrs, ns, n, ofp, key_len, projector, embd, rows_cap,
                                   raise_on_error)

    def audio_features_host_mel(self, mels, projector=None, seek=None, key_len=None, embd: bool = True,
                                rows_cap: int | None = None, raise_on_error: bool = True):
        """q2a_audio_features_host_mel over host arrays mels[c] = [n_mels][n_len[c]] f32; results as audio_features_host."""
        mels = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        n = len(mels)
        for m in mels:
            if m.ndim != 2 or m.shape[0] != self.info.n_mels:
                raise ValueError(f"mel arrays must be [{self.info.n_mels}][n_len]")
        ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in mels])
        nl = np.array([m.shape[1] for m in mels], dtype=np.int32)
        _sk, skp = self._i32(seek, n, "seek")
        return self._features_host(lib().q2a_audio_features_host_mel, ptrs, nl, n, skp, key_len, projector, embd, rows_cap,
                                   raise_on_error)

    def audio_features(self, input_features, feature_attention_mask=None, projector=None, return_embd: bool = False,
                       out=None, clip_rows=None):
        """What Qwen2AudioForConditionalGeneration scatters into the text embeddings, from what its processor hands the
        model: input_features [B][n_mels][L] f32 (a torch CUDA tensor: device entry point on torch's current stream, the
        results tensors on that device; or a numpy array: host entry point) and optionally feature_attention_mask [B][L]
        — encode_features' argument handling. Returns (features [N_tot][d_out], out_len [B]): the projector applied to
        the valid rows of embd_enc alone, clip c's out_len[c] rows at the prefix sum of out_len; with return_embd also
        the packed embd_enc [N_tot][n_audio_state]. projector=None (return_embd required): features is None.
        out: a contiguous CUDA tensor [rows][d_out] or [B][S][d_out] (viewed as rows) of float32, float16 or bfloat16 —
        inputs_embeds. The features are then written into it (q2a_audio_features_device_mel_to, on torch's current
        stream), clip c's rows from flat row clip_rows[c] on (audio_token_runs' starts; None: packed from row 0), and
        out is returned in place of the packed features. input_features must be a CUDA tensor on out's device."""
        if out is not None:
            return self._audio_features_into(input_features, feature_attention_mask, projector, return_embd, out, clip_rows)
        if clip_rows is not None:
            raise ValueError("audio_features: clip_rows goes with out")
        if projector is None and not return_embd:
            raise ValueError("audio_features: a projector, or return_embd=True")
        shape = tuple(input_features.shape)
        if len(shape) != 3 or shape[1] != self.info.n_mels:
            raise ValueError(f"input_features must be [B][{self.info.n_mels}][L]")
        B, _, L = shape
        if feature_attention_mask is not None:
            m = feature_attention_mask
            m = m.detach().cpu().numpy() if hasattr(m, "detach") else np.asarray(m)
            if m.shape != (B, L):
                raise ValueError(f"feature_attention_mask must be [{B}][{L}]")
            kl = features_key_len(m.astype(np.int64).sum(-1))
        else:
            kl = np.full(B, mel_valid_lengths(L, 0, self.info.n_audio_ctx)[0], dtype=np.int32)
        n_tot, _ = packed_out_rows(kl, self.info.n_audio_ctx)   # (log-mel input: no clip is skipped)
        if hasattr(input_features, "is_cuda"):
            import torch
            if not input_features.is_cuda or input_features.dtype != torch.float32:
                raise ValueError("input_features: a float32 CUDA tensor (or a numpy array)")
            x = input_features.contiguous()
            feat = torch.empty((n_tot, projector.d_out), dtype=torch.float32, device=x.device) if projector is not None else None
            emb = torch.empty((n_tot, self.info.n_audio_state), dtype=torch.float32, device=x.device) if return_embd else None
            ol = np.zeros(B, dtype=np.int32)
            if n_tot:   # (an empty tensor has no pointer to pass)
                ol, _ = self.audio_features_device_mel(x.data_ptr(), self.info.n_mels * L, L, [L] * B,
                                                       feat.data_ptr() if feat is not None else 0,
                                                       emb.data_ptr() if emb is not None else 0, n_tot, projector=projector,
                                                       key_len=kl, stream=torch.cuda.current_stream(x.device).cuda_stream)
        else:
            x = np.ascontiguousarray(input_features, dtype=np.float32)
            feat, emb, ol, _ = self.audio_features_host_mel(list(x), projector=projector, key_len=kl, embd=return_embd,
                                                            rows_cap=n_tot)
        return (feat, ol, emb) if return_embd else (feat, ol)

    def _audio_features_into(self, input_features, feature_attention_mask, projector, return_embd, out, clip_rows):
        import torch
        if projector is None:
            raise ValueError("audio_features: out needs a projector")
        dts = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.is_contiguous() and out.dtype in dts and out.dim() in (2, 3)
                and out.shape[-1] == projector.d_out):
            raise ValueError(f"out: a contiguous CUDA tensor [rows][{projector.d_out}] or [B][S][{projector.d_out}] of "
                             "float32, float16 or bfloat16")
        x = input_features
        if not (hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.float32 and x.device == out.device):
            raise ValueError("input_features: a float32 CUDA tensor on out's device")
        shape = tuple(x.shape)
        if len(shape) != 3 or shape[1] != self.info.n_mels:
            raise ValueError(f"input_features must be [B][{self.info.n_mels}][L]")
        B, _, L = shape
        if feature_attention_mask is not None:
            m = feature_attention_mask
            m = m.detach().cpu().numpy() if hasattr(m, "detach") else np.asarray(m)
            if m.shape != (B, L):
                raise ValueError(f"feature_attention_mask must be [{B}][{L}]")
            kl = features_key_len(m.astype(np.int64).sum(-1))
        else:
            kl = np.full(B, mel_valid_lengths(L, 0, self.info.n_audio_ctx)[0], dtype=np.int32)
        n_tot, _ = packed_out_rows(kl, self.info.n_audio_ctx)
        n_rows = out.numel() // projector.d_out
        x = x.contiguous()
        emb = torch.empty((n_tot, self.info.n_audio_state), dtype=torch.float32, device=x.device) if return_embd else None
        ol = np.zeros(B, dtype=np.int32)
        if n_tot:
            dst = feat_dst(out.data_ptr(), projector.d_out, n_rows, dts[out.dtype])
            ol, _ = self.audio_features_device_mel_to(x.data_ptr(), self.info.n_mels * L, L, [L] * B, dst, projector,
                                                      clip_rows=clip_rows, embd_ptr=emb.data_ptr() if emb is not None else 0,
                                                      embd_rows_cap=n_tot, key_len=kl,
                                                      stream=torch.cuda.current_stream(x.device).cuda_stream)
        return (out, ol, emb) if return_embd else (out, ol)

    def inputs_embeds(self, input_features, feature_attention_mask, input_ids, audio_token_id: int, projector,
                      embed_tokens=None, out=None, check: bool = True):
        """The language model's inputs_embeds in one call (q2a_inputs_embeds_device_mel, on torch's current stream):
        embed_tokens[input_ids] with the k-th audio feature row stored at the k-th position whose id is audio_token_id —
        Qwen2AudioForConditionalGeneration's embedding pass, cast and masked_scatter, without a host copy of input_ids.
        input_features [B][n_mels][L] f32 (CUDA) and feature_attention_mask [B][L] (or None) as for audio_features — the
        key lengths are host arithmetic, so a mask that lives on the device is copied back; pass it as a host tensor;
        input_ids: a contiguous CUDA int32 or int64 tensor [B][S] or [n]; embed_tokens: the embedding weight [vocab][d_out]
        of out's dtype on that device (rows may be strided), or None: text rows keep what out holds; out: a contiguous
        CUDA tensor input_ids.shape + (d_out,) of float32 / float16 / bfloat16 (None: allocated, embed_tokens' dtype, or
        float32 zeros without a table). Returns (inputs_embeds, out_len [B], report): report is a CUDA int32[4] tensor —
        audio tokens found, feature rows, text ids outside [0, vocab), flags (bit 0: found != rows, bit 1: bad ids). With
        check=True the four words are read (one synchronising copy) and a mismatch or a bad id raises ValueError;
        check=False reads nothing on the host."""
        import torch
        if projector is None:
            raise ValueError("inputs_embeds: a projector is required")
        ids = input_ids
        if not (hasattr(ids, "is_cuda") and ids.is_cuda and ids.dtype in (torch.int32, torch.int64) and ids.dim() in (1, 2)
                and ids.is_contiguous() and ids.numel() >= 1):
            raise ValueError("input_ids: a contiguous CUDA int32 or int64 tensor [B][S] or [n]")
        n_tok = ids.numel()
        if n_tok > 1 << 24:
            raise ValueError("input_ids: at most 2^24 tokens")
        d_out = projector.d_out
        dts = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
        tab = embed_tokens
        if tab is not None and not (hasattr(tab, "is_cuda") and tab.is_cuda and tab.device == ids.device and tab.dim() == 2
                                    and tab.shape[1] == d_out and tab.dtype in dts and tab.stride(1) == 1 and tab.shape[0] >= 1
                                    and tab.stride(0) >= d_out):
            raise ValueError(f"embed_tokens: a CUDA tensor [vocab][{d_out}] of float32, float16 or bfloat16 on input_ids' device")
        if out is None:
            shape = tuple(ids.shape) + (d_out,)
            out = (torch.empty(shape, dtype=tab.dtype, device=ids.device) if tab is not None
                   else torch.zeros(shape, dtype=torch.float32, device=ids.device))
        elif not (hasattr(out, "is_cuda") and out.is_cuda and out.device == ids.device and out.is_contiguous() and out.dtype in dts
                  and tuple(out.shape) == tuple(ids.shape) + (d_out,)):
            raise ValueError(f"out: a contiguous CUDA tensor input_ids.shape + ({d_out},) of float32, float16 or bfloat16")
        if tab is not None and tab.dtype != out.dtype:
            raise ValueError("embed_tokens: out's dtype")
        x = input_features
        if not (hasattr(x, "is_cuda") and x.is_cuda and x.dtype == torch.float32 and x.device == out.device):
            raise ValueError("input_features: a float32 CUDA tensor on input_ids' device")
        shape = tuple(x.shape)
        if len(shape) != 3 or shape[1] != self.info.n_mels:
            raise ValueError(f"input_features must be [B][{self.info.n_mels}][L]")
        B, _, L = shape
        if feature_attention_mask is not None:
            m = feature_attention_mask
            m = m.detach().cpu().numpy() if hasattr(m, "detach") else np.asarray(m)
            if m.shape != (B, L):
                raise ValueError(f"feature_attention_mask must be [{B}][{L}]")
            kl = features_key_len(m.astype(np.int64).sum(-1))
        else:
            kl = np.full(B, mel_valid_lengths(L, 0, self.info.n_audio_ctx)[0], dtype=np.int32)
        x = x.contiguous()
        report = torch.empty(4, dtype=torch.int32, device=ids.device)
        dst = feat_dst(out.data_ptr(), d_out, n_tok, dts[out.dtype])
        src = embeds_src(ids.data_ptr(), ids.element_size(), n_tok, int(audio_token_id),
                         tab.data_ptr() if tab is not None else 0, tab.shape[0] if tab is not None else 0,
                         tab.stride(0) if tab is not None else 0, report.data_ptr())
        ol, _ = self.inputs_embeds_device_mel(x.data_ptr(), self.info.n_mels * L, L, [L] * B, dst, src, projector, key_len=kl,
                                              stream=torch.cuda.current_stream(x.device).cuda_stream)
        if check:
            found, rows, bad, flags = (int(v) for v in report.cpu())
            if flags:
                raise ValueError(f"inputs_embeds: {found} audio tokens in input_ids for {rows} audio feature rows, "
                                 f"{bad} text ids outside the embedding table")
        return out, ol, report

    def test_pool_operand(self, mode, x_ptr, n_clips, key_len, embd_ptr=0, codes_ptr=0, dy_ptr=0, aext_ptr=0, ld=0, stream=None):
        """q2a_test_pool_operand: the audio-feature calls' pool kernel alone on packed caller rows x [M_tot][D] ->
        embd [N_tot][D] f32 and / or the operand of `mode` (0 fp16, 1 Q8_K, 2 Q8_0) in test_operand's layouts."""
        kl = np.ascontiguousarray(key_len, dtype=np.int32)
        assert len(kl) == n_clips
        p = lambda a: C.c_void_p(a) if a else None   # noqa: E731
        _check(lib().q2a_test_pool_operand(self.h, mode, p(x_ptr), n_clips, kl.ctypes.data_as(C.POINTER(C.c_int32)),
                                           p(embd_ptr), p(codes_ptr), p(dy_ptr), p(aext_ptr), ld, p(stream)))

    def pcm_to_mel(self, pcm: np.ndarray) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n_len = (len(pcm) + 480000) // 160
        out = np.empty((self.info.n_mels, n_len), dtype=np.float32)
        got = C.c_int32(0)
        _check(lib().q2a_pcm_to_mel(self.h, C.c_void_p(pcm.ctypes.data), len(pcm), C.c_void_p(out.ctypes.data),
                                    C.c_int64(out.size), C.byref(got)))
        assert got.value == n_len
        return out

    # kernel-level entry points on device pointers (parity tests)
    def test_linear(self, layer, which, x_ptr, M, y_ptr, stream=None):
        _check(lib().q2a_test_linear(self.h, layer, which, C.c_void_p(x_ptr), M, C.c_void_p(y_ptr),
                                     C.c_void_p(stream) if stream else None))

    def test_block(self, layer, x_ptr, n_clips, stream=None):
        _check(lib().q2a_test_block(self.h, layer, C.c_void_p(x_ptr), n_clips, C.c_void_p(stream) if stream else None))

    def test_block_taps(self, layer, x_ptr, n_clips, tap_ptrs, stream=None):
        arr = (C.c_void_p * 4)(*[C.c_void_p(t) if t else None for t in tap_ptrs])
        _check(lib().q2a_test_block_taps(self.h, layer, C.c_void_p(x_ptr), n_clips, arr,
                                         C.c_void_p(stream) if stream else None))

    def test_frontend(self, pcm_ptr, pcm_stride, n_samples, x_ptr, stream=None):
        ns = np.ascontiguousarray(n_samples, dtype=np.int32)
        _check(lib().q2a_test_frontend(self.h, C.c_void_p(pcm_ptr), C.c_int64(pcm_stride),
                                       ns.ctypes.data_as(C.POINTER(C.c_int32)), len(ns), C.c_void_p(x_ptr),
                                       C.c_void_p(stream) if stream else None))

    def test_pool_ln(self, x_ptr, n_clips, out_ptr, stream=None):
        _check(lib().q2a_test_pool_ln(self.h, C.c_void_p(x_ptr), n_clips, C.c_void_p(out_ptr),
                                      C.c_void_p(stream) if stream else None))

    def test_fc1_path(self, path):
        _check(lib().q2a_test_fc1_path(self.h, path))

    def test_operand(self, producer, mode, x_ptr, M, K, out_ptr, dy_ptr=0, aext_ptr=0, ld=None, g_ptr=0, b_ptr=0, stream=None):
        """q2a_test_operand: one conversion kernel (OPERAND_*) on caller rows; ld defaults to M."""
        p = lambda a: C.c_void_p(a) if a else None   # noqa: E731
        _check(lib().q2a_test_operand(self.h, producer, mode, p(x_ptr), M, K, p(g_ptr), p(b_ptr), p(out_ptr), p(dy_ptr),
                                      p(aext_ptr), M if ld is None else ld, p(stream)))

    def test_gemm_epi(self, layer, which, epi, x_ptr, M, out_ptrs, ld=0, stream=None):
        """q2a_test_gemm_epi: the block's GEMM `which` with its fused epilogue EPI_* on caller rows, stored straight into
        the caller's buffers out_ptrs (their order: include/q2a_encoder.h)."""
        arr = (C.c_void_p * 6)(*([C.c_void_p(p) if p else None for p in out_ptrs] + [None] * (6 - len(out_ptrs))))
        _check(lib().q2a_test_gemm_epi(self.h, layer, which, epi, C.c_void_p(x_ptr), M, arr, ld,
                                       C.c_void_p(stream) if stream else None))

    def test_gemm_regime(self, which, epi, M) -> int:
        """q2a_test_gemm_regime: the REGIME_* the launcher picks for that GEMM at M rows on this device."""
        rg = lib().q2a_test_gemm_regime(self.h, which, epi, M)
        if rg < 0:
            _check(rg)
        return rg

    def test_attention(self, q_ptr, k_ptr, v_ptr, n_clips, out_ptr, stream=None):
        _check(lib().q2a_test_attention(self.h, C.c_void_p(q_ptr), C.c_void_p(k_ptr), C.c_void_p(v_ptr), n_clips,
                                        C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    # the same two with per-clip key lengths (host list, uploaded by the call)
    def test_attention_len(self, q_ptr, k_ptr, v_ptr, n_clips, key_len, out_ptr, stream=None):
        kl = np.ascontiguousarray(key_len, dtype=np.int32)
        assert len(kl) == n_clips
        _check(lib().q2a_test_attention_len(self.h, C.c_void_p(q_ptr), C.c_void_p(k_ptr), C.c_void_p(v_ptr), n_clips,
                                            kl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out_ptr),
                                            C.c_void_p(stream) if stream else None))

    def test_block_len(self, layer, x_ptr, n_clips, key_len, stream=None):
        kl = np.ascontiguousarray(key_len, dtype=np.int32)
        assert len(kl) == n_clips
        _check(lib().q2a_test_block_len(self.h, layer, C.c_void_p(x_ptr), n_clips,
                                        kl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream) if stream else None))

    # the same two on packed rows (varlen_rows over key_len): q, k, v, out and x are [M_tot][D]
    def test_attention_varlen(self, q_ptr, k_ptr, v_ptr, n_clips, key_len, out_ptr, stream=None):
        kl = np.ascontiguousarray(key_len, dtype=np.int32)
        assert len(kl) == n_clips
        _check(lib().q2a_test_attention_varlen(self.h, C.c_void_p(q_ptr), C.c_void_p(k_ptr), C.c_void_p(v_ptr), n_clips,
                                               kl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out_ptr),
                                               C.c_void_p(stream) if stream else None))

    def test_block_varlen(self, layer, x_ptr, n_clips, key_len, stream=None):
        kl = np.ascontiguousarray(key_len, dtype=np.int32)
        assert len(kl) == n_clips
        _check(lib().q2a_test_block_varlen(self.h, layer, C.c_void_p(x_ptr), n_clips,
                                           kl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream) if stream else None))


_host_lib = None


def _host() -> C.CDLL:
    """lib/libq2a_host.so: host arithmetic, needs no GPU."""
    global _host_lib
    if _host_lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise Q2AError(f"{HOST_LIB_PATH} not built; run `make -C {PKG_DIR} host`")
        _host_lib = C.CDLL(HOST_LIB_PATH)
        _host_lib.q2a_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _host_lib.q2a_mel_valid_lengths.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _host_lib.q2a_varlen_rows.restype = C.c_int64
        _host_lib.q2a_varlen_rows.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _host_lib.q2a_packed_out_rows.restype = C.c_int64
        _host_lib.q2a_packed_out_rows.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _host_lib.q2a_feat_rows.restype = C.c_int64
        _host_lib.q2a_feat_rows.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int64, C.POINTER(C.c_int32)]
        _host_lib.q2a_audio_token_rows.restype = C.c_int64
        _host_lib.q2a_audio_token_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64]
    return _host_lib


def varlen_rows(key_len, n_audio_ctx: int = 1500) -> tuple[int, np.ndarray]:
    """(M_tot, row_start): the packed layout of the variable-length encode (q2a_varlen_rows) — clip c occupies rows
    row_start[c] .. row_start[c+1]-1 (its key length rounded up to 16, inside the window; none for key length 0) of
    M_tot = row_start[-1] rows. Host arithmetic through lib/libq2a_host.so: needs no GPU."""
    kl = np.ascontiguousarray(key_len, dtype=np.int32)
    rs = np.zeros(len(kl) + 1, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    m = _host().q2a_varlen_rows(kl.ctypes.data_as(i32p), len(kl), n_audio_ctx, rs.ctypes.data_as(i32p))
    if m < 0:
        err = Q2AError(f"q2a error {m}: invalid arguments to q2a_varlen_rows")
        err.rc = int(m)
        raise err
    return int(m), rs


def packed_out_rows(key_len, n_audio_ctx: int = 1500) -> tuple[int, np.ndarray]:
    """(N_tot, out_start): the packed output layout of the audio-feature calls (q2a_packed_out_rows) — clip c's
    key_len[c] // 2 output rows are rows out_start[c] .. out_start[c+1]-1 of N_tot = out_start[-1]. Host arithmetic
    through lib/libq2a_host.so: needs no GPU."""
    kl = np.ascontiguousarray(key_len, dtype=np.int32).reshape(-1)
    os_ = np.zeros(len(kl) + 1, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    n = _host().q2a_packed_out_rows(kl.ctypes.data_as(i32p), len(kl), n_audio_ctx, os_.ctypes.data_as(i32p))
    if n < 0:
        err = Q2AError(f"q2a error {n}: invalid arguments to q2a_packed_out_rows")
        err.rc = int(n)
        raise err
    return int(n), os_


def feat_rows(out_len, clip_rows, n_rows: int, row_map: np.ndarray | None = None) -> tuple[int, np.ndarray]:
    """(N_tot, row_map): the destination rows of the audio-feature _to calls (q2a_feat_rows) — packed row m of the call
    goes to row row_map[m]; clip c's out_len[c] rows are rows clip_rows[c] .. of a destination of n_rows rows
    (clip_rows None: packed from row 0; a clip with no rows is ignored). Raises Q2AError (rc -4) for a negative start, a
    range past n_rows or two non-empty ranges that overlap, and then writes nothing into row_map (an int32 array of at
    least N_tot entries to fill; None: a new one). Host arithmetic through lib/libq2a_host.so: needs no GPU."""
    ol = np.ascontiguousarray(out_len, dtype=np.int32).reshape(-1)
    cr = None if clip_rows is None else np.ascontiguousarray(clip_rows, dtype=np.int32).reshape(-1)
    if cr is not None and len(cr) != len(ol):
        raise ValueError("clip_rows: one entry per clip")
    if row_map is None:
        row_map = np.zeros(int(np.maximum(ol, 0).sum()), dtype=np.int32)
    elif row_map.dtype != np.int32 or not row_map.flags.c_contiguous or row_map.size < int(np.maximum(ol, 0).sum()):
        raise ValueError("row_map: a contiguous int32 array of at least sum(out_len) entries")
    i32p = C.POINTER(C.c_int32)
    n = _host().q2a_feat_rows(ol.ctypes.data_as(i32p), cr.ctypes.data_as(i32p) if cr is not None else None, len(ol),
                              C.c_int64(n_rows), row_map.ctypes.data_as(i32p))
    if n < 0:
        err = Q2AError(f"q2a error {n}: invalid arguments to q2a_feat_rows")
        err.rc = int(n)
        raise err
    return int(n), row_map


def audio_token_rows(input_ids, audio_token_id: int, map_cap: int | None = None) -> tuple[int, np.ndarray]:
    """(count, row_map): the row map the inputs_embeds calls derive on the device (q2a_audio_token_rows) — row_map[k] is
    the flat position of the k-th entry of input_ids (numpy int32 or int64, any shape, row-major) equal to
    audio_token_id, -1 for count <= k < map_cap (None: map_cap = count). count is the number found, also where it
    exceeds map_cap. Host arithmetic through lib/libq2a_host.so: needs no GPU."""
    ids = np.asarray(input_ids)
    if ids.dtype not in (np.int32, np.int64):
        raise ValueError("input_ids: int32 or int64")
    ids = np.ascontiguousarray(ids).reshape(-1)
    fn = _host().q2a_audio_token_rows
    i32p = C.POINTER(C.c_int32)
    args = (ids.ctypes.data_as(C.c_void_p), ids.itemsize, C.c_int64(ids.size), C.c_int64(int(audio_token_id)))
    if map_cap is None:
        map_cap = int(fn(*args, None, C.c_int64(0)))
    if map_cap < 0:
        raise ValueError("map_cap must be >= 0")
    row_map = np.zeros(map_cap, dtype=np.int32)
    n = fn(*args, row_map.ctypes.data_as(i32p) if map_cap else None, C.c_int64(map_cap))
    if n < 0:
        err = Q2AError(f"q2a error {n}: invalid arguments to q2a_audio_token_rows")
        err.rc = int(n)
        raise err
    return int(n), row_map


def test_embed_gather(src: EmbedsSrc, dst: FeatDst, d_out: int, stream=None):
    """q2a_test_embed_gather: the text-row gather of the inputs_embeds calls alone."""
    _check(lib().q2a_test_embed_gather(C.byref(src) if src is not None else None, C.byref(dst) if dst is not None else None,
                                       d_out, C.c_void_p(stream) if stream else None))


test_embed_gather.__test__ = False   # (a library hook, not a test)


def audio_token_runs(input_ids, audio_token_id: int) -> tuple[np.ndarray, np.ndarray]:
    """(starts, lengths) of every maximal run of audio_token_id in input_ids [B][S] (numpy, host only), in row-major
    order: starts are flat rows b * S + s of inputs_embeds viewed as [B * S][d], a run never crosses a sequence's end.
    The starts are the clip_rows of Engine.audio_features(..., out=inputs_embeds) once the lengths have been checked
    against out_len — the processor emits one run of out_len[c] audio tokens per clip."""
    ids = np.asarray(input_ids)
    if ids.ndim != 2:
        raise ValueError("input_ids must be [B][S]")
    B, S = ids.shape
    hit = np.zeros((B, S + 2), dtype=np.int8)
    hit[:, 1:-1] = ids == audio_token_id
    d = np.diff(hit, axis=1)          # +1 where a run starts (at s), -1 one past its end
    b0, s0 = np.nonzero(d == 1)
    _, s1 = np.nonzero(d == -1)
    return (b0 * S + s0).astype(np.int64), (s1 - s0).astype(np.int64)


def valid_lengths(n_samples: int, offset_ms: int = 0, n_audio_ctx: int = 1500) -> tuple[int, int]:
    """(enc_len, out_len): the valid encoder positions and output vectors of a clip of n_samples samples encoded from
    offset_ms (q2a_valid_lengths). Host arithmetic through lib/libq2a_host.so: needs no GPU."""
    a, b = C.c_int32(), C.c_int32()
    rc = _host().q2a_valid_lengths(n_samples, offset_ms, n_audio_ctx, C.byref(a), C.byref(b))
    if rc != 0:
        err = Q2AError(f"q2a error {rc}: invalid arguments to q2a_valid_lengths")
        err.rc = rc
        raise err
    return a.value, b.value


def mel_valid_lengths(n_len: int, seek: int = 0, n_audio_ctx: int = 1500) -> tuple[int, int]:
    """(enc_len, out_len) of n_len log-mel frames encoded from frame seek (q2a_mel_valid_lengths). Host arithmetic
    through lib/libq2a_host.so: needs no GPU."""
    a, b = C.c_int32(), C.c_int32()
    rc = _host().q2a_mel_valid_lengths(n_len, seek, n_audio_ctx, C.byref(a), C.byref(b))
    if rc != 0:
        err = Q2AError(f"q2a error {rc}: invalid arguments to q2a_mel_valid_lengths")
        err.rc = rc
        raise err
    return a.value, b.value


def features_key_len(n_frames) -> np.ndarray:
    """Engine.encode_features' key lengths from the valid mel frames of each clip (feature_attention_mask.sum(-1)):
    (n - 1) // 2 + 1, the encoder positions transformers' _get_feat_extract_output_lengths keeps after conv2."""
    return ((np.asarray(n_frames, dtype=np.int64) - 1) // 2 + 1).astype(np.int32)


def group_split(n_clips: int, n_devices: int) -> list[range]:
    """The contiguous clip ranges q2a_group gives each device (q2a_group_split)."""
    out = []
    for i in range(n_devices):
        f, c = C.c_int32(), C.c_int32()
        _check(lib().q2a_group_split(n_clips, n_devices, i, C.byref(f), C.byref(c)))
        out.append(range(f.value, f.value + c.value))
    return out


class Group:
    """Several GPUs in ONE process (q2a_group_*): one RCCL broadcast of the weights at open, then clip batches split
    into contiguous ranges, a host thread per device. devices=None: every visible device.
    From a model file (q2a_group_open: the compact blob packed once on the host), or with engine= an open Engine
    (q2a_group_open_with: its own device-layout weights are the broadcast's root, its device's group engine shares
    them; the Engine must outlive the group)."""

    def __init__(self, model_path: str | None = None, devices=None, act: int = ACT_REFERENCE, engine=None):
        L = lib()
        devs = np.ascontiguousarray(devices if devices is not None else [], dtype=np.int32)
        dptr = devs.ctypes.data_as(C.POINTER(C.c_int32)) if len(devs) else None
        if engine is not None:
            self.h = L.q2a_group_open_with(C.c_void_p(engine.h), dptr, len(devs))
        else:
            self.h = L.q2a_group_open(model_path.encode(), dptr, len(devs), act)
        if not self.h:
            raise Q2AError(L.q2a_last_error().decode())
        self.size = L.q2a_group_size(self.h)
        info = Info()
        _check(L.q2a_get_info(L.q2a_group_engine(self.h, 0), C.byref(info)))
        self.out_shape = (info.n_out, info.n_audio_state)

    def setup_times(self) -> dict:
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        _check(lib().q2a_group_setup_times(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"pack_s": a.value, "broadcast_s": b.value, "open_s": c.value, "blob_bytes": n.value}

    def encode_host(self, clips, offset_ms: int = 0, offsets_ms=None, out: np.ndarray | None = None):
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        n = len(clips)
        if out is None:
            out = np.zeros((n,) + self.out_shape, dtype=np.float32)
        ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in clips])
        ns = np.array([len(c) for c in clips], dtype=np.int32)
        st = np.full(n, -1, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        offs = None if offsets_ms is None else np.ascontiguousarray(offsets_ms, dtype=np.int32)
        if offs is not None and len(offs) != n:
            raise ValueError(f"offsets_ms has {len(offs)} entries for {n} clips")
        _check(lib().q2a_group_encode_host(self.h, ptrs, ns.ctypes.data_as(i32p),
                                           offs.ctypes.data_as(i32p) if offs is not None else None, n, offset_ms,
                                           C.c_void_p(out.ctypes.data), st.ctypes.data_as(i32p)))
        return out, st

    def close(self):
        if self.h:
            lib().q2a_group_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Projector:
    """The Qwen2-Audio multi-modal projector (Linear d_model -> text hidden, bias) on the GPU: the consumer of embd_enc
    (include/q2a_encoder.h, q2a_projector_*). No CPU fallback."""

    def __init__(self, path: str, device: int = 0):
        self.h = lib().q2a_projector_open(path.encode(), device)
        if not self.h:
            raise Q2AError(lib().q2a_last_error().decode())
        a, b, w = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().q2a_projector_get_dims(self.h, C.byref(a), C.byref(b), C.byref(w)))
        self.d_in, self.d_out, self.wtype = a.value, b.value, w.value

    def apply(self, x_ptr: int, rows: int, y_ptr: int, stream=None):
        _check(lib().q2a_projector_apply(self.h, C.c_void_p(x_ptr), rows, C.c_void_p(y_ptr),
                                         C.c_void_p(stream) if stream else None))

    def apply_to(self, x_ptr: int, rows: int, dst: FeatDst, row_map_ptr: int = 0, stream=None):
        """q2a_projector_apply_to: apply's values as dst's type, packed row m stored at row row_map[m] of dst
        (row_map_ptr: device int32 [rows]; 0: the identity)."""
        _check(lib().q2a_projector_apply_to(self.h, C.c_void_p(x_ptr), rows, C.byref(dst) if dst is not None else None,
                                            C.c_void_p(row_map_ptr) if row_map_ptr else None,
                                            C.c_void_p(stream) if stream else None))

    def apply_ids(self, x_ptr: int, rows: int, dst: FeatDst, src: EmbedsSrc, stream=None):
        """q2a_projector_apply_ids: apply_to with the row map derived on the device from src's input_ids (feature row k
        at the k-th audio token), and the text rows gathered from src's embedding table."""
        _check(lib().q2a_projector_apply_ids(self.h, C.c_void_p(x_ptr), rows, C.byref(dst) if dst is not None else None,
                                             C.byref(src) if src is not None else None,
                                             C.c_void_p(stream) if stream else None))

    def test_audio_token_rows(self, ids_ptr: int, ids_width: int, n_tokens: int, audio_token_id: int, n_feat: int,
                              row_map_ptr: int, report_ptr: int, stream=None):
        """q2a_test_audio_token_rows: the compaction of the inputs_embeds calls alone — the n_feat map words to
        row_map_ptr (device int32 [n_feat]), {found, n_feat, 0, found != n_feat} to report_ptr (device int32[4])."""
        p = lambda a: C.c_void_p(a) if a else None   # noqa: E731
        _check(lib().q2a_test_audio_token_rows(self.h, p(ids_ptr), ids_width, C.c_int64(n_tokens), C.c_int64(audio_token_id),
                                               C.c_int64(n_feat), p(row_map_ptr), p(report_ptr), p(stream)))

    def regime(self, rows: int) -> int:
        """q2a_projector_regime: the REGIME_* the projector's GEMM takes at `rows` rows (nothing is launched)."""
        r = lib().q2a_projector_regime(self.h, rows)
        if r < 0:
            _check(r)
        return r

    def close(self):
        if self.h:
            lib().q2a_projector_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def pack_model(path: str, act: int = ACT_REFERENCE, compact: bool = False) -> bytearray:
    """Pack a model file into a blob (host bytes, one copy out of the library's buffer): the device layout, or with
    compact=True its transport form (ggml weight rows, expanded on the GPU by Engine(device_blob=...)), e.g. for the
    RCCL broadcast."""
    p = C.c_void_p()
    f = lib().q2a_pack_model_compact if compact else lib().q2a_pack_model_ex
    n = f(path.encode(), act, C.byref(p))
    if n < 0:
        raise Q2AError(lib().q2a_last_error().decode())
    try:
        out = bytearray(n)
        C.memmove((C.c_char * n).from_buffer(out), p, n)
        return out
    finally:
        lib().q2a_free_host_blob(p)


def blob_device_size(blob) -> tuple[int, int]:
    """(device-layout bytes, transport bytes) of a host blob (its header)."""
    head = (C.c_char * 32768).from_buffer_copy(bytes(blob[:32768]))
    tb = C.c_int64(0)
    n = lib().q2a_blob_device_size(C.cast(head, C.c_void_p), 32768, C.byref(tb))
    if n < 0:
        raise Q2AError(lib().q2a_last_error().decode())
    return int(n), int(tb.value)


def expand_blob(dev_ptr: int, size: int, out_ptr: int, out_bytes: int, device: int = 0, stream=None):
    """Expand a compact blob on the device into the device layout (what q2a_open_device_blob does internally)."""
    _check(lib().q2a_expand_blob(C.c_void_p(dev_ptr), C.c_int64(size), C.c_void_p(out_ptr), C.c_int64(out_bytes),
                                 device, C.c_void_p(stream) if stream else None))
