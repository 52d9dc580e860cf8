"""Reader for the reference's unchanged ggml model file (numpy, no execution of file content).

Layout restated from models/convert-pt-to-ggml.py:268-337 and whisper_model_load
(src/qwen2-whisper.cpp:1350-1872).
"""
from __future__ import annotations

import dataclasses
import struct

import numpy as np

MAGIC = 0x67676D6C
TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q8_0, TYPE_Q4_K, TYPE_Q8_K = 0, 1, 2, 8, 12, 15
TYPE_Q5_K, TYPE_Q6_K = 13, 14
FTYPE_TO_WTYPE = {0: TYPE_F32, 1: TYPE_F16, 2: TYPE_Q4_0, 7: TYPE_Q8_0, 12: TYPE_Q4_K, 13: TYPE_Q5_K, 14: TYPE_Q6_K}
HPARAM_NAMES = ("n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_mels", "ftype")


def row_size(t: int, n: int) -> int:
    if t == TYPE_F32:
        return 4 * n
    if t == TYPE_F16:
        return 2 * n
    if t == TYPE_Q4_0:
        return (n // 32) * 18
    if t == TYPE_Q8_0:
        return (n // 32) * 34
    if t == TYPE_Q4_K:
        return (n // 256) * 144
    if t == TYPE_Q5_K:
        return (n // 256) * 176
    if t == TYPE_Q6_K:
        return (n // 256) * 210
    if t == TYPE_Q8_K:
        return (n // 256) * 292
    raise ValueError(f"unsupported ggml type {t}")


@dataclasses.dataclass
class Tensor:
    name: str
    type: int
    ne: tuple          # ggml order: ne[0] fastest
    data: np.ndarray   # raw bytes (uint8) or typed view for F32/F16
    offset: int = 0    # of the payload in the file

    def as_f32(self) -> np.ndarray:
        if self.type == TYPE_F32:
            return self.data.view(np.float32).reshape(tuple(reversed(self.ne)))
        if self.type == TYPE_F16:
            return self.data.view(np.float16).astype(np.float32).reshape(tuple(reversed(self.ne)))
        if self.type in (TYPE_Q5_K, TYPE_Q6_K):
            return self._dequant_kq()
        raise ValueError("quantized tensor has no plain f32 view")

    def kq(self) -> dict:
        """The integer view of a Q5_K / Q6_K tensor, rows = prod(ne[1:]), nb = ne[0] / 256 blocks per row:
        Q5_K: d, dmin f32 [rows][nb]; sc, m int32 [rows][nb][8] (6-bit, get_scale_min_k4); q int32 [rows][K] in 0..31
              (weight = d*sc*q - dmin*m per 32-weight sub-block, dequantize_row_q5_K ggml-quants.c:2763)
        Q6_K: d f32 [rows][nb]; sc int32 [rows][nb][16] (int8); q int32 [rows][K] in 0..63
              (weight = d*sc*(q - 32) per 16-weight sub-block, dequantize_row_q6_K ggml-quants.c:2977)"""
        K = self.ne[0]
        rows, nb = int(np.prod(self.ne)) // K, K // 256
        if self.type == TYPE_Q5_K:
            blk = self.data.reshape(rows, nb, 176)
            d = blk[:, :, 0:2].copy().view(np.float16).astype(np.float32)[..., 0]
            dmin = blk[:, :, 2:4].copy().view(np.float16).astype(np.float32)[..., 0]
            s = blk[:, :, 4:16].astype(np.int32)
            sc = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], axis=-1)
            m = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], axis=-1)
            qh = blk[:, :, 16:48].astype(np.int32)                         # [rows][nb][32]
            qs = blk[:, :, 48:176].astype(np.int32).reshape(rows, nb, 4, 32)
            q = np.empty((rows, nb, 8, 32), np.int32)
            for g in range(4):   # 64 weights per group: low nibbles + bit 2g of qh, then high nibbles + bit 2g+1
                q[:, :, 2 * g] = (qs[:, :, g] & 0xF) + (((qh >> (2 * g)) & 1) << 4)
                q[:, :, 2 * g + 1] = (qs[:, :, g] >> 4) + (((qh >> (2 * g + 1)) & 1) << 4)
            return {"d": d, "dmin": dmin, "sc": sc, "m": m, "q": q.reshape(rows, K)}
        if self.type == TYPE_Q6_K:
            blk = self.data.reshape(rows, nb, 210)
            ql = blk[:, :, 0:128].astype(np.int32).reshape(rows, nb, 2, 2, 32)   # [half][l / 32][l % 32]
            qh = blk[:, :, 128:192].astype(np.int32).reshape(rows, nb, 2, 32)
            sc = blk[:, :, 192:208].copy().view(np.int8).astype(np.int32)
            d = blk[:, :, 208:210].copy().view(np.float16).astype(np.float32)[..., 0]
            q = np.empty((rows, nb, 2, 4, 32), np.int32)
            q[:, :, :, 0] = (ql[:, :, :, 0] & 0xF) | (((qh >> 0) & 3) << 4)
            q[:, :, :, 1] = (ql[:, :, :, 1] & 0xF) | (((qh >> 2) & 3) << 4)
            q[:, :, :, 2] = (ql[:, :, :, 0] >> 4) | (((qh >> 4) & 3) << 4)
            q[:, :, :, 3] = (ql[:, :, :, 1] >> 4) | (((qh >> 6) & 3) << 4)
            return {"d": d, "sc": sc, "q": q.reshape(rows, K)}
        raise ValueError("not a Q5_K / Q6_K tensor")

    def _dequant_kq(self) -> np.ndarray:
        """dequantize_row_q5_K / dequantize_row_q6_K, their f32 operations in their order"""
        K = self.ne[0]
        v = self.kq()
        rows, nb = v["d"].shape
        f = np.float32
        if self.type == TYPE_Q5_K:
            d1 = (v["d"][..., None] * v["sc"].astype(f)).astype(f)         # d * sc
            m1 = (v["dmin"][..., None] * v["m"].astype(f)).astype(f)       # min * m
            q = v["q"].reshape(rows, nb, 8, 32).astype(f)
            y = ((d1[..., None] * q).astype(f) - m1[..., None]).astype(f)
        else:
            ds = (v["d"][..., None] * v["sc"].astype(f)).astype(f)         # d * sc
            q = (v["q"] - 32).reshape(rows, nb, 16, 16).astype(f)
            y = (ds[..., None] * q).astype(f)
        return y.reshape(tuple(reversed(self.ne)))


@dataclasses.dataclass
class ModelFile:
    hparams: dict
    qntvr: int
    wtype: int
    filters: np.ndarray  # [n_mel][n_fft]
    tensors: dict

    def t(self, name: str) -> Tensor:
        return self.tensors[name]


def read(path: str) -> ModelFile:
    buf = np.fromfile(path, dtype=np.uint8)
    mv = memoryview(buf)
    off = 0

    def i32():
        nonlocal off
        v = struct.unpack_from("<i", mv, off)[0]
        off += 4
        return v

    magic = struct.unpack_from("<I", mv, 0)[0]
    off = 4
    if magic != MAGIC:
        raise ValueError("invalid model data (bad magic)")
    hp = {k: i32() for k in HPARAM_NAMES}
    qntvr = hp["ftype"] // 1000
    ft = hp["ftype"] % 1000
    if ft not in FTYPE_TO_WTYPE:
        raise ValueError(f"unsupported ftype {ft}")
    n_mel, n_fft = i32(), i32()
    filters = buf[off:off + 4 * n_mel * n_fft].view(np.float32).reshape(n_mel, n_fft)
    off += 4 * n_mel * n_fft
    n_vocab = i32()
    for _ in range(n_vocab):
        ln = struct.unpack_from("<I", mv, off)[0]
        off += 4 + ln
    tensors = {}
    while off < len(buf):
        n_dims, ln, ttype = i32(), i32(), i32()
        ne = tuple(i32() for _ in range(n_dims))
        name = bytes(buf[off:off + ln]).decode()
        off += ln
        nel = int(np.prod(ne))
        nbytes = row_size(ttype, ne[0]) * (nel // ne[0])
        tensors[name] = Tensor(name, ttype, ne, buf[off:off + nbytes], off)
        off += nbytes
    return ModelFile(hp, qntvr, FTYPE_TO_WTYPE[ft], filters, tensors)
