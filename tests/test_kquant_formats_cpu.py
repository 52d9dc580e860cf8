"""CPU checks of the Q5_K / Q6_K format layer: the byte-exact quantizers behind `q2a_tool quantize IN OUT q5_k|q6_k`,
the Python decoder (q2a/ggmlfile.py) and the host packer (device layout and compact transport form). The reference's
bytes and hashes come from tests/golden/golden_kq.* (make_golden_kq.py: `ref_harness quantize-model IN OUT 13|14`)."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import kquant_cases as kc
from conftest import GOLDEN_DIR, TOOL, _sha
from q2a import ggmlfile
from test_pack_cpu import (A_COUNT, A_DX, A_W, G_COUNT, L_COUNT, L_MAT0, OFF_COMPACT, OFF_GOFF, OFF_TOTAL, bf16_bits,
                           header)

TYPES = ["q5_k", "q6_k"]
A_DMIN, A_WEXT, A_BETA, A_GAMMA = 2, 3, 4, 5
A_SC = A_WEXT   # Q6_K keeps its sub-block scales in the WEXT slot


@pytest.fixture(scope="module")
def golden_kq():
    return kc.load_golden_kq(GOLDEN_DIR)


@pytest.fixture(scope="module")
def ext_model(make_model, workdir, golden_kq):
    """The hand-made rows (tests/kquant_cases.py) in the tiny F16 model, quantized by bin/q2a_tool."""
    meta, _ = golden_kq

    def make(wt):
        ext = os.path.join(workdir, "tinyext-f16.bin")
        if not os.path.exists(ext):
            kc.write_ext_model(make_model("tiny", "f16"), ext)
        assert _sha(ext) == meta["models"]["tinyext-f16"]["sha256"], "the hand-made input drifted"
        path = os.path.join(workdir, f"tinyext-{wt}.bin")
        if not os.path.exists(path):
            subprocess.check_call([TOOL, "quantize", ext, path, wt, "8"])
        return path

    return make


# ---------------------------------------------------------------- quantizers
@pytest.mark.parametrize("wt", TYPES)
def test_tool_quantizes_the_tiny_model_like_the_reference(make_model, golden_kq, wt):
    """q2a_quantize_row_q5_K / _q6_K and the file writer: the whole file has the SHA-256 of the reference's."""
    meta, _ = golden_kq
    path = make_model("tiny", wt)   # (conftest passes the type name through to the tool)
    assert _sha(path) == meta["models"][f"tiny-{wt}"]["sha256"]
    mf = ggmlfile.read(path)
    assert mf.wtype == kc.WT_TYPE[wt] and mf.hparams["ftype"] == 2000 + kc.WT_FTYPE[wt]
    assert mf.t("layers.0.fc1.weight").type == kc.WT_TYPE[wt]
    assert mf.t("conv1.weight").type == ggmlfile.TYPE_F16 and mf.t("embed_positions.weight").type == ggmlfile.TYPE_F32


@pytest.mark.parametrize("wt", TYPES)
def test_tool_quantizes_the_hand_made_rows_like_the_reference(ext_model, golden_kq, wt):
    """All-zero 256-blocks (Q6_K's GROUP_MAX_EPS branch, Q5_K's d = 0), a block with a single large outlier, constant
    and alternating rows: the file hash, and the hand-made rows' bytes one tensor at a time."""
    meta, kq = golden_kq
    path = ext_model(wt)
    mf = ggmlfile.read(path)
    for i, name in enumerate(kc.EXT_TENSORS):
        t = mf.t(name)
        n = kc.EXT_ROWS * ggmlfile.row_size(t.type, t.ne[0])
        assert np.array_equal(t.data[:n], kq[f"ext_{wt}_{i}"]), name
    assert _sha(path) == meta["models"][f"tinyext-{wt}"]["sha256"]
    # the branches are really there: zeroed blocks (row 0: every block; row 5: the first)
    v = mf.t("layers.0.fc2.weight").kq()
    assert (v["d"][0] == 0).all() and v["d"][5, 0] == 0 and (v["d"][5, 1:] != 0).all()
    if wt == "q6_k":
        blk = mf.t("layers.0.fc2.weight").data.reshape(-1, 4, 210)
        assert not blk[0].any() and not blk[5, 0].any()   # memset(&y[i], 0, sizeof(block_q6_K))


# ---------------------------------------------------------------- Python decode
def _recombine(t):
    """dequantize_row_q5_K / _q6_K element by element from the integer view (f32 operations in ggml's order)."""
    v = t.kq()
    K = t.ne[0]
    rows, nb = v["d"].shape
    f = np.float32
    if t.type == ggmlfile.TYPE_Q5_K:
        j = np.arange(K) // 32 % 8
        b = np.arange(K) // 256
        d1 = (v["d"][:, b] * v["sc"][:, b, j].astype(f)).astype(f)
        m1 = (v["dmin"][:, b] * v["m"][:, b, j].astype(f)).astype(f)
        return ((d1 * v["q"].astype(f)).astype(f) - m1).astype(f)
    j = np.arange(K) // 16 % 16
    b = np.arange(K) // 256
    return ((v["d"][:, b] * v["sc"][:, b, j].astype(f)).astype(f) * (v["q"] - 32).astype(f)).astype(f)


@pytest.mark.parametrize("wt", TYPES)
def test_python_decode_and_the_end_codes(ext_model, wt):
    """as_f32 = the integer view recombined; equal bit for bit (after bf16 rounding) to what the C packer dequantizes
    (the bf16 contract's blob holds dequant_row's values). The hand-made rows reach both ends of the codes, so the GPU
    tests on this file cover them: Q5_K q = 31 with sc = 63; Q6_K sc = -128 with q = 0 and with q = 63."""
    import q2a
    path = ext_model(wt)
    mf = ggmlfile.read(path)
    for name in kc.EXT_TENSORS:
        t = mf.t(name)
        w = t.as_f32()
        assert w.dtype == np.float32 and w.shape == (t.ne[1], t.ne[0])
        assert np.array_equal(w.view(np.uint32), _recombine(t).view(np.uint32)), name
        v = t.kq()
        K, nb = t.ne[0], t.ne[0] // 256
        if wt == "q5_k":
            sc = np.repeat(v["sc"].reshape(-1, nb * 8), 32, axis=1)
            assert v["q"].min() == 0 and v["q"].max() == 31 and v["sc"].max() == 63 and v["m"].max() == 63
            assert ((v["q"] == 31) & (sc == 63)).any(), name
            assert ((v["q"][2] == 31) & (sc[2] == 63)).all(), "the constant row sits at the end code"
        else:
            sc = np.repeat(v["sc"].reshape(-1, nb * 16), 16, axis=1)
            assert v["q"].min() == 0 and v["q"].max() == 63 and v["sc"].min() == -128
            assert ((v["q"] == 0) & (sc == -128)).any() and ((v["q"] == 63) & (sc == -128)).any(), name
            assert ((v["q"][2] == 0) & (sc[2] == -128)).all(), "the constant row sits at the end code"
            assert (sc[3] == -128).all() and (v["q"][3, 1::2] == 63).all(), "the alternating row's -1s sit at q = 63"
    blob = q2a.pack_model(path, q2a.ACT_BF16)
    wtype, blk, act, total, loff0 = header(blob)
    assert (wtype, blk, act, total) == (kc.WT_TYPE[wt], 0, q2a.ACT_BF16, len(blob)) and loff0[L_MAT0 + A_DX] == 0
    want = np.concatenate([bf16_bits(mf.t(f"layers.0.self_attn.{n}_proj.weight").as_f32()) for n in "qkv"])
    got = np.frombuffer(blob, dtype=np.uint16, count=3 * kc.D * kc.D, offset=loff0[L_MAT0 + A_W]).reshape(3 * kc.D, kc.D)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("wt", TYPES)
def test_device_layout_holds_the_integer_operands(ext_model, wt):
    """Layer 0's fc2 (four 256-blocks) in the packed blob: Q5_K = Q4_K's sections with sc*q from the 5-bit codes (zero
    weights and dx = 1 for a d = 0 block); Q6_K = q - 32, dx = d [K/256][N] and the sub-block-major scales [K/16][N]."""
    import q2a
    path = ext_model(wt)
    blob = q2a.pack_model(path)
    wtype, blk, act, total, loff0 = header(blob)
    assert (wtype, blk, act, total) == (kc.WT_TYPE[wt], 256, q2a.ACT_REFERENCE, len(blob))
    t = ggmlfile.read(path).t("layers.0.fc2.weight")
    v = t.kq()
    N, K, nb = kc.D, kc.F, kc.F // 256
    a = loff0[L_MAT0 + 3 * A_COUNT:L_MAT0 + 4 * A_COUNT]
    W = np.frombuffer(blob, dtype=np.float16, count=N * K, offset=a[A_W]).reshape(N, K).astype(np.int64)
    dx = np.frombuffer(blob, dtype=np.float32, count=nb * N, offset=a[A_DX]).reshape(nb, N)
    if wt == "q5_k":
        live = np.repeat(v["d"] != 0, 256, axis=1)
        want = v["q"].reshape(N, nb, 8, 32) * v["sc"][..., None]
        assert np.array_equal(W, np.where(live, want.reshape(N, K), 0)) and W.max() == 63 * 31
        assert np.array_equal(dx.T, np.where(v["d"] != 0, v["d"], np.float32(1)))
        dmin = np.frombuffer(blob, dtype=np.float32, count=nb * N, offset=a[A_DMIN]).reshape(nb, N)
        wext = np.frombuffer(blob, dtype=np.float16, count=nb * N * 16, offset=a[A_WEXT]).reshape(nb, N, 8, 2)
        assert np.array_equal(dmin.T, v["dmin"])
        assert np.array_equal(wext[..., 1].astype(np.int64), v["m"].transpose(1, 0, 2))
        assert np.array_equal(wext[..., 0].astype(np.int64), 64 * v["m"].transpose(1, 0, 2))
        assert a[A_BETA] and a[A_GAMMA]
    else:
        assert np.array_equal(W, v["q"] - 32) and W.min() == -32 and W.max() == 31
        assert np.array_equal(dx.T, v["d"])
        sc = np.frombuffer(blob, dtype=np.float32, count=(K // 16) * N, offset=a[A_SC]).reshape(K // 16, N)
        assert np.array_equal(sc.T.astype(np.int64), v["sc"].reshape(N, K // 16))
        assert a[A_DMIN] == 0 and a[A_BETA] == 0 and a[A_GAMMA] == 0


@pytest.mark.parametrize("wt", TYPES)
def test_compact_blob_and_header_validation(make_model, wt):
    """The compact transport form: the header (compact = 1), the small sections, then the file's own rows — its size is
    exactly that sum; header validation accepts both forms and refuses a moved offset or a device size that is not the
    plan's."""
    import q2a
    path = make_model("tiny", wt)
    full = q2a.pack_model(path)
    comp = q2a.pack_model(path, compact=True)
    assert struct.unpack_from("<i", comp, OFF_COMPACT)[0] == 1 and struct.unpack_from("<i", full, OFF_COMPACT)[0] == 0
    hc = bytearray(comp[:32768])
    hc[OFF_COMPACT:OFF_COMPACT + 4] = b"\0\0\0\0"
    assert bytearray(full[:32768]) == hc
    assert q2a.blob_device_size(comp) == (len(full), len(comp)) and q2a.blob_device_size(full) == (len(full), len(full))
    pad = lambda n: (n + 255) & ~255  # noqa: E731
    _, _, _, _, loff0 = header(full)
    L = struct.unpack_from("<i", full, 8 + 4 * 4)[0]
    size = 32768 + pad(loff0[0] - 32768)
    mf = ggmlfile.read(path)
    first_rows = None
    for l in range(L):
        lo = struct.unpack_from(f"<{L_COUNT}Q", full, OFF_GOFF + 8 * G_COUNT + 8 * L_COUNT * l)
        size += pad(lo[L_MAT0 + A_W] - lo[0])
    rows_at = size
    for l in range(L):
        for names in kc.MATRIX_NAMES.values():
            raw = b"".join(np.ascontiguousarray(mf.t(f"layers.{l}.{n}").data).tobytes() for n in names)
            first_rows = first_rows or raw
            size += pad(len(raw))
    assert size == len(comp)
    assert comp[rows_at:rows_at + len(first_rows)] == first_rows   # layer 0's q | k | v rows first
    head = bytearray(comp[:32768])
    for mutate in (lambda h: struct.pack_into("<Q", h, OFF_GOFF + 8 * G_COUNT + 8 * (L_MAT0 + A_WEXT), 7),   # a moved offset
                   lambda h: struct.pack_into("<Q", h, OFF_GOFF + 8 * G_COUNT + 8 * (L_MAT0 + A_DX), 0),
                   lambda h: struct.pack_into("<Q", h, OFF_TOTAL, len(full) + 256),
                   lambda h: struct.pack_into("<i", h, 52, 12 if wt == "q6_k" else 14)):   # another type's layout
        bad = bytearray(head)
        mutate(bad)
        with pytest.raises(q2a.Q2AError, match="not a q2a weight blob"):
            q2a.blob_device_size(bad)


def test_existing_types_blobs_are_byte_identical(make_model, golden_kq):
    """The F16 and Q4_K blobs of the tiny model (device layout, compact form, bf16 contract) have the SHA-256 recorded
    on the commit before Q5_K / Q6_K support: adding the types moved no byte of an existing type's blob."""
    import q2a
    want = golden_kq[0]["parent_blobs"]
    for wt in ("f16", "q4_k"):
        path = make_model("tiny", wt)
        assert hashlib.sha256(bytes(q2a.pack_model(path))).hexdigest() == want[wt]
        assert hashlib.sha256(bytes(q2a.pack_model(path, compact=True))).hexdigest() == want[f"{wt}_compact"]
        assert hashlib.sha256(bytes(q2a.pack_model(path, q2a.ACT_BF16))).hexdigest() == want[f"{wt}_bf16"]


# ---------------------------------------------------------------- no device
@pytest.mark.parametrize("wt", TYPES)
def test_open_fails_like_an_f16_file_without_a_device(make_model, wt):
    """Where there is no HIP device, opening a Q5_K / Q6_K file fails with the error an F16 file gets, not with
    'unsupported ftype'; where there is one, both open."""
    import q2a
    L = q2a.lib()

    def try_open(path):
        h = L.q2a_open(path.encode(), 0)
        if h:
            L.q2a_close(h)
            return None
        return L.q2a_last_error().decode()

    e16, eq = try_open(make_model("tiny", "f16")), try_open(make_model("tiny", wt))
    assert (e16 is None) == (eq is None), (e16, eq)
    if eq is not None:
        assert eq == e16 and "unsupported ftype" not in eq
