"""The packer under Q2A_ACT_MXFP8 (no GPU needed): every linear weight is ggml's dequantize_row_* value
MX-quantized on the host, e4m3 bytes [N][K] in the W slot, e8m0 scale codes [N][K/32] in the DX slot. Layer 0's four
matrices against the numpy rule; q_proj row 0 carries an all-zero block and a block whose maximum scales into (448, 512)."""
import ctypes as C
import hashlib
import shutil
import struct

import numpy as np

import q2a
from mxfp8_cases import mx_quant
from q2a import ggmlfile
from test_pack_cpu import A_COUNT, A_DX, A_W, L_MAT0, dequant_q8_0, header


def test_mxfp8_blob_holds_mx_quantized_weights(make_model, tmp_path):
    src, path = make_model("tiny", "q8_0"), str(tmp_path / "tiny-q8_0-edges.bin")
    shutil.copyfile(src, path)
    with open(path, "r+b") as f:
        f.seek(ggmlfile.read(src).t("layers.0.self_attn.q_proj.weight").offset)
        f.write(struct.pack("<e32b", 0.0, *([0] * 32)))                  # block 0: all zero -> code 127, zero bytes
        f.write(struct.pack("<e32b", 1.0, 127, -127, *range(-15, 15)))   # block 1: 127 * 2^2 = 508 -> saturates at 448
    blob = q2a.pack_model(path, q2a.ACT_MXFP8)
    wt, blk, act, total, loff0 = header(blob)
    assert (wt, blk, act, total) == (8, 0, q2a.ACT_MXFP8, len(blob))
    mf = ggmlfile.read(path)
    mats = [["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"], ["self_attn.out_proj"], ["fc1"], ["fc2"]]
    for w, names in enumerate(mats):
        deq = np.concatenate([dequant_q8_0(mf.t(f"layers.0.{n}.weight")) for n in names])
        N, K = deq.shape
        want8, wantsc = mx_quant(deq)
        a = loff0[L_MAT0 + w * A_COUNT:]
        got8 = np.frombuffer(blob, dtype=np.uint8, count=N * K, offset=a[A_W]).reshape(N, K)
        gotsc = np.frombuffer(blob, dtype=np.uint8, count=N * K // 32, offset=a[A_DX]).reshape(N, K // 32)
        assert np.array_equal(gotsc, wantsc) and np.array_equal(got8, want8), names
        if w == 0:
            assert gotsc[0, 0] == 127 and not got8[0, :32].any() and gotsc[0, 1] == 125 and got8[0, 32] == 0x7E and got8[0, 33] == 0xFE


def test_other_contracts_blobs_unchanged_and_compact_refused(make_model):
    """Packing act 0 and act 1 around an act 2 pack gives the same bytes: no state crosses the calls (that their layout is
    the parent's is what test_pack_cpu.py's layout tests hold). The compact form of act 2: Q2A_ERR_UNSUPPORTED, no blob."""
    path = make_model("tiny", "q8_0")
    for act in (q2a.ACT_REFERENCE, q2a.ACT_BF16):
        first = q2a.pack_model(path, act)
        q2a.pack_model(path, q2a.ACT_MXFP8)
        assert hashlib.sha256(q2a.pack_model(path, act)).digest() == hashlib.sha256(first).digest() and header(first)[2] == act
    p = C.c_void_p()
    assert q2a.lib().q2a_pack_model_compact(path.encode(), q2a.ACT_MXFP8, C.byref(p)) == -6 and not p.value
