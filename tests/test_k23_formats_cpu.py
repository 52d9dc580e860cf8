"""Q2_K / Q3_K model files on the host: the reader's integer view, the tool's quantizers and the blob packer, against
the reference-made fixture (tests/golden/golden_k23.*). No GPU."""
import os
import subprocess

import numpy as np
import pytest

import k23_cases as k23
import kquant_cases as kc
from conftest import GOLDEN_DIR, TOOL, _sha
from q2a import ggmlfile
from test_pack_cpu import A_COUNT, A_DX, A_W, L_MAT0, bf16_bits, header


@pytest.fixture(scope="module")
def fixture():
    return k23.load_golden_k23(GOLDEN_DIR)


@pytest.fixture(scope="module")
def ext_model(make_model, workdir, fixture):
    def make(wt):
        ext, path = os.path.join(workdir, "tinyext-f16.bin"), os.path.join(workdir, f"tinyext-{wt}.bin")
        if not os.path.exists(path):
            kc.write_ext_model(make_model("tiny", "f16"), ext)
            subprocess.check_call([TOOL, "quantize", ext, path, wt, "8"])
        return path
    return make


@pytest.mark.parametrize("wt", k23.TYPES)
def test_tool_quantizes_like_the_reference(make_model, ext_model, fixture, wt):
    """bin/q2a_tool's files hash to the reference-quantized ones, and the hand-made rows' bytes are the reference's."""
    meta, arr = fixture
    assert _sha(make_model("tiny", wt)) == meta["models"][f"tiny-{wt}"]["sha256"]
    assert _sha(ext_model(wt)) == meta["models"][f"tinyext-{wt}"]["sha256"]
    mf = ggmlfile.read(ext_model(wt))
    assert mf.wtype == k23.WT_TYPE[wt]
    for i, name in enumerate(kc.EXT_TENSORS):
        want = arr[f"ext_{wt}_{i}"]
        assert np.array_equal(mf.t(name).data[:want.size], want)


@pytest.mark.parametrize("wt", k23.TYPES)
def test_kq_decodes_the_reference_values(ext_model, fixture, wt):
    """Tensor.kq()'s integers give the reference's dequantize_row_* values of the hand-made rows bit for bit (as_f32), and
    those rows reach the cases the GPU tests are about."""
    mf = ggmlfile.read(ext_model(wt))
    seen = set()
    for i, name in enumerate(kc.EXT_TENSORS):
        t = mf.t(name)
        want = fixture[1][f"extdq_{wt}_{i}"]
        assert np.array_equal(t.as_f32()[:kc.EXT_ROWS].view(np.uint32), want.view(np.uint32))
        v = {k: a[:kc.EXT_ROWS] for k, a in t.kq().items()}
        q, sc = v["q"].reshape(kc.EXT_ROWS, -1, 16, 16), v["sc"][..., None]
        if wt == "q2_k":
            seen |= {"d0" for _ in [0] if ((v["d"] == 0) & (v["dmin"] != 0)).any()} | {"end" for _ in [0] if ((q == 3) & (sc == 15)).any()}
        else:
            seen |= {"d0" for _ in [0] if (v["d"] < 0).any()} | {"end" for _ in [0] if ((q == 0) & (sc == 0)).any()}
    assert seen == {"d0", "end"}


@pytest.mark.parametrize("wt", k23.TYPES)
def test_device_layout_holds_the_integer_operands(ext_model, wt):
    """Layer 0's fc2 (four 256-blocks) in the packed blob, Q4_K's sections: W' the scale-folded integers (zeros where
    d = 0, dx = 1 there), beta the block ratio; Q2_K wext = the sixteen mins, gamma = -(dmin / dx); Q3_K dmin, gamma and
    wext zeros. The bf16 contract's blob holds bf16(as_f32). The compact form carries the file's rows."""
    import q2a
    path = ext_model(wt)
    blob = q2a.pack_model(path)
    wtype, blk, act, total, loff0 = header(blob)
    assert (wtype, blk, act, total) == (k23.WT_TYPE[wt], 256, q2a.ACT_REFERENCE, len(blob))
    t = ggmlfile.read(path).t("layers.0.fc2.weight")
    v = k23.int_weights([t])
    N, K, nb = kc.D, kc.F, kc.F // 256
    a = loff0[L_MAT0 + 3 * A_COUNT:L_MAT0 + 4 * A_COUNT]
    arr = lambda i, dt, n: np.frombuffer(blob, dtype=dt, count=n, offset=a[i])  # noqa: E731
    deff = np.where(v["d"] != 0, v["d"], np.float32(1))
    assert np.array_equal(arr(A_W, np.float16, N * K).reshape(N, K).astype(np.float64), v["wint"] * np.repeat(v["d"] != 0, 256, axis=1))
    assert np.array_equal(arr(A_DX, np.float32, nb * N).reshape(nb, N).T, deff)
    prev = np.concatenate([np.ones((N, 1), np.float32), deff[:, :-1]], axis=1)
    assert np.array_equal(arr(4, np.float32, nb * N).reshape(nb, N).T, prev / deff)
    dmin, gamma, wext = arr(2, np.float32, nb * N).reshape(nb, N).T, arr(5, np.float32, nb * N).reshape(nb, N).T, arr(3, np.float16, nb * N * 16)
    if wt == "q2_k":
        assert np.array_equal(dmin, v["dmin"]) and np.array_equal(gamma, -(v["dmin"] / deff))
        assert np.array_equal(wext.reshape(nb, N, 16).astype(np.int64), v["m"].transpose(1, 0, 2))
        assert v["wint"].max() == 45
    else:
        assert not dmin.any() and not gamma.any() and not wext.any() and not np.signbit(gamma).any()
        assert v["wint"].max() == 128 and v["wint"].min() >= -124
    bblob = q2a.pack_model(path, q2a.ACT_BF16)
    ob = header(bblob)[4][L_MAT0 + 3 * A_COUNT + A_W]
    assert np.array_equal(np.frombuffer(bblob, dtype=np.uint16, count=N * K, offset=ob).reshape(N, K), bf16_bits(t.as_f32()))
    comp = q2a.pack_model(path, compact=True)
    assert q2a.blob_device_size(comp) == (len(blob), len(comp)) and bytes(np.ascontiguousarray(t.data)) in bytes(comp)
