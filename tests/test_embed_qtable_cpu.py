"""q2a_dequantize_row (include/q2a_encoder.h), the host twin and value contract of the quantized embedding gather: bit for
bit float32(the float64 formula) decoded from the block bytes in numpy (tests/embed_q_cases.py), on quantizer output and
on hand-made end-code blocks. No GPU."""
import numpy as np
import pytest

import embed_q_cases as qc


@pytest.mark.parametrize("n_cols", [256, 512])
@pytest.mark.parametrize("name", list(qc.TYPES))
def test_dequantize_row_is_the_float64_formula(host_build, name, n_cols):
    import q2a
    t = qc.TYPES[name]
    rows, want = qc.rows(t, n_cols), qc.values(t, n_cols)
    assert rows.shape == (qc.N_QUANT + 16, q2a.quant_row_size(t, n_cols)) and np.isfinite(want).all()
    got = np.stack([q2a.dequantize_row(t, r, n_cols) for r in rows])
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, f"{name} {n_cols}: rows {bad[:8]} differ"
    # the end codes are in: a negative zero and the largest magnitudes
    assert (want.view(np.uint32) == 0x80000000).any() and np.abs(want).max() > 1e5


def test_dequantize_row_arguments(host_build):
    import q2a
    with pytest.raises(ValueError):
        q2a.dequantize_row(1, np.zeros(512, dtype=np.uint8), 256)       # F16 is no block type
    with pytest.raises(ValueError):
        q2a.dequantize_row(qc.Q6_K, np.zeros(209, dtype=np.uint8), 256)  # a short row
    assert q2a._host().q2a_dequantize_row(qc.Q4_K, None, None, 256) == -4
