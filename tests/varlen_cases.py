"""Inputs shared by tests/test_varlen_cpu.py and tests/test_gpu_varlen.py: a clip whose padded queries alone re-base
the last partly valid 16-query block of the attention kernel (the reason the packed layout of the variable-length
encode carries whole 16-row blocks; include/q2a_encoder.h, q2a_varlen_rows)."""
import numpy as np

from attn_model import H, STEP, STEPS_ALIGNED, _stair_head, clip_of

KEY_LEN = 1481                      # 9 valid rows (1472 .. 1480) and 7 padded ones (1481 .. 1487) in block 92
BLOCK = KEY_LEN // 16               # 92
VALID = slice(BLOCK * 16, KEY_LEN)              # rows 1472 .. 1480
PADDED = slice(KEY_LEN, (BLOCK + 1) * 16)       # rows 1481 .. 1487


def rebase_heads():
    """The stair-up heads (k[:, 0] climbs 13 nats at keys 32, 64, 736, 1440, 1472: a query with q[:, 0] = 1 re-bases at
    each stair) with q[:, 0] = 0 on the valid rows of the last block — they see noise only — and 1 on its padded rows."""
    heads = []
    for h in range(H):
        q, k, v = _stair_head(300 + h, STEPS_ALIGNED, STEP)
        q[VALID, 0] = 0.0
        assert (q[PADDED, 0] == 1.0).all()
        heads.append((q, k, v))
    return heads


def quiet_padding(q):
    """q with the block's padded query rows replaced by copies of its last valid row: nothing in the block re-bases."""
    q = np.array(q, copy=True)
    q[PADDED] = q[KEY_LEN - 1]
    return q


def rebase_clip():
    """(q, k, v) [T][H * 64] of the clip, the layout the attention hooks take."""
    return clip_of(rebase_heads())
