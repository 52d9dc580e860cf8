"""Cases and plain-numpy statements for the log-mel entry points (q2a_encode_device_mel and friends), shared by
tests/test_mel_input_cpu.py (no GPU) and tests/test_gpu_mel_input.py.

The caller's mel is [n_mels][ld] f32, already normalised, with n_len <= ld frames. The encoder window of a clip is
frames seek .. seek + 2 n_ctx - 1; window frames at or past n_len are ZEROS (the reference clears the window and copies
what exists, qwen2-whisper.cpp:2264-2286), and nothing at or past frame n_len of a row is read."""
import numpy as np

N_CTX = 1500
TM = 2 * N_CTX   # mel frames of one encoder window


def mel_window(mel, n_len, seek, n_ctx=N_CTX):
    """The window rule, stated frame by frame: window[:, t] = mel[:, seek + t] if seek + t < n_len else 0."""
    mel = np.asarray(mel, dtype=np.float32)
    win = np.zeros((mel.shape[0], 2 * n_ctx), dtype=np.float32)
    for t in range(2 * n_ctx):
        if seek + t < n_len:
            win[:, t] = mel[:, seek + t]
    return win


def valid_lengths(n_len, seek, n_ctx=N_CTX):
    """(enc_len, out_len) as include/q2a_encoder.h states q2a_mel_valid_lengths."""
    frames = min(max(n_len - seek, 1), 2 * n_ctx)
    enc = (frames - 1) // 2 + 1
    return enc, enc // 2


def hf_lengths(n_frames):
    """transformers' Qwen2AudioEncoder._get_feat_extract_output_lengths: (encoder positions, output vectors)."""
    enc = (n_frames - 1) // 2 + 1
    return enc, (enc - 2) // 2 + 1


# (n_len, seek) of the zeros-and-bounds test: every n_len the issue names, with seeks that put the clip's last frame one
# short of, on and one past a 64-frame tile edge of the window, a clip that ends inside the last (56-frame) tile, a full
# window, and a window that starts behind the clip's last frame (all zeros)
EDGE_CLIPS = [(1, 0), (63, 0), (64, 0), (65, 0), (777, 100), (777, 713), (777, 712), (777, 714), (2999, 7), (2999, 0),
              (3000, 0), (3000, 2937), (65, 70)]
# ragged n_len / seek of the window-rule test against the oracle's mel_window (seek past the end: clamped, all zeros)
RAGGED = [(3000, 0), (777, 100), (50, 0), (4000, 1001), (4000, 3999), (10, 10), (10, 25), (3001, 1)]


def layout(n_lens, n_mels, ld):
    """Floats of the smallest buffer that holds len(n_lens) clips [n_mels][ld] at stride n_mels * ld when the last
    clip's last row ends with its frame n_len - 1: the buffer ends where the last readable float does."""
    stride = n_mels * ld
    return stride, (len(n_lens) - 1) * stride + (n_mels - 1) * ld + n_lens[-1]


def poisoned(mels, n_lens, ld, fill=np.nan):
    """One flat f32 buffer (layout above) with clip c's frames 0 .. n_len[c]-1 from mels[c] and `fill` in every frame
    at or past n_len[c] of every row."""
    n_mels = mels[0].shape[0]
    stride, total = layout(n_lens, n_mels, ld)
    buf = np.full(len(n_lens) * stride, fill, dtype=np.float32)
    for c, (m, n) in enumerate(zip(mels, n_lens)):
        rows = buf[c * stride:(c + 1) * stride].reshape(n_mels, ld)
        rows[:, :n] = m[:, :n]
    return buf[:total].copy()
