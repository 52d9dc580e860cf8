"""A numpy model of the reference-contract attention kernel's arithmetic, and the adversarial inputs built on it.

THE MODEL MIRRORS THE POLICY OF k_attn_t AS WRITTEN IN qwen2-audio-whisper-ggml_amd/csrc/q2a_attn.hip: the lazy
re-basing threshold PLIM and the P hi/lo split (lines 98-119), the per-query shift sh = max(mx, 0) and the rescale of
l and O (rebase, lines 373-393), and the per-tile order of the decision (iter, lines 447-495). Whoever changes that
policy changes model() with it: tests/test_attn_model_cpu.py proves on the CPU that the GPU cases of
tests/test_gpu_attention_edges.py drive the paths they name, and that proof is only as good as this mirror.

What is modelled (one head, [T][64] f32 operands, q NOT yet multiplied by log2 e — the hooks do that):
  * qs = f32(q * f32(log2 e)); every operand split as hi = fp16(x), lo = fp16(x - hi) (k_split_hilo);
  * S = f32(qh.kh^T + qh.kl^T + ql.kh^T), keys at or past key_len at -1e30;
  * per 16-query block m' = the per-query maximum of tile 0; per 32-key tile p = exp2(S - m'); the block re-bases when
    t > 0 and one lane's eight exponentials (keys 8g .. 8g+7 of the tile, one query) sum past PLIM: sh = max(tile max
    - m', 0) per query, l and o times exp2(-sh), m' += sh, p again against the new m';
  * l += sum p; ph = p truncated to fp16, pl = fp16(p - ph); o += ph.vl + pl.vh + ph.vh in f32; out = o / l.
What is not: the order of the f32 additions inside an MFMA and across lanes (the model rounds the running
sum after each 32-deep MFMA as the kernel's chain does, but treats the 32 products inside one as exact), and the
kernel's carrying S - m' as the MFMA accumulator's start value (the model's chain starts at 0). Measured, the kernel's
error is 0.3 - 2.3 times the model's on the same rows, 3.8 times on the 750-key cut staircase."""
import numpy as np

T = 1500
HD = 64                      # head dimension
KS = 32                      # keys per tile
QB = 16                      # queries per re-base decision
PLIM = np.float32(32768.0)
L2E = np.float32(1.4426950408889634)
NBLOCKS = (T + QB - 1) // QB

f32, f64, f16 = np.float32, np.float64, np.float16


def split_hilo(x):
    """x (f32) -> (hi, lo) fp16 with hi = fp16(x), lo = fp16(x - hi); both returned widened to float64."""
    x = np.asarray(x, dtype=f32)
    hi = x.astype(f16)
    lo = (x - hi.astype(f32)).astype(f16)
    return hi.astype(f64), lo.astype(f64)


def trunc_f16(p):
    """p (f32, >= 0 or +inf) rounded toward zero to fp16 (v_cvt_pkrtz_f16_f32); +inf stays +inf."""
    with np.errstate(over="ignore"):
        h = p.astype(f16)
    over = h.astype(f32) > p
    h[over] = np.nextafter(h[over], f16(0))
    return h


def block_rows(blocks, n=T):
    """Row indices of the given 16-query blocks (the last block of 1500 rows has 12)."""
    return np.concatenate([np.arange(b * QB, min((b + 1) * QB, n)) for b in blocks])


def model(q, k, v, key_len=T, blocks=None, _drop=None):
    """(out [T][64] f32 with NaN in the rows of blocks not evaluated, re-bases per evaluated block).

    _drop = "o" or "l" leaves that factor of the re-base out — a deliberately wrong copy for the self-check in
    tests/test_attn_model_cpu.py, never a description of the kernel."""
    q, k, v = (np.asarray(a, dtype=f32) for a in (q, k, v))
    n = q.shape[0]
    blocks = np.arange((n + QB - 1) // QB) if blocks is None else np.asarray(list(blocks))
    nb = len(blocks)
    # a block's 16 rows; past the last row the kernel loads row n - 1 again (the Q-row clamp), and so does the model
    rows = np.minimum(blocks[:, None] * QB + np.arange(QB)[None, :], n - 1)
    qh, ql = split_hilo((q[rows.reshape(-1)] * L2E).astype(f32))
    kh, kl = split_hilo(k[:key_len])
    vh, vl = split_hilo(v[:key_len])
    ntiles = (key_len + KS - 1) // KS
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        # the kernel's chain of MFMAs, one f32 rounding after each: two 32-deep halves of d, three terms each
        Sv = np.zeros((nb * QB, key_len), dtype=f32)
        for c in (slice(0, 32), slice(32, 64)):
            for a, b in ((qh, kh), (qh, kl), (ql, kh)):
                Sv = (Sv.astype(f64) + a[:, c] @ b[:, c].T).astype(f32)
        S = np.full((nb, QB, ntiles * KS), -1e30, dtype=f32)
        S[:, :, :key_len] = Sv.reshape(nb, QB, key_len)
        m = S[:, :, :KS].max(axis=2)
        l = np.zeros((nb, QB), dtype=f32)
        o = np.zeros((nb, QB, HD), dtype=f32)
        counts = np.zeros(nb, dtype=np.int64)
        for t in range(ntiles):
            St = S[:, :, t * KS:(t + 1) * KS]
            d = St - m[:, :, None]
            p = np.exp2(d)
            lane = p.reshape(nb, QB, KS // 8, 8).sum(axis=3, dtype=f32)
            rb = (lane > PLIM).any(axis=(1, 2)) if t > 0 else np.zeros(nb, dtype=bool)
            if rb.any():
                # per query; a block that does not re-base shifts by exactly 0 and keeps its exponentials
                sh = np.where(rb[:, None], np.maximum(d.max(axis=2), f32(0)), f32(0)).astype(f32)
                alpha = np.exp2(-sh)
                if _drop != "l":
                    l = l * alpha
                if _drop != "o":
                    o = o * alpha[:, :, None]
                m = m + sh
                p = np.where(rb[:, None, None], np.exp2(St - m[:, :, None]), p)
                counts += rb
            l = l + p.sum(axis=2, dtype=f32)
            ph16 = trunc_f16(p)
            pl = (p - ph16.astype(f32)).astype(f16).astype(f64)
            ph = ph16.astype(f64)
            k0, k1 = t * KS, min((t + 1) * KS, key_len)
            w = k1 - k0   # keys past key_len: p = 0 exactly, and V is not read there
            for a, b in ((ph, vl), (pl, vh), (ph, vh)):   # small terms first, one f32 rounding per MFMA
                o = (o.astype(f64) + a[:, :, :w] @ b[k0:k1]).astype(f32)
        res = o / l[:, :, None]
        out = np.full((n, HD), np.nan, dtype=f32)
        out[rows.reshape(-1)] = res.reshape(-1, HD)
    return out, [int(c) for c in counts]


def ref64(q, k, v, key_len=T):
    """float64 softmax attention of one head, keys at or past key_len at -inf -> [T][64] float64."""
    q, k, v = (np.asarray(a, dtype=f64) for a in (q, k, v))
    s = q @ k[:key_len].T
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    return (p @ v[:key_len]) / p.sum(axis=1, keepdims=True)


def rel_err(out, ref):
    """max-rel and rel-L2 as conftest.rel_errors defines them (without its log)."""
    d = np.asarray(out, dtype=f64) - np.asarray(ref, dtype=f64)
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.linalg.norm(d) / np.linalg.norm(ref))


# ---------------------------------------------------------------------------------------------------------------------
# The adversarial cases (tests/test_gpu_attention_edges.py runs them on the kernel, tests/test_attn_model_cpu.py proves
# here that they reach the paths they name). One case = one clip = H heads of [T][64]; levels are in nats.
H = 4
BASE_BAR = (2e-5, 5e-6)      # max-rel, rel-L2: the bar of test_attention_matches_fp32_reference
MARGIN = 4.0                 # bar = max(BASE_BAR, MARGIN x the model's own error on the case)
STEP = 13.0                  # nats per stair
STEPS_ALIGNED = (32, 64, 736, 1440, 1472)   # t = 1 and 2 (consecutive), mid-clip, the last whole tile, the 28-key tail
STEPS_MID = (40, 77, 750, 1471, 1499)       # a lane-group boundary, mid-group, one key before the last tile, the last key


def stair(steps, step):
    j = np.arange(T)
    lvl = np.zeros(T)
    for s in steps:
        lvl += step * (j >= s)
    return (lvl - 0.5 * (lvl.max() + lvl.min())).astype(f32)   # centred: max = -min


def _noise(seed, qs, ks):
    g = np.random.default_rng(seed)
    return ((g.standard_normal((T, HD)) * qs).astype(f32), (g.standard_normal((T, HD)) * ks).astype(f32),
            g.standard_normal((T, HD)).astype(f32))


def _stair_head(seed, steps, step, qmask=None):
    q, k, v = _noise(seed, 0.3, 0.3)
    q[:, 0] = 1.0 if qmask is None else qmask
    k[:, 0] = stair(steps, step)
    return q, k, v


def _spike_head(seed, pos):
    q, k, v = _noise(seed, 0.5, 1.5)
    q[:, 0] = 4.0
    k[:, 0] = 0.0
    k[pos, 0] = 40.0    # +160 nats = +230 log2 units: exp2 overflows before the re-base
    return q, k, v


def _uniform_head(seed):
    q, k, v = _noise(seed, 0.3, 0.3)
    q[:] = 0.0
    return q, k, v


def _base_head(seed, qs=1.0, ks=1.0, vs=1.0):
    q, k, v = _noise(seed, 0.5, 1.5)
    return (q * f32(qs)).astype(f32), (k * f32(ks)).astype(f32), (v * f32(vs)).astype(f32)


_rows = np.arange(T)
SPIKE_POS = (31, 33, 1471, 1499)

# name -> (head builder(head index) -> (q, k, v), key_len, expected re-bases: f(block, head) -> int or (lo, None))
CASES = {
    "stair_up_aligned": (lambda h: _stair_head(100 + h, STEPS_ALIGNED, STEP), T, lambda b, h: 5),
    "stair_up_mid": (lambda h: _stair_head(110 + h, STEPS_MID, STEP), T, lambda b, h: 5),
    "stair_down": (lambda h: _stair_head(120 + h, STEPS_ALIGNED, -STEP), T, lambda b, h: 0),
    "alt_blocks": (lambda h: _stair_head(130 + h, STEPS_ALIGNED, STEP, ((_rows // QB) % 2 == 0).astype(f32)), T,
                   lambda b, h: 0 if b % 2 else 5),
    "alt_rows": (lambda h: _stair_head(140 + h, STEPS_ALIGNED, STEP, (_rows % 2 == 0).astype(f32)), T, lambda b, h: 5),
    "spikes": (lambda h: _spike_head(150 + h, SPIKE_POS[h]), T, lambda b, h: 0 if SPIKE_POS[h] == 31 else (1, None)),
    "uniform_1500": (lambda h: _uniform_head(160 + h), 1500, lambda b, h: 0),
    "uniform_1473": (lambda h: _uniform_head(164 + h), 1473, lambda b, h: 0),
    "uniform_33": (lambda h: _uniform_head(168 + h), 33, lambda b, h: 0),
    "stair_cut_1471": (lambda h: _stair_head(170 + h, STEPS_ALIGNED, STEP), 1471, lambda b, h: 4),
    "stair_cut_750": (lambda h: _stair_head(174 + h, STEPS_ALIGNED, STEP), 750, lambda b, h: 3),
    "stair_cut_65": (lambda h: _stair_head(178 + h, STEPS_ALIGNED, STEP), 65, lambda b, h: 2),
}
# the scale window: baseline distribution with operands moved by powers of two; asserted inside
# 2^+-4, logged beyond
SCALES = {
    "v_m4": (dict(vs=2.0 ** -4), True), "q_m4_k_p4": (dict(qs=2.0 ** -4, ks=2.0 ** 4), True),
    "q_p4_k_m4": (dict(qs=2.0 ** 4, ks=2.0 ** -4), True),
    "v_m8": (dict(vs=2.0 ** -8), False), "q_m8_k_p8": (dict(qs=2.0 ** -8, ks=2.0 ** 8), False),
    "q_p8_k_m8": (dict(qs=2.0 ** 8, ks=2.0 ** -8), False),
    "v_m12": (dict(vs=2.0 ** -12), False), "q_m12_k_p12": (dict(qs=2.0 ** -12, ks=2.0 ** 12), False),
    "q_p12_k_m12": (dict(qs=2.0 ** 12, ks=2.0 ** -12), False),
}


def case_heads(name):
    """The H heads of a case: list of (q, k, v) [T][64] f32."""
    return [CASES[name][0](h) for h in range(H)]


def scale_heads(name):
    return [_base_head(200 + h, **SCALES[name][0]) for h in range(H)]


def clip_of(heads):
    """H heads of [T][64] -> the clip's (q, k, v) [T][H*64], the layout the hooks take."""
    return tuple(np.concatenate([hd[i] for hd in heads], axis=1) for i in range(3))


def sample_blocks(key_len=T):
    """First, middle and last of the 16-query blocks that hold a valid row (full length: 0, 47, 93 — an even block,
    an odd one, and the 12-query block)."""
    nb = (key_len + QB - 1) // QB
    return sorted({0, nb // 2, nb - 1})


def model_error(heads, key_len, head=0, blocks=None):
    """The model's own (max-rel, rel-L2) against float64 on one head and the sampled blocks, valid rows only."""
    q, k, v = heads[head]
    blocks = sample_blocks(key_len) if blocks is None else blocks
    out, _ = model(q, k, v, key_len, blocks)
    rows = block_rows(blocks)
    rows = rows[rows < key_len]
    return rel_err(out[rows], ref64(q, k, v, key_len)[rows])


def bar_of(model_err):
    """The case's bar: max(existing bar, MARGIN x the model's own error), per statistic."""
    return tuple(max(b, MARGIN * e) for b, e in zip(BASE_BAR, model_err))
