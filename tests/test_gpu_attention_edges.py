"""Adversarial parity of the reference-contract attention kernel (k_attn_t, q2a_attn.hip) through q2a_test_attention /
q2a_test_attention_len on the tiny F16 engine (D = 256, H = 4, T = 1500): inputs built so that the lazy re-base of the
softmax reference point runs where it can go wrong — in consecutive tiles, in the last whole tile and the 28-key tail,
after exp2 has overflowed, for some queries or one block of a wave only, never at all — each compared with float64.

The cases, their re-base counts and the bars come from tests/attn_model.py; tests/test_attn_model_cpu.py proves on the
CPU that every case reaches the path it names and that the model of a correct kernel passes it. Bar per case and
statistic: max(2e-5 / 5e-6, 4 x the model's own error against float64 on the case), never the kernel's own output.
Set Q2A_PARITY_LOG to collect the figures; DESIGN.md §2 has the measured table."""
import numpy as np
import pytest

import attn_model as am
from conftest import rel_errors

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, D, H = am.T, am.H * am.HD, am.H
NAMES = list(am.CASES)
LENS = [am.CASES[n][1] for n in NAMES]
LEN_CASES = [n for n in NAMES if n.startswith(("uniform", "stair_cut"))]   # these go through q2a_test_attention_len
SCALE_NAMES = list(am.SCALES)


@pytest.fixture(scope="module")
def engine(make_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    e = q2a.Engine(make_model("tiny", "f16"), device=0)
    yield e
    e.close()


def _attn(e, q, k, v, B, lens=None):
    out = torch.full_like(q, float("nan"))   # every row must be written by the kernel
    if lens is None:
        e.test_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, out.data_ptr())
    else:
        e.test_attention_len(q.data_ptr(), k.data_ptr(), v.data_ptr(), B, lens, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _query_tile(B):
    """Queries per workgroup of the launch (q2a_attn.hip launcher): 64 when the 128-query grid would not fill the CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 64 if ((T + 127) // 128) * H * B < cus else 128


def _batch(heads_of):
    clips = [am.clip_of(hd) for hd in heads_of]
    return tuple(torch.from_numpy(np.concatenate([c[i] for c in clips], axis=0)).cuda() for i in range(3))


def _ref_rows(q, k, v, c, L):
    """float64 softmax attention of clip c's queries < L with keys >= L at -inf -> [L][D] (float64, on the GPU)."""
    sl = slice(c * T, (c + 1) * T)
    qh = q[sl][:L].view(L, H, 64).permute(1, 0, 2).double()
    kh = k[sl].view(T, H, 64).permute(1, 0, 2).double()
    vh = v[sl].view(T, H, 64).permute(1, 0, 2).double()
    s = qh @ kh.transpose(-1, -2)
    s.masked_fill_(torch.arange(T, device=s.device) >= L, float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).permute(1, 0, 2).reshape(L, D)


@pytest.fixture(scope="module")
def cases(engine):
    """The one batch of all cases (12 clips, 128-query workgroups) and its three launches: the unmasked kernel, the
    key-length kernel at the cases' lengths, the key-length kernel with every length = T."""
    B = len(NAMES)
    assert B >= 6 and _query_tile(B) == 128 and _query_tile(1) == 64
    heads = {n: am.case_heads(n) for n in NAMES}
    q, k, v = _batch([heads[n] for n in NAMES])
    return {"heads": heads, "q": q, "k": k, "v": v, "plain": _attn(engine, q, k, v, B),
            "len": _attn(engine, q, k, v, B, LENS), "len_full": _attn(engine, q, k, v, B, [T] * B)}


def _case_out(cases, name):
    c, L = NAMES.index(name), am.CASES[name][1]
    out = cases["len" if name in LEN_CASES else "plain"]
    return c, L, out[c * T:c * T + L]


# ---------------------------------------------------------------- (a), (d): against float64, finite
@pytest.mark.parametrize("name", NAMES)
def test_case_matches_float64(cases, name):
    """(a) and (d). Measured on an MI355X, kernel (whole clip) | model (head 0, first / middle / last block), max-rel
    rel-L2: stair_up_aligned 3.8e-6 2.4e-6 | 2.3e-6 1.6e-6; stair_up_mid 3.7e-7 1.4e-7 | 2.7e-7 1.3e-7; stair_down
    5.3e-6 4.0e-6 | 2.2e-6 1.7e-6; alt_blocks 3.5e-6 2.4e-6 | 2.1e-6 1.8e-6; alt_rows 5.0e-6 2.6e-6 | 2.2e-6 1.9e-6;
    spikes 6.4e-8 5.3e-8 | 5.5e-8 2.8e-8; uniform <= 3.2e-7 2.4e-7 | 2.3e-7 1.7e-7; stair_cut_1471 3.3e-6 2.0e-6 |
    7.6e-7 8.0e-7; stair_cut_750 2.3e-6 1.7e-6 | 4.9e-7 4.8e-7; stair_cut_65 2.6e-7 9.0e-8 | 2.2e-7 7.8e-8."""
    c, L, got = _case_out(cases, name)
    q, k, v = cases["q"], cases["k"], cases["v"]
    assert torch.isfinite(got).all(), name
    if name.startswith("uniform"):   # the mean of V over exactly key_len keys
        ref = v[c * T:c * T + L].double().mean(dim=0, keepdim=True).expand(L, D)
    else:
        ref = _ref_rows(q, k, v, c, L)
    model_err = am.model_error(cases["heads"][name], L)
    bar = am.bar_of(model_err)
    mx, l2 = rel_errors(got.cpu().numpy(), ref.cpu().numpy())
    print(f"{name}: kernel max-rel {mx:.3e} rel-L2 {l2:.3e} | model {model_err[0]:.3e} {model_err[1]:.3e} | "
          f"bar {bar[0]:.2e} {bar[1]:.2e}")
    assert mx < bar[0] and l2 < bar[1], (name, mx, l2, bar)


# ---------------------------------------------------------------- (b): batch position / grid shape
@pytest.mark.parametrize("name", NAMES)
def test_case_batched_equals_single_clip_bits(engine, cases, name):
    """The batch runs 32 queries per wave (a re-basing block beside one that does not: alt_blocks), the clip alone 16."""
    c, L, wide = _case_out(cases, name)
    sl = slice(c * T, (c + 1) * T)
    q1, k1, v1 = (cases[x][sl].contiguous() for x in ("q", "k", "v"))
    one = _attn(engine, q1, k1, v1, 1, [L] if name in LEN_CASES else None)
    assert torch.isfinite(one[:L]).all(), name
    assert torch.equal(one[:L], wide), f"{name}: the batched launch differs from the one-clip launch"


# ---------------------------------------------------------------- (c): key_len = T == the unmasked kernel
def test_full_length_key_len_gives_the_unmasked_bits(cases):
    for c, name in enumerate(NAMES):
        sl = slice(c * T, (c + 1) * T)
        assert torch.isfinite(cases["plain"][sl]).all(), name
        assert torch.equal(cases["len_full"][sl], cases["plain"][sl]), name


# ---------------------------------------------------------------- padded keys are never read, with re-bases running
def test_len_cases_never_read_padded_keys(engine, cases):
    """Rows >= key_len of K and V hold NaN in a second run (as test_attention_len_never_reads_padded_keys): a re-base
    in the clip's last tile recomputes scores from K in LDS, whose rows past the length are the clamped last key's."""
    kn, vn = cases["k"].clone(), cases["v"].clone()
    for name in LEN_CASES:
        c, L = NAMES.index(name), am.CASES[name][1]
        kn[c * T + L:(c + 1) * T] = float("nan")
        vn[c * T + L:(c + 1) * T] = float("nan")
    dirty = _attn(engine, cases["q"], kn, vn, len(NAMES), LENS)
    for name in LEN_CASES:
        c, L, clean = _case_out(cases, name)
        got = dirty[c * T:c * T + L]
        assert torch.isfinite(got).all(), f"{name} read a padded key"
        assert torch.equal(got, clean), name
    for c, name in enumerate(NAMES):   # the full-length clips of the batch: untouched
        if name not in LEN_CASES:
            assert torch.equal(dirty[c * T:(c + 1) * T], cases["len"][c * T:(c + 1) * T]), name


# ---------------------------------------------------------------- the operand-scale window of the hi/lo contract
@pytest.fixture(scope="module")
def scales(engine):
    B = len(SCALE_NAMES)
    assert _query_tile(B) == 128
    q, k, v = _batch([am.scale_heads(n) for n in SCALE_NAMES])
    return q, k, v, _attn(engine, q, k, v, B)


@pytest.mark.parametrize("name", SCALE_NAMES)
def test_scale_window(scales, name):
    """Baseline distribution (q * 0.5, k * 1.5, v) with operands moved by powers of two. Inside 2^+-4 the F32-class bar
    2e-5 / 5e-6 is asserted; the 2^+-8 and 2^+-12 settings are measured and logged, not asserted: they show where the
    fp16 lo halves stop carrying bits (remainders under fp16's 2^-24 spacing) and the contract ends. Measured (MI355X,
    max-rel / rel-L2): 2^+-4 <= 2.9e-6 / 1.2e-6; V 2^-8 2.5e-6 / 4.5e-6, Q / K 2^+-8 up to 4.5e-5 / 1.7e-5; V 2^-12
    3.0e-5 / 7.1e-5, Q / K 2^+-12 up to 6.5e-4 / 2.6e-4. DESIGN.md §2."""
    q, k, v, out = scales
    c = SCALE_NAMES.index(name)
    got = out[c * T:(c + 1) * T]
    assert torch.isfinite(got).all(), name
    mx, l2 = rel_errors(got.cpu().numpy(), _ref_rows(q, k, v, c, T).cpu().numpy())
    asserted = am.SCALES[name][1]
    print(f"scale {name}: kernel max-rel {mx:.3e} rel-L2 {l2:.3e} ({'asserted' if asserted else 'logged only'})")
    if asserted:
        assert mx < am.BASE_BAR[0] and l2 < am.BASE_BAR[1], (name, mx, l2)
