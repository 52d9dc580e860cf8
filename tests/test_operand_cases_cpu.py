"""The operand test inputs (tests/operand_cases.py) hit what they claim — proven on the CPU against the oracle before any
GPU sees them: tie counts and the rounding rule they separate, end codes and block sums, the order-independence of the
lattice rows, the GELU pattern coverage, and the layout decoders."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import operand_cases as oc


@pytest.fixture(scope="module", autouse=True)
def _oracle(host_build):
    return True


def half_away(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


def test_q8k_tie_blocks_separate_the_rounding_rule_and_the_first_maximum():
    x = oc.tie_rows_q8k(8, 512)
    qs, d, _ = oc.ref_q8k(x)
    blocks, codes = x.reshape(-1, 256), qs.reshape(-1, 256)
    seen = set()
    for i, (b, q) in enumerate(zip(blocks, codes)):
        p, p2 = oc.TIE_POSITIONS[i % 4]
        first = b[p]
        assert abs(first) == 127 and b[p2] == -first and np.abs(b).argmax() == p   # first occurrence of the maximum
        iscale = np.float32(-127.0) / first
        assert abs(iscale) == 1 and d.reshape(-1)[i] == 1 / iscale
        v = (iscale * b).astype(np.float64)
        ties = np.abs(v - np.trunc(v)) == 0.5
        assert ties.sum() >= 200 and ties.sum() == 254
        assert np.array_equal(q, np.rint(v).astype(np.int32))          # round half to even
        assert not np.array_equal(q, half_away(v))
        assert (q[ties] != half_away(v)[ties]).sum() >= 100
        assert q[p] == -127 and q[p2] == 127                           # a last-maximum scan would negate every code
        seen.add((i % 4, float(first)))
    assert len(seen) == 8                                               # every position with either sign


def test_q80_tie_blocks():
    x = oc.tie_rows_q80(5, 1024)
    qs, d, dbits = oc.ref_q80(x)
    assert (dbits == 0x3C00).all() and (np.abs(x.reshape(-1, 32)).max(axis=1) == 127).all()
    v = x.astype(np.float64)
    ties = np.abs(v - np.trunc(v)) == 0.5
    assert (ties.reshape(-1, 256).sum(axis=1) >= 200).all()
    assert np.array_equal(qs, np.rint(v).astype(np.int32)) and not np.array_equal(qs, half_away(v))
    assert {127, -127} <= set(qs.reshape(-1).tolist())


def test_gelu_tie_rows():
    xh = oc.gelu_tie_rows(5, 1024)
    y = oc.gelu_ref(xh)
    assert np.array_equal(y, xh.astype(np.float32)) and y.min() >= 10     # the x >= 10 branch: unchanged
    qs, d, _ = oc.ref_q8k(y)
    assert (d == -1).all()
    v = -y.astype(np.float64)
    ties = np.abs(v - np.trunc(v)) == 0.5
    assert (ties.reshape(-1, 256).sum(axis=1) >= 200).all()
    assert np.array_equal(qs, np.rint(v).astype(np.int32)) and not np.array_equal(qs, half_away(v))


def test_gelu_sign_rows():
    xh = oc.gelu_sign_rows(8, 512)
    y = oc.gelu_ref(xh).reshape(-1, 256)
    qs, d, _ = oc.ref_q8k(y.reshape(8, 512))
    signs = set()
    for i, (b, q, dd) in enumerate(zip(y, qs.reshape(-1, 256), d.reshape(-1))):
        p, p2 = oc.TIE_POSITIONS[i % 4]
        assert b[p] == -b[p2] != 0 and np.abs(b).argmax() == p and (np.abs(np.delete(b, [p, p2])) < abs(b[p])).all()
        assert q[p] == -127 and q[p2] == 127 and np.sign(dd) == -np.sign(b[p])   # the FIRST maximum sets the sign
        signs.add((i % 4, float(np.sign(b[p]))))
    assert len(signs) == 8


@pytest.mark.parametrize("half", [False, True])
def test_edge_blocks_reach_the_end_codes(half):
    M, K = 7, 1792      # 7 blocks per row: every variant in every row, rotating
    x = oc.edge_rows(M, K, half=half).astype(np.float32)
    nb = K // 256
    qs, d, bs32 = oc.ref_q8k(x)
    q0, d0, d0bits = oc.ref_q80(x)
    qs, q0 = qs.reshape(M, nb, 256), q0.reshape(M, nb, 256)
    d0bits = d0bits.reshape(M, nb, 8)
    seen = set()
    for m in range(M):
        for b in range(nb):
            name = oc.edge_variant(m, b, nb)
            seen.add(name)
            if name == "const":
                assert (qs[m, b] == -127).all() and (bs32[m, b] == -4064).all()
                hi = bs32[m, b] // 64
                assert (hi == -64).all() and (bs32[m, b] - 64 * hi == 32).all()
                assert (q0[m, b] == 127).all()
            elif name == "one_then_minus":
                assert qs[m, b, 0] == -127 and (qs[m, b, 1:] == 127).all()
                assert bs32[m, b, 0] == 3810 and (bs32[m, b, 1:] == 4064).all()
            elif name == "zero":
                assert (qs[m, b] == 0).all() and d[m, b] == 0 and (bs32[m, b] == 0).all()
                assert (q0[m, b] == 0).all() and (d0bits[m, b] == 0).all()
                assert np.signbit(x[m, b * 256:(b + 1) * 256]).any()
            elif name == "tiny_only":
                assert qs[m, b, 77] == -127 and np.count_nonzero(qs[m, b]) == 1 and np.isfinite(d[m, b]) and d[m, b] != 0
            elif name == "amax_1e-5":
                assert (d0bits[m, b] == 0x0001).all()          # one fp16 subnormal ulp
                assert np.abs(q0[m, b]).max() == 127
            elif name == "amax_6e6":
                assert ((d0bits[m, b] >= (0x5800 if half else 0x7800)) & (d0bits[m, b] < 0x7C00)).all()
                assert np.abs(q0[m, b]).max() == 127
    assert seen == set(oc.EDGE_VARIANTS)
    assert (oc.edge_rows(9, 512)[3] == 0).all() and (oc.edge_rows(9, 512)[8] == 0).all()   # all-zero rows


@pytest.mark.parametrize("D", [256, 1024, 1280])
def test_lattice_rows_are_order_independent(D):
    M = 6
    x = oc.lattice_rows(M, D)
    g, b = oc.affine(D)
    assert (g < 0).any() and (g == 0).any()
    y, mean, var = oc.ln_ref(x, g, b, return_stats=True)
    rng = np.random.default_rng(1)
    for _ in range(5):
        p = rng.permutation(D)
        # sequential (cumsum), numpy's pairwise and a reversed order: the same bits
        _, m2, v2 = oc.ln_ref(x[:, p], g[p], b[p], return_stats=True)
        assert np.array_equal(mean.view(np.uint32), m2.view(np.uint32)) and np.array_equal(var.view(np.uint32), v2.view(np.uint32))
        seq = np.cumsum(x[:, p].astype(np.float64), axis=1)[:, -1]
        assert np.array_equal((seq / D).astype(np.float32), mean)
    for m in range(M):
        k = [int(v) for v in np.rint(x[m].astype(np.float64) * 64)]
        assert sum(k) % (D // 4) == 0 and max(abs(v) for v in k) <= 4096
        exact_mean = Fraction(sum(k), 64 * D)
        assert Fraction(float(mean[m])) == exact_mean                      # the f32 mean is the exact mean
        v = x[m] - mean[m]
        assert all(Fraction(float(a)) == Fraction(kk, 64) - exact_mean for a, kk in zip(v[:32], k[:32]))   # exact centring
        sq = (v * v).astype(np.float64)
        exact_s2 = sum(Fraction(float(s)) for s in sq)
        assert exact_s2 < 2 ** 25 and all((Fraction(float(s)) * 2 ** 16).denominator == 1 for s in sq)
        assert Fraction(float(sq.sum())) == exact_s2 and Fraction(float(np.cumsum(sq[::-1])[-1])) == exact_s2
    assert np.array_equal(y[2], b)                                         # constant row: variance 0, output = bias
    assert var[2] == 0


def test_realistic_rows_have_outliers_and_an_offset():
    x = oc.realistic_rows(13, 256)
    assert abs(float(np.median(x)) - 30) < 1 and np.abs(x - 30).max() > 200


def test_gelu_patterns_cover_every_finite_half_and_minus_inf():
    pool = oc.gelu_pattern_pool()
    assert pool.shape == (249, 256)
    want = set(range(0x7C00)) | {v | 0x8000 for v in range(0x7C00)} | {0xFC00}
    assert set(pool.reshape(-1).tolist()) == want
    rows = oc.gelu_pattern_rows(63, 1024)                                   # 252 blocks: the whole pool
    assert set(rows.reshape(-1).tolist()) == want
    # magnitudes within a block stay close: the codes spread instead of collapsing under one huge maximum
    mag = (pool & 0x7FFF).astype(np.int32)
    assert ((mag.max(axis=1) - mag.min(axis=1))[:-1] <= 128).all()
    g = oc.gelu_values()
    xs = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    fin = np.isfinite(xs)
    assert (g[fin & (xs >= 10)] == xs[fin & (xs >= 10)]).all() and (g[xs <= -10] == 0).all() and g[0xFC00] == 0
    mid = np.abs(xs) < 10
    assert np.array_equal(g[mid].astype(np.float16).astype(np.float32), g[mid])   # fp16-valued between the branches
    qs, d, _ = oc.ref_q8k(oc.gelu_ref(rows))
    assert np.isfinite(d).all() and len(np.unique(qs)) >= 200 and {-127, 0, 127} <= set(np.unique(qs).tolist())


def test_engine_gelu_table_is_the_reference_table():
    """q2a_make_gelu_table (what the engine uploads, and the GELU + Q8_K kernel stages in LDS) against oracle_gelu +
    oracle_fp32_to_fp16 wherever ggml_vec_gelu_f32 reads the table (|x| < 10)."""
    import q2a
    tab = np.zeros(65536, np.uint16)
    q2a._host().q2a_make_gelu_table(C.c_void_p(tab.ctypes.data))
    ref = oc.gelu_table_bits()
    xs = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    mid = np.abs(xs) < 10
    assert np.array_equal(tab[mid], ref[mid])


def test_casts_and_decoders():
    import torch
    rng = np.random.default_rng(3)
    y = (rng.standard_normal(4096) * np.exp(rng.uniform(-8, 8, 4096))).astype(np.float32)
    y[:4] = [0.0, -0.0, 1.00390625, 1.01171875]                             # bf16 ties: to even both ways
    want = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(oc.bf16_bits(y), want)
    s = oc.split_bits(y.reshape(4, 1024))
    hi, lo = s[:, :1024].view(np.float16), s[:, 1024:2048].view(np.float16)
    assert np.array_equal(s[:, 2048:], s[:, :1024])
    ok = np.abs(y) < 6e4
    assert np.abs((hi.astype(np.float64) + lo.astype(np.float64)).reshape(-1) - y)[ok].max() <= 2.0 ** -22 * np.abs(y[ok]).max()
    o = oc.ordered16(np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0x3C01], np.uint16))
    assert o.tolist() == [0, 0, 1, -1, 0x3C00, 0x3C01]
    # layouts: d[bf * ld + m], (hi, lo) pairs, codes as halves
    M, nb, ld = 3, 2, 5
    dy = np.full((nb, ld), np.float32(7))
    aext = np.full((nb, ld, 16), np.float16(9))
    for m in range(M):
        for bf in range(nb):
            dy[bf, m] = 10 * m + bf
            aext[bf, m, 0::2] = -m - bf
            aext[bf, m, 1::2] = np.arange(8) + m
    assert oc.decode_d(dy, M).tolist() == [[0, 1], [10, 11], [20, 21]]
    hi, lo = oc.decode_bsum(aext.view(np.uint16), M)
    assert hi.shape == (M, nb, 8) and hi[2, 1].tolist() == [-3] * 8 and lo[1, 0].tolist() == list(range(1, 9))
    assert oc.decode_codes(np.array([-127, 0, 5], np.float16).view(np.uint16)).tolist() == [-127, 0, 5]
    with pytest.raises(AssertionError):
        oc.decode_codes(np.array([0.5], np.float16).view(np.uint16))
