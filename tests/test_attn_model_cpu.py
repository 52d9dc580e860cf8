"""The attention contract model (tests/attn_model.py) against float64, on the CPU: the adversarial cases of
tests/test_gpu_attention_edges.py reach the re-base paths they name, and an implementation that follows the kernel's
policy passes their bars — so a failure of a GPU case is the kernel's, not the case's."""
import numpy as np
import pytest

import attn_model as am


@pytest.fixture(scope="module")
def runs():
    """name -> per head (out, re-bases per block, blocks evaluated, float64 reference): head 0 on every block, the
    others on the sampled blocks (spikes: every head is its own position, all on every block)."""
    cache = {}

    def get(name):
        if name not in cache:
            _, key_len, _ = am.CASES[name]
            res = []
            for h, (q, k, v) in enumerate(am.case_heads(name)):
                blocks = list(range(am.NBLOCKS)) if h == 0 or name == "spikes" else am.sample_blocks(key_len)
                out, counts = am.model(q, k, v, key_len, blocks)
                res.append((out, counts, blocks, am.ref64(q, k, v, key_len)))
            cache[name] = res
        return cache[name]

    return get


def test_truncation_to_fp16_rounds_toward_zero():
    p = np.array([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24,
                  65504.0, 65519.0, 1e6, np.inf], dtype=np.float32)
    want = np.array([0.0, 1.0, 1.0, 1.0, 2.0 ** -24, 0.0, 2.0 ** -24, 65504.0, 65504.0, 65504.0, np.inf])
    assert np.array_equal(am.trunc_f16(p).astype(np.float64), want)
    g = np.random.default_rng(1)
    x = np.exp2(g.uniform(-30, 15, 4096)).astype(np.float32)
    h = am.trunc_f16(x).astype(np.float32)
    assert (h <= x).all() and (np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float32) > x).all()


def test_model_meets_the_existing_bar_on_the_existing_distribution():
    """q * 0.5, k * 1.5, seed 0, one head (test_attention_matches_fp32_reference's inputs): the kernel measured
    1.3e-6 / 5.7e-7 there; the bar is 2e-5 / 5e-6."""
    q, k, v = am._base_head(0)
    out, counts = am.model(q, k, v)
    mx, l2 = am.rel_err(out, am.ref64(q, k, v))
    print(f"baseline: model max-rel {mx:.3e} rel-L2 {l2:.3e}, re-bases per block {np.mean(counts):.2f}")
    assert mx < am.BASE_BAR[0] and l2 < am.BASE_BAR[1]
    # what the suite's other float64 comparisons exercise: about two re-bases per block, wherever the noise puts them
    assert 1.0 <= np.mean(counts) <= 3.0


@pytest.mark.parametrize("name", list(am.CASES))
def test_case_reaches_its_path_and_a_correct_kernel_passes(runs, name):
    _, key_len, expect = am.CASES[name]
    heads = am.case_heads(name)
    bar = am.bar_of(am.model_error(heads, key_len))   # as the GPU test computes it
    for h, (out, counts, blocks, ref) in enumerate(runs(name)):
        for b, c in zip(blocks, counts):
            if b * am.QB >= key_len:
                continue   # a block wholly in the padding: its output is not compared
            e = expect(b, h)
            if isinstance(e, tuple):
                assert c >= e[0], (name, h, b, c)
            else:
                assert c == e, (name, h, b, c)
        rows = am.block_rows(blocks)
        rows = rows[rows < key_len]
        assert np.isfinite(out[rows]).all(), (name, h)
        mx, l2 = am.rel_err(out[rows], ref[rows])
        print(f"{name} head {h}: model max-rel {mx:.3e} rel-L2 {l2:.3e} (bar {bar[0]:.2e} / {bar[1]:.2e})")
        # the model alone, every block of head 0 and the samples of the others, inside the bar the samples of head 0 set
        assert mx < bar[0] and l2 < bar[1], (name, h, mx, l2, bar)


def test_uniform_case_is_the_mean_of_v():
    for name, key_len in (("uniform_1500", 1500), ("uniform_1473", 1473), ("uniform_33", 33)):
        q, k, v = am.case_heads(name)[0]
        want = v[:key_len].astype(np.float64).mean(axis=0)
        assert np.allclose(am.ref64(q, k, v, key_len), want[None, :], rtol=0, atol=1e-13)


def test_spike_overflows_exp2_before_the_re_base():
    """The case's point: against the stale reference point the spike's exponential is +inf in f32."""
    q, k, v = am.case_heads("spikes")[1]   # position 33
    s = (q.astype(np.float64) * float(am.L2E)) @ k.astype(np.float64).T
    assert ((s[:, 33] - s[:, :32].max(axis=1)) > 128).all()


@pytest.mark.parametrize("name", ["stair_up_aligned", "stair_up_mid"])
@pytest.mark.parametrize("drop", ["o", "l"])
def test_model_without_a_rescale_is_far_off(name, drop):
    """Self-check of the model (not of the kernel): a copy whose re-base forgets o *= alpha or l *= alpha disagrees
    with float64 by orders of magnitude on the staircases, so these inputs tell a wrong re-base from a right one."""
    q, k, v = am.case_heads(name)[0]
    blocks = am.sample_blocks()
    rows = am.block_rows(blocks)
    ref = am.ref64(q, k, v)[rows]
    good = am.rel_err(am.model(q, k, v, blocks=blocks)[0][rows], ref)
    bad = am.rel_err(am.model(q, k, v, blocks=blocks, _drop=drop)[0][rows], ref)
    print(f"{name} without {drop} *= alpha: {bad[0]:.3e} / {bad[1]:.3e} (with: {good[0]:.3e} / {good[1]:.3e})")
    assert good[1] < am.BASE_BAR[1] * am.MARGIN
    assert bad[1] > 1e4 * good[1] and bad[1] > 0.1


@pytest.mark.parametrize("name", list(am.SCALES))
def test_scale_window_of_the_hi_lo_contract(name):
    """Inside 2^+-4 the split operands keep the F32-class bar; by 2^-12 (V) / 2^+-12 (Q against K) the lo halves have
    sunk under fp16's 2^-24 spacing and the model itself leaves it."""
    q, k, v = am.scale_heads(name)[0]
    blocks = am.sample_blocks()
    rows = am.block_rows(blocks)
    mx, l2 = am.rel_err(am.model(q, k, v, blocks=blocks)[0][rows], am.ref64(q, k, v)[rows])
    print(f"{name}: model max-rel {mx:.3e} rel-L2 {l2:.3e}")
    if am.SCALES[name][1]:
        assert mx < am.BASE_BAR[0] and l2 < am.BASE_BAR[1]
    elif name.endswith("12"):
        assert mx > am.BASE_BAR[0] and l2 > am.BASE_BAR[1]
