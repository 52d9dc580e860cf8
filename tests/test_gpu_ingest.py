"""Native-rate PCM ingestion on the GPU (q2a_ingest_device / _host, csrc/q2a_ingest.hip) against the float64
restatement of its value contract in tests/ingest_cases.py.

The bound of every output is the standard one of a T-term f32 FMA sum whose coefficients were rounded once to f32:
|y - y64| <= (T + 3) 2^-24 S[n], S[n] = sum |g x|. Largest |y - y64| / bound measured on an MI355X: see DESIGN.md §2d."""
import numpy as np
import pytest

import ingest_cases as ic

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_ARG, ERR_UNSUPPORTED = -4, -6
PAD = 8   # sentinel columns behind the longest clip


@pytest.fixture(scope="module")
def eng(make_model):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    e = q2a.Engine(make_model("tiny", "f16"), device=0)
    yield e
    e.close()


def dev(w):
    return torch.from_numpy(w).cuda()


def ingest_nan(eng, waves, rates, width=None):
    """Ingest into a NaN-filled destination; returns the rows as numpy and the lengths."""
    import q2a
    lens = [q2a.resampled_length(len(w), r) for w, r in zip(waves, rates)]
    out = torch.full((len(waves), (max(lens) + PAD) if width is None else width), float("nan"), device="cuda")
    y, ns = eng.ingest([dev(w) for w in waves], rates, out=out)
    torch.cuda.synchronize()
    assert list(ns) == lens
    return y.cpu().numpy(), lens


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fmt", ["s16", "f32"])
@pytest.mark.parametrize("rate", [8000, 11025, 22050, 44100, 48000])
def test_resampler_against_float64(eng, rate, fmt, channels):
    T = ic.plan(rate)[3]
    waves = [ic.wave(rate, n, fmt, channels, seed=rate + i) for i, n in enumerate(ic.clip_lengths(rate))]
    y, lens = ingest_nan(eng, waves, [rate] * len(waves))
    worst = 0.0
    for c, w in enumerate(waves):
        ref, S = ic.resample64(ic.source(w), rate)
        assert len(ref) == lens[c]
        assert np.isnan(y[c, lens[c]:]).all(), "samples behind n_out were written"
        got = y[c, :lens[c]].astype(np.float64)
        assert np.isfinite(got).all()
        bound = (T + 3) * 2.0 ** -24 * S
        worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
        assert (np.abs(got - ref) <= bound).all(), (c, int(np.argmax(np.abs(got - ref) - bound)))
    print(f"ingest {rate} {fmt} x{channels}: largest |y - y64| / bound = {worst:.3f}")


@pytest.mark.parametrize("channels", [1, 2])
def test_16k_is_the_read_wav_rule_bit_for_bit(eng, channels):
    waves = [ic.wave(16000, n, "s16", channels, seed=n) for n in (1, 1023, 5001)]
    y, lens = ingest_nan(eng, waves, [16000] * 3)
    for c, w in enumerate(waves):
        assert np.array_equal(y[c, :lens[c]].view(np.uint32), ic.source(w).view(np.uint32))
        assert np.isnan(y[c, lens[c]:]).all()


@pytest.fixture(scope="module")
def mixed():
    specs = [(48000, "s16", 2, 9000), (44100, "f32", 1, 30011), (16000, "s16", 1, 4000), (8000, "f32", 2, 1500)]
    return [ic.wave(r, n, f, ch, seed=r) for r, f, ch, n in specs], [s[0] for s in specs]


def test_batch_invariance(eng, mixed):
    waves, rates = mixed
    y, lens = ingest_nan(eng, waves, rates)
    for c, (w, r) in enumerate(zip(waves, rates)):
        alone, _ = ingest_nan(eng, [w], [r])
        assert np.array_equal(alone[0, :lens[c]].view(np.uint32), y[c, :lens[c]].view(np.uint32)), c


def test_host_call_equals_device_call(eng, mixed):
    waves, rates = mixed
    y, lens = ingest_nan(eng, waves, rates)
    for c, h in enumerate(eng.ingest_host(waves, rates)):
        assert np.array_equal(h.view(np.uint32), y[c, :lens[c]].view(np.uint32)), c


def test_ingest_feeds_encode_device(eng):
    import q2a
    waves = [ic.wave(44100, 88200, "s16", 2, seed=5), ic.wave(48000, 60000, "f32", 1, seed=6)]
    pcm, ns = eng.ingest([dev(w) for w in waves], [44100, 48000])
    out = torch.zeros((2,) + eng.out_shape, device="cuda")
    st = eng.encode_device(pcm.data_ptr(), pcm.shape[1], ns, out.data_ptr())
    torch.cuda.synchronize()
    host = pcm.cpu().numpy()
    ref, st_h = eng.encode_host([host[c, :ns[c]] for c in range(2)])
    assert list(st) == list(st_h) == [q2a.CLIP_ENCODED] * 2
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_q2a_main_encodes_a_44k_stereo_wav(eng, make_model, tmp_path):
    import os
    import subprocess
    import wave

    from conftest import PKG
    s16 = ic.wave(44100, 88200, "s16", 2, seed=9)
    with wave.open(str(tmp_path / "s.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(s16.tobytes())
    emb = tmp_path / "emb.f32"
    subprocess.run([os.path.join(PKG, "bin", "q2a_main"), "-m", make_model("tiny", "f16"), "-np", "-oemb", str(emb),
                    str(tmp_path / "s.wav")], check=True, timeout=120, capture_output=True)
    want, st = eng.encode_host(eng.ingest_host([s16], [44100]))
    assert st[0] == 0
    assert np.array_equal(np.fromfile(emb, dtype=np.float32).view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("rate,channels,width,rc", [(44101, 1, None, ERR_UNSUPPORTED), (48000, 3, None, ERR_ARG),
                                                     (48000, 1, 300, ERR_ARG)])
def test_refusals_write_nothing(eng, rate, channels, width, rc):
    import q2a
    w = np.zeros((1000, channels), np.float32) if channels > 1 else np.zeros(1000, np.float32)
    out = torch.full((2, width or 1200), float("nan"), device="cuda")
    good = np.zeros(100, np.float32)   # a valid clip in front: nothing of the call may run
    with pytest.raises(q2a.Q2AError) as e:
        eng.ingest([dev(good), dev(w)], [48000, rate], out=out)
    torch.cuda.synchronize()
    assert e.value.rc == rc
    assert torch.isnan(out).all()
