"""Key lengths under the bf16-activation contract (q2a_set_bf16_key_lengths): the attention's key-length and packed forms
against float64 and the plain kernel's bits, the block, the entry points. Tiny model, Q8_0 weights; needs an MI355X."""
import numpy as np
import pytest
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import q2a  # noqa: E402
T, D, H = 1500, 256, 4
pack = lambda x, rs: torch.cat([x[c * T:c * T + rs[c + 1] - rs[c]] for c in range(len(rs) - 1)]).contiguous()  # noqa: E731


@pytest.fixture(scope="module")
def eng(make_model):
    e = q2a.Engine(make_model("tiny", "q8_0"), device=0, act=q2a.ACT_BF16, bf16_key_lengths=True)
    yield e
    e.close()


def qkv(n_clips, seed):   # bf16-representable q ~ N(0,1)/8 and k, v ~ N(0,1), windows [n_clips*T][D] f32
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n_clips * T, D, generator=g).bfloat16().float().cuda() for _ in range(3))
    return q / 8, k, v


def attention(e, kind, q, k, v, lens):
    out = torch.zeros_like(q)
    e.test_attention_bf16(kind, q.data_ptr(), k.data_ptr(), v.data_ptr(), len(lens), lens, out.data_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("lens", [[1, 64, 65, 257, 1500], [63, 256, 255], [16]], ids=str)
def test_attention_matches_float64(eng, lens):
    """|out - ref| <= 2^-8 max|v|: the only rounding beyond f32 is P to bf16 (relative 2^-9) against an unrounded
    normaliser, so the error is <= 2^-9 sum(P|v|) / sum(P) <= 2^-9 max|v|; the factor 2 covers the f32 sums and exp2.
    K and V rows at or past a clip's key length are NaN: a key wrongly included poisons the row."""
    q, k, v = qkv(len(lens), 3 + len(lens))
    _, rs = q2a.varlen_rows(lens, T)
    qp, kp, vp = (pack(x, rs) for x in (q, k, v))
    for c, n in enumerate(lens):
        k[c * T + n:(c + 1) * T] = v[c * T + n:(c + 1) * T] = float("nan")
        kp[rs[c] + n:rs[c + 1]] = vp[rs[c] + n:rs[c + 1]] = float("nan")
    padded = attention(eng, q2a.ENCODE_PADDED, q, k, v, lens)
    packed = attention(eng, q2a.ENCODE_VARLEN, qp, kp, vp, lens)
    for c, n in enumerate(lens):
        rows = slice(c * T, c * T + n)
        qc, kc, vc = (x[rows].double().reshape(n, H, 64).transpose(0, 1) for x in (q, k, v))
        ref = (torch.softmax(qc @ kc.transpose(1, 2), -1) @ vc).transpose(0, 1).reshape(n, D)
        err, bound = (padded[rows].double() - ref).abs().max().item(), 2.0 ** -8 * v[rows].abs().max().item()
        print(f"clip {c} key_len {n}: max |out - ref| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (c, n, err, bound)   # (a NaN fails the comparison)
        assert torch.equal(packed[rs[c]:rs[c] + n], padded[rows]), (c, n)


@pytest.mark.parametrize("n_clips", [1, 3])
def test_full_key_length_is_the_plain_kernel(eng, n_clips):
    q, k, v = qkv(n_clips, 17)
    plain = attention(eng, q2a.ENCODE_PLAIN, q, k, v, [T] * n_clips)
    assert torch.isfinite(plain).all() and torch.equal(plain, attention(eng, q2a.ENCODE_PADDED, q, k, v, [T] * n_clips))


def block_input(n_clips):
    x0 = (np.random.default_rng(11).standard_normal((T, D)) * 0.5).astype(np.float32)
    return torch.from_numpy(np.tile(x0, (n_clips, 1))).cuda()


@pytest.mark.parametrize("n_clips", [1, 30])   # narrow tiles / the 8-phase QKV epilogue writing V rows
def test_block_full_key_length_is_the_plain_block(eng, n_clips):
    x, y, z = (block_input(n_clips) for _ in range(3))
    eng.test_block(0, x.data_ptr(), n_clips)
    eng.test_block_len(0, y.data_ptr(), n_clips, [T] * n_clips)
    eng.test_block(0, z.data_ptr(), n_clips)   # the plain block again, behind a call that wrote V rows
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.equal(x, y) and torch.equal(x, z)


def test_block_varlen_is_the_padded_block(eng):
    lens = [700, 16, 1500, 333]
    _, rs = q2a.varlen_rows(lens, T)
    x = block_input(len(lens))
    xp = pack(x, rs)
    eng.test_block_len(0, x.data_ptr(), len(lens), lens)
    eng.test_block_varlen(0, xp.data_ptr(), len(lens), lens)
    torch.cuda.synchronize()
    for c, n in enumerate(lens):
        assert torch.isfinite(xp[rs[c]:rs[c] + n]).all() and torch.equal(xp[rs[c]:rs[c] + n], x[c * T:c * T + n]), c


def test_entry_points_and_the_default(eng, make_clip):
    clips = [make_clip(0, 160000), make_clip(1, 8000), make_clip(2, 52345), make_clip(3, 480000)]   # 8000: under 1 s
    pcm, ns = torch.zeros(len(clips), 480000), [len(c) for c in clips]
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = torch.from_numpy(c)
    pcm = pcm.cuda()
    a, b = (torch.full((len(clips),) + eng.out_shape, 7.0, device="cuda") for _ in range(2))
    pl, pst = eng.encode_device_padded(pcm.data_ptr(), 480000, ns, a.data_ptr())
    vl, vst = eng.encode_device_varlen(pcm.data_ptr(), 480000, ns, b.data_ptr())
    torch.cuda.synchronize()
    assert list(pst) == list(vst) == [q2a.CLIP_ENCODED, q2a.CLIP_SKIPPED, q2a.CLIP_ENCODED, q2a.CLIP_ENCODED]
    assert list(pl) == list(vl) and pl[0] == 250 and pl[1] == 0 and pl[3] == eng.info.n_out
    assert torch.isfinite(a).all() and torch.equal(a, b) and a[0, :250].abs().max() > 0 and (a[0, 250:] == 0).all()
    eng.encode_device(pcm[3:].data_ptr(), 480000, [480000], b.data_ptr())   # a full 30 s clip: padded is plain
    torch.cuda.synchronize()
    assert torch.equal(a[3], b[0])
    mel = torch.from_numpy(np.stack([eng.pcm_to_mel(clips[i])[:, :3000] for i in (0, 2)])).cuda()   # log-mel input
    mask = (torch.arange(3000)[None] < torch.tensor([[1000], [327]])).long()
    (mv, lv), (mp, lp) = (eng.encode_features(mel, mask, kind=kd) for kd in ("varlen", "padded"))
    torch.cuda.synchronize()
    assert list(lv) == list(lp) == [250, 82] and torch.isfinite(mv).all() and torch.equal(mv, mp)
    eng.set_bf16_key_lengths(False)   # off, the default: the key-length kinds are refused
    with pytest.raises(q2a.Q2AError) as ei:
        eng.encode_host_varlen([clips[0]])
    eng.set_bf16_key_lengths(True)
    assert ei.value.rc == -6
