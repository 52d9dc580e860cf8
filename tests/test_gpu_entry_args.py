"""Argument rejection of the encode and feature entry points: the return code of calls that are wrong in one or two ways,
and that a handle still computes the same bytes afterwards.

Every row is rejected before anything is launched or copied (the check that rejects it is named beside the row), so no
row reaches a kernel with a bad pointer. The expected codes are literals: what the checks return, in the order the
entry points make them — arguments, then the activation contract (the bf16-contract engine refuses the key-length
kinds), then the key lengths, then the sink's requirements, then encode()'s own checks (the feature checks before the
per-clip ranges). A two-fault row pins which of two checks comes first.

The entry points are the eighteen q2a_encode_* / q2a_audio_features_* / q2a_inputs_embeds_* calls and the two front-end
hooks. One engine, one bf16-contract engine (for its rows alone) and one projector per module; B = 2 on the tiny model.
Each family's valid call runs once before any rejected call (the reference bytes) and once after the family's rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import TOOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

AUDIO = 151646
D_OUT = 256
I32P = C.POINTER(C.c_int32)

PCM_DEV = ("q2a_encode_device", "q2a_encode_device_ex", "q2a_encode_device_padded", "q2a_encode_device_varlen",
           "q2a_audio_features_device", "q2a_audio_features_device_to", "q2a_inputs_embeds_device", "q2a_test_frontend")
MEL_DEV = ("q2a_encode_device_mel", "q2a_audio_features_device_mel", "q2a_audio_features_device_mel_to",
           "q2a_inputs_embeds_device_mel", "q2a_test_frontend_mel")
PCM_HOST = ("q2a_encode_host", "q2a_encode_host_ex", "q2a_encode_host_padded", "q2a_encode_host_varlen", "q2a_audio_features_host")
MEL_HOST = ("q2a_encode_host_mel", "q2a_audio_features_host_mel")
ALL = PCM_DEV + MEL_DEV + PCM_HOST + MEL_HOST
# the entry points that take key lengths (the log-mel encodes are called with kind ENCODE_VARLEN)
KEYLEN = tuple(n for n in ALL if n not in ("q2a_encode_device", "q2a_encode_device_ex", "q2a_encode_host", "q2a_encode_host_ex",
                                           "q2a_test_frontend", "q2a_test_frontend_mel"))
PACKED = ("q2a_audio_features_device", "q2a_audio_features_device_mel", "q2a_audio_features_host", "q2a_audio_features_host_mel")
TO = ("q2a_audio_features_device_to", "q2a_audio_features_device_mel_to")
IDS = ("q2a_inputs_embeds_device", "q2a_inputs_embeds_device_mel")
FAMILIES = {
    "encode_device": ("q2a_encode_device", "q2a_encode_device_ex", "q2a_encode_device_padded", "q2a_encode_device_varlen",
                      "q2a_encode_device_mel", "q2a_test_frontend", "q2a_test_frontend_mel"),
    "encode_host": ("q2a_encode_host", "q2a_encode_host_ex", "q2a_encode_host_padded", "q2a_encode_host_varlen", "q2a_encode_host_mel"),
    "features": ("q2a_audio_features_device", "q2a_audio_features_device_mel"),
    "features_to": TO,
    "inputs_embeds": IDS,
    "features_host": ("q2a_audio_features_host", "q2a_audio_features_host_mel"),
}
VALID = {"encode_device": "q2a_encode_device_varlen", "encode_host": "q2a_encode_host_mel", "features": "q2a_audio_features_device_mel",
         "features_to": "q2a_audio_features_device_to", "inputs_embeds": "q2a_inputs_embeds_device_mel",
         "features_host": "q2a_audio_features_host"}


def _i32(a):
    return None if a is None else a.ctypes.data_as(I32P)


def _vp(ptr):
    return C.c_void_p(ptr) if ptr else None


class Ctx:
    """The valid arguments of every entry point, by name; call(name, **over) replaces some and returns the code."""

    def __init__(self, eng, eng_bf16, proj):
        import q2a
        self.q2a, self.eng, self.eng_bf16, self.proj = q2a, eng, eng_bf16, proj
        i = eng.info
        self.T, self.M, self.D, self.TO = i.n_audio_ctx, i.n_mels, i.n_audio_state, i.n_out
        rng = np.random.default_rng(7)
        self.stride = 32000
        self.ns = np.array([32000, 24000], dtype=np.int32)
        self.pcm_host = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in self.ns]
        pcm = np.zeros((2, self.stride), dtype=np.float32)
        for c, x in enumerate(self.pcm_host):
            pcm[c, :len(x)] = x
        self.pcm = torch.from_numpy(pcm).cuda()
        self.ld = 2 * self.T
        self.nl = np.array([self.ld, self.ld - 10], dtype=np.int32)
        self.mel_host = [rng.uniform(-1, 1, size=(self.M, int(n))).astype(np.float32) for n in self.nl]
        mel = np.zeros((2, self.M, self.ld), dtype=np.float32)
        for c, x in enumerate(self.mel_host):
            mel[c, :, :x.shape[1]] = x
        self.mel = torch.from_numpy(mel).cuda()
        self.zeros2 = np.zeros(2, dtype=np.int32)
        # the defaulted key lengths, and with them the rows of the feature calls
        self.kl_pcm = np.array([q2a.valid_lengths(int(n), 0, self.T)[0] for n in self.ns], dtype=np.int32)
        self.kl_mel = np.array([q2a.mel_valid_lengths(int(n), 0, self.T)[0] for n in self.nl], dtype=np.int32)
        self.rows = {False: int((self.kl_pcm // 2).sum()), True: int((self.kl_mel // 2).sum())}
        cap = max(self.rows.values())
        self.out = torch.zeros((2, self.T, self.D), dtype=torch.float32, device="cuda")   # (the hooks write [B][T][D])
        self.out_host = np.zeros((2, self.TO, self.D), dtype=np.float32)
        self.feat = torch.zeros((cap, D_OUT), dtype=torch.float32, device="cuda")
        self.embd = torch.zeros((cap, self.D), dtype=torch.float32, device="cuda")
        self.feat_host = np.zeros((cap, D_OUT), dtype=np.float32)
        self.embd_host = np.zeros((cap, self.D), dtype=np.float32)
        self.n_tok = cap + 6
        self.dst_t = torch.zeros((self.n_tok, D_OUT), dtype=torch.bfloat16, device="cuda")
        self.dst = q2a.feat_dst(self.dst_t.data_ptr(), D_OUT, self.n_tok, q2a.DT_BF16)
        self.ids = {}
        for mel_in, rows in self.rows.items():   # the audio token exactly where the call's rows go
            ids = np.full(self.n_tok, 5, dtype=np.int32)
            ids[3:3 + rows] = AUDIO
            t = torch.from_numpy(ids).cuda()
            self.ids[mel_in] = (t, q2a.embeds_src(t.data_ptr(), 4, self.n_tok, AUDIO))
        self.ol = np.zeros(2, dtype=np.int32)
        self.st = np.zeros(2, dtype=np.int32)

    def argv(self, name, **o):
        mel, host = name in MEL_DEV + MEL_HOST, name in PCM_HOST + MEL_HOST
        g = lambda k, d: o[k] if k in o else d   # noqa: E731
        # (handles are Python ints: as c_void_p, or an entry point without ctypes prototypes would get 32 bits of them)
        e = g("e", self.eng)
        e = C.c_void_p(e.h) if e is not None else None
        p = g("p", self.proj)
        p = C.c_void_p(p.h) if p is not None else None
        n = C.c_int(g("n", 2))
        lens = _i32(g("lens", self.nl if mel else self.ns))
        second = _i32(g("second", None))           # offsets_ms / seek
        kl = _i32(g("kl", None))
        if host:
            src = self.mel_host if mel else self.pcm_host
            data = g("data", (C.c_void_p * 2)(*[x.ctypes.data for x in src]))
            out, feat, embd = _vp(self.out_host.ctypes.data), self.feat_host.ctypes.data, self.embd_host.ctypes.data
            head = [data, lens]
        else:
            data = _vp(g("data", (self.mel if mel else self.pcm).data_ptr()))
            out, feat, embd = _vp(self.out.data_ptr()), self.feat.data_ptr(), self.embd.data_ptr()
            head = [data, C.c_int64(g("stride", self.M * self.ld))] + [C.c_int64(g("ld", self.ld))] if mel else \
                   [data, C.c_int64(g("stride", self.stride))]
            head += [lens]
        cap = C.c_int64(g("cap", self.rows[mel]))
        ol, st, tail = _i32(self.ol), _i32(self.st), ([] if host else [None])   # stream: the default one
        kind = [C.c_int(self.q2a.ENCODE_VARLEN)] if name in ("q2a_encode_device_mel", "q2a_encode_host_mel") else []
        if name in ("q2a_encode_device", "q2a_encode_host"):
            return [e] + head + [n, C.c_int(g("offset_ms", 0)), out, st] + tail
        if name == "q2a_encode_device_ex":
            return [e] + head + [_i32(g("second", self.zeros2)), n, out, st] + tail
        if name == "q2a_encode_host_ex":
            return [e] + head + [second, n, C.c_int(g("offset_ms", 0)), out, st]
        if name in ("q2a_test_frontend", "q2a_test_frontend_mel"):
            return [e] + head + ([second] if mel else []) + [n, out] + tail
        if name.startswith("q2a_encode_"):
            return [e] + kind + head + [second, kl, n, out, ol, st] + tail
        if name in PACKED:
            sink = [_vp(g("feat", feat)), _vp(g("embd", embd)), cap]
        else:
            dst = g("dst", self.dst)
            dst = C.byref(dst) if dst is not None else None
            if name in TO:
                sink = [dst, _i32(g("clip_row", None))]
            else:
                src = g("src", self.ids[mel][1])
                sink = [dst, C.byref(src) if src is not None else None]
            sink += [_vp(g("embd", 0)), C.c_int64(g("cap", 0))]
        return [e, p] + head + [second, kl, n] + sink + [ol, st] + tail

    def call(self, name, **over):
        return getattr(self.q2a.lib(), name)(*self.argv(name, **over))

    def valid_bytes(self, family):
        """The family's valid call on buffers filled with a pattern first: the bytes of everything it writes."""
        name = VALID[family]
        for t in (self.out, self.feat, self.embd, self.dst_t):
            t.fill_(-3.0)
        for a in (self.out_host, self.feat_host, self.embd_host):
            a.fill(-3.0)
        self.ol.fill(-1)
        self.st.fill(-1)
        over = {"embd": self.embd.data_ptr(), "cap": self.embd.shape[0]} if name in TO + IDS else {}
        if name in TO:
            over["clip_row"] = np.array([4, 4 + int(self.kl_pcm[0]) // 2], dtype=np.int32)
        assert self.call(name, **over) == 0, self.q2a.lib().q2a_last_error()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().tobytes() for t in (self.out, self.feat, self.embd, self.dst_t.view(torch.int16))]
        return got + [a.tobytes() for a in (self.out_host, self.feat_host, self.embd_host, self.ol, self.st)]


@pytest.fixture(scope="module")
def ctx(make_model, host_build, workdir):
    import q2a
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    model = make_model("tiny", "f16")
    eng, eng_bf16 = q2a.Engine(model, device=0), q2a.Engine(model, device=0, act=q2a.ACT_BF16)
    path = os.path.join(workdir, f"proj-args-{eng.info.n_audio_state}x{D_OUT}-f16.bin")
    subprocess.check_call([TOOL, "gen-projector", path, str(eng.info.n_audio_state), str(D_OUT), "f16", "0x51A2"])
    proj = q2a.Projector(path, device=0)
    c = Ctx(eng, eng_bf16, proj)
    c.reference = {f: c.valid_bytes(f) for f in FAMILIES}   # before any rejected call
    yield c
    proj.close()
    eng_bf16.close()
    eng.close()


def _rows(c, name):
    """(what, overrides, expected code) for entry point `name`. The checks named are those of csrc/q2a_engine.hip."""
    mel, host = name in MEL_DEV + MEL_HOST, name in PCM_HOST + MEL_HOST
    hook = name.startswith("q2a_test_")
    feats = name in PACKED + TO + IDS
    kl_ok = c.kl_mel if mel else c.kl_pcm
    T = c.T
    rows = [
        # the prologue's (hooks, plain device and host calls: the entry point's or encode()'s) first check
        ("null engine", {"e": None}, -4),
        ("n_clips 0", {"n": 0}, -4),
        # device: behind the prologue, before the sink's checks; host: the loop's argument check
        ("null input", {"data": None}, -4),
    ]
    if name in KEYLEN:
        rows += [
            # key_lens: a key length outside 1..T, behind the activation contract
            ("key_len 0", {"kl": np.array([kl_ok[0], 0], dtype=np.int32)}, -4),
            ("key_len T+1", {"kl": np.array([T + 1, kl_ok[1]], dtype=np.int32)}, -4),
            ("bad key_len and null input", {"kl": np.array([0, 0], dtype=np.int32), "data": None}, -4),
            # lens_supported: the bf16 contract has no key-length kinds; the argument check is before it, the key
            # lengths and the input pointer behind it
            ("bf16 engine", {"e": c.eng_bf16}, -6),
            ("bf16 engine, n_clips 0", {"e": c.eng_bf16, "n": 0}, -4),
            ("bf16 engine, key_len 0", {"e": c.eng_bf16, "kl": np.array([0, 0], dtype=np.int32)}, -6),
            ("bf16 engine, null input", {"e": c.eng_bf16, "data": None}, -6),
        ]
    neg = np.array([0, -10], dtype=np.int32)
    if name == "q2a_encode_device":
        rows += [("negative offset_ms", {"offset_ms": -10}, -4)]   # encode(): offset_ms must be >= 0
    elif not host and not mel and not hook:
        # prepare_meta: a negative seek frame (explicit key lengths: the defaulting would refuse the offset first)
        rows += [("negative offset", {"second": neg, "kl": kl_ok if name in KEYLEN else None}, -4)]
    if mel and (not host or name in MEL_HOST):
        # device: prepare_meta's negative seek; host: the per-clip validation before any copy
        rows += [("negative seek", {"second": np.array([-1, 0], dtype=np.int32), "kl": kl_ok if name in KEYLEN else None}, -4)]
    if not host:
        # prepare_meta's per-clip ranges, behind the feature checks
        big = np.array([c.stride + 1, 100], dtype=np.int32)
        rows += [("bad length", {"lens": np.array([c.ld + 1, c.ld], dtype=np.int32) if mel else big,
                                 "kl": kl_ok if name in KEYLEN else None}, -4)]
    if name in MEL_DEV:
        rows += [("clip_stride below n_mels * ld", {"stride": c.M * c.ld - 1}, -4)]   # prepare_meta, before the clips
    if name in PACKED:
        rows += [
            # features_check: the packed rows against rows_cap; feat goes with a projector
            ("rows_cap one short", {"cap": c.rows[mel] - 1}, -4),
            ("null projector with feat", {"p": None}, -4),
        ]
        if not host:
            # features_check (rows_cap) is made before prepare_meta (n_samples / n_len): either way the same code
            bad = np.array([-1, int(c.ns[1])], dtype=np.int32) if not mel else np.array([0, int(c.nl[1])], dtype=np.int32)
            rows += [("bad length and short rows_cap", {"lens": bad, "kl": kl_ok, "cap": c.rows[mel] - 1}, -4)]
    if name in TO + IDS:
        rows += [
            # the entry point: a _to call needs a projector and a destination
            ("null dst", {"dst": None}, -4),
            ("null projector", {"p": None}, -4),
            # features_check: embd's rows_cap
            ("embd rows_cap one short", {"embd": c.embd.data_ptr(), "cap": c.rows[mel] - 1}, -4),
        ]
    if name in IDS:
        rows += [("null src", {"src": None}, -4)]   # the entry point: src is required
    if name in TO:
        rows += [("overlapping clip_row", {"clip_row": np.array([0, 0], dtype=np.int32)}, -4)]   # features_check: q2a_feat_rows
    return rows


@pytest.mark.parametrize("family", list(FAMILIES))
def test_rejected_calls(ctx, family):
    seen = []
    for name in FAMILIES[family]:
        for what, over, want in _rows(ctx, name):
            rc = ctx.call(name, **over)
            seen.append((name, what, rc, want))
    print("\n".join(f"{n}: {w}: rc {rc} (expected {x})" for n, w, rc, x in seen))
    bad = [s for s in seen if s[2] != s[3]]
    assert not bad, bad
    assert ctx.valid_bytes(family) == ctx.reference[family], f"{VALID[family]} after the rejected calls"


def test_every_entry_point_is_covered():
    assert sorted(n for f in FAMILIES.values() for n in f) == sorted(ALL) and len(ALL) == 20
