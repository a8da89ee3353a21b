"""TTS and cloning on the bf16 generator, ragged batches as dense length groups (openvoice_amd/bf16.py
``decode_groups``, csrc/ragged_bf16.hip, the ``generator=`` keyword).

Every bit-for-bit reference here is code that existed before the feature: ``GeneratorBf16.decode`` of the padded batch,
``ov_rows_f32_to_cl_bf16`` and torch's bfloat16 cast.  The two hand-over kernels copy, round and write zeros, so there
is no tolerance: NaN is written wherever they must not read or must overwrite, and wherever they must not write.
Against the fp32 generator the bf16 path is held to the figures of tests/test_gpu_bf16.py (max-abs 3e-2, relative RMS
1.5 %)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, bf16, clone  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
SPF = 256
BF16_MAX_ABS, BF16_REL_RMS = 3e-2, 1.5e-2       # tests/test_gpu_bf16.py: the bf16 generator against fp32
POISON = 0x7fc1                                  # a NaN that no conversion produces (bf16_rne gives 0x7fc0)


def _bits(t):
    return t.view(torch.int16)


# ---- 1. pack -----------------------------------------------------------------------------------------------------------
def _pack_case(C, cols, Ls, groups, src_ld, seed=0):
    """Items of ``cols[b]`` valid columns in rows of ``src_ld``; ``groups[g]``: the items of the group of ``Ls[g]``
    columns.  Returns (src [n, C, src_ld] with NaN beyond cols, records, expected bf16 arena, arena length)."""
    gen = torch.Generator().manual_seed(seed)
    n = len(cols)
    src = torch.randn(n, C, src_ld, generator=gen) * 3.0
    src[0, 0, 0] = float("inf")
    for b, c in enumerate(cols):
        src[b, :, c:] = float("nan")
    records, at = [None] * n, 0
    for idx, L in zip(groups, Ls):
        for b in idx:
            records[b] = (b * C * src_ld, src_ld, at, cols[b], L)
            at += L * C
    want = torch.full((at,), 0, dtype=torch.int16)
    for so, sld, do, c, L in records:
        blk = torch.zeros(L, C, dtype=torch.bfloat16)
        blk[:c] = src.reshape(-1)[so:so + C * sld].view(C, sld)[:, :c].t().to(torch.bfloat16)
        want[do:do + L * C] = _bits(blk).reshape(-1)
    return src, records, want, at


def _run_pack(src, records, C, used, lead_src=0, lead_dst=0, tail=64, dst_len=None):
    """Launch with the source ``lead_src`` floats and the destination ``lead_dst`` elements after a 16-byte boundary,
    the destination pre-filled with a NaN pattern; returns the destination's bits and the untouched parts."""
    sbuf = torch.full((lead_src + src.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    sbuf[lead_src:].copy_(src.reshape(-1))
    s = sbuf[lead_src:]
    dbuf = torch.full((lead_dst + used + tail,), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    d = dbuf[lead_dst:]
    assert s.data_ptr() % 16 == 4 * (lead_src % 4) and d.data_ptr() % 16 == 2 * (lead_dst % 8)
    recs = torch.tensor(records, dtype=torch.int64).to(DEV)
    _lib.call("ov_pack_groups_cl_bf16", s, s.numel(), recs, len(records), C, d, d.numel() if dst_len is None else dst_len)
    torch.cuda.synchronize()
    return _bits(d).cpu(), _bits(dbuf[:lead_dst]).cpu()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("lead_src,lead_dst", [(0, 0), (1, 0), (0, 3), (2, 8)])
def test_pack_is_exact_zero_beyond_and_never_reads_past_cols(monkeypatch, binding, lead_src, lead_dst):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    C, cols, Ls, groups = 192, (1, 5, 37), (21, 53), ([0, 1], [2])
    src, records, want, used = _pack_case(C, cols, Ls, groups, src_ld=40)
    got, lead = _run_pack(src, records, C, used, lead_src, lead_dst)
    assert (lead == POISON).all() and (got[used:] == POISON).all() and got[used:].numel() == 64
    assert torch.equal(got[:used], want)
    x = got[:used].view(torch.bfloat16).float()
    assert not torch.isnan(x).any()                              # no NaN anywhere in a group tensor
    for so, sld, do, c, L in records:                            # stated once more in the issue's own words
        blk = x[do:do + L * C].view(L, C)
        assert torch.equal(blk[:c], src.reshape(-1)[so:so + C * sld].view(C, sld)[:, :c].t().to(torch.bfloat16).float())
        assert (blk[c:] == 0).all()
    # the same bits as the dense hand-over of the live units
    dense = torch.full((37, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    row = src[2].contiguous().to(DEV)
    _lib.call("ov_rows_f32_to_cl_bf16", row, C * 40, 40, dense, 1, C, 37)
    do = records[2][2]
    assert torch.equal(_bits(dense).cpu().reshape(-1), got[do:do + 37 * C])


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_pack_records_the_kernel_must_refuse_leave_their_destination_untouched(monkeypatch, binding):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    C, cols, Ls, groups = 192, (1, 5, 37), (21, 53), ([0, 1], [2])
    src, records, want, used = _pack_case(C, cols, Ls, groups, src_ld=40)
    big = 1 << 62
    bad = [(0, 40, used, 22, 21),                        # cols > L
           (0, 40, used + 64 - 20 * C, 1, 21),           # reaches past dst_len
           (0, 40, used, 1, 1),                          # ... by one column of the tail (64 < C elements)
           (-4, 40, used, 1, 1), (0, -1, used, 1, 1), (0, 40, -8, 1, 1), (0, 40, used, -1, 1), (0, 40, used, 0, 0),
           (src.numel() - 40 * (C - 1) - 4, 40, 0, 5, 5),       # would read past the source
           (big, 40, 0, 1, 1), (0, big, 0, 1, 1), (0, 40, big, 1, 1), (0, 40, 0, 1, big), (0, 40, 0, big, big)]
    for i in range(0, len(bad), 5):
        got, _ = _run_pack(src, records[:2] + bad[i:i + 5] + records[2:], C, used)
        assert torch.equal(got[:used], want) and (got[used:] == POISON).all(), i
    # a destination that ends exactly at dst_len is legal; so is a source row that ends exactly at src_len
    got, _ = _run_pack(src, records, C, used, tail=0)
    assert torch.equal(got, want)


@pytest.mark.parametrize("src_ld", [1031, 1032])
def test_pack_long_rows_take_further_passes_and_a_partial_channel_tile(src_ld):
    """More column tiles than the grid has (16 x 64), C = 40 (a second channel tile of 8 channels), an empty item, an
    item of exactly one tile; rows on the vector path (``src_ld`` % 4 == 0) and on the scalar one."""
    C, cols, Ls, groups = 40, (1030, 0, 64), (1100, 3, 64), ([0], [1], [2])
    src, records, want, used = _pack_case(C, cols, Ls, groups, src_ld=src_ld, seed=3)
    got, _ = _run_pack(src, records, C, used)
    assert torch.equal(got[:used], want) and (got[used:] == POISON).all()


# ---- 2. unpack ---------------------------------------------------------------------------------------------------------
KEEPS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099]
PADS = [0, 1, 3, 1102]


def _unpack_case(shift, long_row=False):
    rng = np.random.default_rng(40 + shift)
    keeps = [KEEPS[i % len(KEEPS)] for i in range(24)]
    rows = [k + PADS[(i // len(KEEPS) + i + shift) % len(PADS)] for i, k in enumerate(keeps)]
    if long_row:                                                   # more chunks than the grid has (64 x 4096 samples)
        keeps, rows = keeps + [270001], rows + [300003]
    ld = max(keeps) + 2                                            # not a multiple of 4 when 4099 is the longest
    src = np.full((len(keeps), ld), np.nan, dtype=np.float32)
    for i, k in enumerate(keeps):
        src[i, :k] = rng.standard_normal(k).astype(np.float32)    # NaN beyond keep: reading past it would show
    order, records, at = rng.permutation(len(keeps)), [None] * len(keeps), 0
    for i in order:
        records[i] = (i * ld, at, keeps[i], rows[i])
        at += rows[i]
    want = np.full(at + 37, np.nan, dtype=np.float32)
    for so, do, k, r in records:
        want[do:do + k] = src.reshape(-1)[so:so + k]
        want[do + k:do + r] = 0.0
    return src, records, want, at


def _run_unpack(src, records, dst_elems, lead):
    srcd = torch.from_numpy(src).to(DEV)
    buf = torch.full((lead + dst_elems,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[lead:]
    recs = torch.tensor(records, dtype=torch.int64).to(DEV)
    _lib.call("ov_unpack_groups_f32", srcd, srcd.numel(), recs, len(records), dst, dst.numel())
    torch.cuda.synchronize()
    return dst.cpu().numpy(), buf[:lead].cpu().numpy()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_unpack_is_exact_at_every_alignment(monkeypatch, binding, shift):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    src, records, want, used = _unpack_case(shift, long_row=shift == 3)
    got, lead = _run_unpack(src, records, want.shape[0], lead=shift)
    assert np.isnan(lead).all() and not np.isnan(got[:used]).any()
    assert np.array_equal(got[:used], want[:used])                  # kept samples exact, the tail of every row zero
    assert np.isnan(got[used:]).all() and got[used:].shape[0] == 37


def test_unpack_records_the_kernel_must_refuse_copy_nothing():
    src, records, want, used = _unpack_case(1)
    n_src, n_dst, big = src.size, want.shape[0], 1 << 62
    bad = [(n_src - 2, used, 4, 4), (-1, used, 2, 2), (0, -1, 2, 2), (0, used, -1, 2), (0, used, 3, 2),
           (0, n_dst - 3, 0, 4), (0, used, 1, 38), (big, used, 1, 1), (0, big, 1, 1), (0, used, big, big),
           (0, used, 0, (1 << 63) - 1)]
    for i in range(0, len(bad), 4):
        got, _ = _run_unpack(src, records[:10] + bad[i:i + 4] + records[10:], n_dst, lead=0)
        assert np.array_equal(got, want, equal_nan=True), i
    got, _ = _run_unpack(src, records + [(0, used, 0, 37)], n_dst, lead=0)          # exactly the tail: legal
    assert np.array_equal(got[:used], want[:used]) and (got[used:] == 0).all()


# ---- 3. grouped decode against the padded decode -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_bf16(synth_sd):
    return bf16.GeneratorBf16(synth_sd, CFG, DEV)


_padded = {}


def _decode_case(gen, lengths, T, fuse):
    """(z_rows with NaN beyond every length, cond rows, the padded reference) -- the reference computed once per case."""
    key = (tuple(lengths), T, fuse)
    if key not in _padded:
        g = torch.Generator().manual_seed(T + len(lengths))
        B, ld = len(lengths), T + 8
        z = torch.randn(B, 192, ld, generator=g)
        cond_g = 0.3 * torch.randn(B, 256, 1, generator=g)
        rows = z.clone()
        for b, n in enumerate(lengths):
            z[b, :, n:] = 0.0                                       # what the flow's mask leaves beyond a length
            rows[b, :, n:] = float("nan")                           # ... and what decode_groups must never read
        gen.fuse_pairs = fuse
        ref = gen.decode(z[:, :, :T].to(DEV), cond_g.to(DEV)).clone()
        _padded[key] = (rows.to(DEV), gen.cond_rows(cond_g.to(DEV)), ref)
    return _padded[key]


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("max_groups", [1, 2, 3, 5])
def test_grouped_decode_equals_the_padded_decode_on_every_valid_sample(gen_bf16, max_groups, fuse):
    gen, lengths, T = gen_bf16, (3, 20, 21, 47, 64), 64
    rows, cond, ref = _decode_case(gen, lengths, T, fuse)
    gen.fuse_pairs = fuse
    gen.group_cost = 0                      # a group is free: the plan uses every group it is allowed
    try:
        o = gen.decode_groups(rows, T + 8, cond, lengths, T, max_groups=max_groups)
        again = gen.decode_groups(rows, T + 8, cond, list(lengths), T, max_groups=max_groups)
    finally:
        gen.group_cost, gen.fuse_pairs = bf16.DEFAULT_GROUP_COST, True
    torch.cuda.synchronize()
    assert len(gen.last_plan) == max_groups
    assert o.shape == ref.shape == (5, 1, T * SPF) and o.dtype == torch.float32
    assert torch.isfinite(o).all() and torch.equal(o, again)
    for b, n in enumerate(lengths):
        assert torch.equal(o[b, 0, :n * SPF], ref[b, 0, :n * SPF]), (b, n)
        assert (o[b, 0, n * SPF:] == 0).all(), (b, n)


def test_grouped_decode_of_equal_lengths_is_one_group_and_the_padded_decode(gen_bf16):
    gen, lengths, T = gen_bf16, (33, 33, 33), 33
    rows, cond, ref = _decode_case(gen, lengths, T, True)
    o = gen.decode_groups(rows, T + 8, cond, lengths, T, max_groups=5)
    assert gen.last_plan == [([0, 1, 2], T)]
    assert torch.equal(o, ref)
    # one shared cond row, lengths longer than Td (max_len cuts the decoder input): clamped
    o1 = gen.decode_groups(rows, T + 8, cond[:1], (40, 33, 50), T)
    r1 = gen.decode_groups(rows, T + 8, cond[:1].expand(3, -1).contiguous(), lengths, T)
    assert torch.equal(o1, r1)
    with pytest.raises(_lib.OvError):
        gen.decode_groups(rows[:, :, :T], T + 8, cond, lengths, T)
    with pytest.raises(_lib.OvError):
        gen.decode_groups(rows, T + 8, cond, lengths, T, max_groups=0)


# ---- 4. TTS ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tts_model(synth_tts_sd):
    m = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    m.load_state_dict(synth_tts_sd, strict=True)
    return m.to(DEV).eval()


def _tts_inputs():
    gen = torch.Generator().manual_seed(21)
    B, Tx = 4, 12
    lengths = torch.tensor([12, 9, 5, 2])
    tokens = torch.randint(1, 68, (B, Tx), generator=gen)
    for b, n in enumerate(lengths.tolist()):
        tokens[b, n:] = 0
    sid = torch.tensor([0, 3, 3, 9])
    return tokens, lengths, sid, torch.randn(B, 2, Tx, generator=gen), torch.randn(B, 192, 64 * Tx, generator=gen)


def _within_bf16_tolerance(o, o32, lens):
    valid = torch.arange(o.shape[2], device=o.device)[None, None, :] < (lens * SPF).view(-1, 1, 1).to(o.device)
    err, ref = (o - o32)[valid], o32[valid]
    mx, rel = err.abs().max().item(), (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"bf16 TTS against fp32 on the valid samples: max-abs {mx:.4f}, rel RMS {rel:.4f}")
    assert 1e-5 < mx <= BF16_MAX_ABS and rel <= BF16_REL_RMS, (mx, rel)


@pytest.mark.parametrize("noise", ["explicit", "seed"])
def test_tts_on_the_bf16_generator(tts_model, noise):
    tokens, lengths, sid, noise_w, noise_z = _tts_inputs()
    kw = dict(noise_scale=0.667, noise_scale_w=0.6, sdp_ratio=0.2)
    kw.update(dict(noise_w=noise_w, noise_z=noise_z) if noise == "explicit" else dict(seed=77))
    o32, attn32, ym32, lat32 = tts_model.infer(tokens, lengths, sid=sid, skip_padding=True, **kw)
    gen = tts_model.engine().core.bf16_generator()
    assert not getattr(tts_model.engine().core, "_bf16_on", False)
    lens = ym32[:, 0].sum(1).long()
    Ty = int(lens.max())
    assert len(set(lens.tolist())) > 1 and o32.shape == (4, 1, Ty * SPF)
    by_hand = gen.decode(lat32[0], tts_model.engine().emb_g.index_select(0, sid.to(DEV)).unsqueeze(-1)).clone()

    def check_front(attn, ym, lat):
        assert torch.equal(attn, attn32) and torch.equal(ym, ym32)
        assert all(torch.equal(a, b) for a, b in zip(lat, lat32))

    for settings in (None, (4, 0)):                    # the defaults, then four free groups
        if settings is not None:
            gen.max_groups, gen.group_cost = settings
        try:
            o, attn, ym, lat = tts_model.infer(tokens, lengths, sid=sid, skip_padding=True, generator="bf16", **kw)
        finally:
            gen.max_groups, gen.group_cost = bf16.DEFAULT_MAX_GROUPS, bf16.DEFAULT_GROUP_COST
        check_front(attn, ym, lat)
        if settings is not None:
            assert len(gen.last_plan) == len(set(min(Ty, n + gen.margin) for n in lens.tolist())) > 1
        assert o.shape == o32.shape
        for b, n in enumerate(lens.tolist()):
            assert torch.equal(o[b, 0, :n * SPF], by_hand[b, 0, :n * SPF]), (settings, b)
            assert (o[b, 0, n * SPF:] == 0).all(), (settings, b)
        _within_bf16_tolerance(o, o32, lens)
    o, attn, ym, lat = tts_model.infer(tokens, lengths, sid=sid, generator="bf16", **kw)     # padded: equal everywhere
    check_front(attn, ym, lat)
    assert torch.equal(o, by_hand)
    assert not getattr(tts_model.engine().core, "_bf16_on", False)         # the switch was neither read nor set
    with pytest.raises(_lib.OvError, match="generator must be"):
        tts_model.engine().infer(tokens, lengths, sid, generator="fp16", **kw)


# ---- 5. the cloner ---------------------------------------------------------------------------------------------------------
def _converter(d, synth_sd, sr):
    hps = default_converter_hparams("v2")
    data = dict(hps.data.items(), sampling_rate=sr)
    (d / f"conv{sr}.json").write_text(json.dumps({"_version_": "v2", "data": data, "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "converter.pth")
    t = api.ToneColorConverter(str(d / f"conv{sr}.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "converter.pth"))
    return t


@pytest.fixture(scope="module")
def models(tmp_path_factory, synth_sd, synth_tts_sd):
    d = tmp_path_factory.mktemp("clone_bf16")
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1, "whispering": 2}}
    (d / "tts.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, d / "tts.pth")
    tts = api.BaseSpeakerTTS(str(d / "tts.json"), device=DEV)
    tts.load_ckpt(str(d / "tts.pth"))
    return tts, _converter(d, synth_sd, 22050)


FRAMES_PER_ID = 64          # columns of explicit noise per symbol id: far more than the duration predictor gives


def _requests(seed=5):
    """Two requests of two sentences of 4-11 ids, explicit noise for every draw of the chain."""
    gen = torch.Generator().manual_seed(seed)
    ids = [[api.intersperse(torch.randint(1, 68, (n,), generator=gen).tolist(), 0) for n in ns] for ns in ([7, 4], [5, 11])]
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV), 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV))
           for _ in ids]
    requests = [(i, "default", s, t, 1.0, None) for i, (s, t) in zip(ids, ses)]
    noise_w = [[torch.randn(2, len(s), generator=gen) for s in req] for req in ids]
    noise_z = [[torch.randn(192, FRAMES_PER_ID * len(s), generator=gen) for s in req] for req in ids]
    noise = [torch.randn(1, 192, FRAMES_PER_ID * sum(len(s) for s in req) + 64, generator=gen) for req in ids]
    return requests, dict(noise_w=noise_w, noise_z=noise_z, noise=noise)


def _manual_chain(tts, conv, requests, nz, **gen_kw):
    """The chain as a user of the public pieces writes it: host waveforms between the two models."""
    ids = [q[0] for q in requests]
    sid = lambda spk: tts.hps.speakers[spk] if isinstance(spk, str) else spk
    batches = clone.sentence_batches([[len(s) for s in req] for req in ids], [(q[4], sid(q[1])) for q in requests], 32)
    seg = {}
    for (speed, speaker), items in batches:
        audios = tts.tts_from_ids([ids[r][s] for r, s in items], speaker, speed=speed, batched=True,
                                  noise_w=[nz["noise_w"][r][s] for r, s in items],
                                  noise_z=[nz["noise_z"][r][s] for r, s in items], **gen_kw)
        seg.update(zip(items, audios))
    sr = tts.hps.data.sampling_rate
    joined = [tts.audio_numpy_concat([seg[(r, s)] for s in range(len(q[0]))], sr=sr, speed=q[4])
              for r, q in enumerate(requests)]
    return joined, conv.convert_many(joined, [q[2] for q in requests], [q[3] for q in requests], noise=nz["noise"], sr=sr,
                                     out_sr=[q[5] for q in requests], **gen_kw)


def test_cloner_on_bf16_equals_the_chain_of_the_public_pieces_on_bf16(models):
    tts, conv = models
    requests, nz = _requests()
    vc = clone.VoiceCloner(tts, conv)
    got = vc.speak_ids_many(requests, generator="bf16", **nz)
    joined, want = _manual_chain(tts, conv, requests, nz, generator="bf16")
    assert len(got) == len(want) == 2
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape and len(g) > 4000 and np.isfinite(g).all(), r
        assert np.array_equal(g, w), r
    one = vc.speak_ids(*requests[0][:4], generator="bf16", noise_w=nz["noise_w"][0], noise_z=nz["noise_z"][0],
                       noise=nz["noise"][0])
    many = vc.speak_ids_many(requests[:1], generator="bf16", noise_w=nz["noise_w"][:1], noise_z=nz["noise_z"][:1],
                             noise=nz["noise"][:1])
    assert np.array_equal(one, many[0])
    # genuinely another generator than the default chain, and within the bf16 path's tolerance of it per half:
    # the fp32 chain on the same numbers
    got32 = vc.speak_ids_many(requests, **nz)
    assert all(a.shape == b.shape and not np.array_equal(a, b) for a, b in zip(got, got32))
    # the converter half alone: the keyword equals the engine's switch
    ses = [q[2] for q in requests], [q[3] for q in requests]
    by_kw = conv.convert_many(joined, *ses, noise=nz["noise"], sr=22050, generator="bf16")
    eng = conv.model.engine()
    assert not getattr(eng, "_bf16_on", False)
    eng.use_bf16_generator(True)
    try:
        by_switch = conv.convert_many(joined, *ses, noise=nz["noise"], sr=22050)
        forced32 = conv.convert_many(joined, *ses, noise=nz["noise"], sr=22050, generator="fp32")
    finally:
        eng.use_bf16_generator(False)
    plain32 = conv.convert_many(joined, *ses, noise=nz["noise"], sr=22050)
    for a, b, c, d in zip(by_kw, by_switch, forced32, plain32):
        assert np.array_equal(a, b) and np.array_equal(c, d) and not np.array_equal(a, c)


# ---- 6. defaults -------------------------------------------------------------------------------------------------------
def test_every_new_keyword_left_out_or_fp32_is_the_same_call(models, tts_model):
    tts, conv = models
    tokens, lengths, sid, noise_w, noise_z = _tts_inputs()
    kw = dict(sid=sid, noise_scale=0.667, noise_scale_w=0.6, noise_w=noise_w, noise_z=noise_z)
    for skip in (False, True):
        a = tts_model.infer(tokens, lengths, skip_padding=skip, **kw)
        b = tts_model.infer(tokens, lengths, skip_padding=skip, generator="fp32", **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    requests, nz = _requests(seed=6)
    ids = [s for q in requests for s in q[0]]
    flat = lambda v: [x for per in v for x in per]
    for batched in (False, True):
        a = tts.tts_from_ids(ids, 1, batched=batched, noise_w=flat(nz["noise_w"]), noise_z=flat(nz["noise_z"]))
        b = tts.tts_from_ids(ids, 1, batched=batched, noise_w=flat(nz["noise_w"]), noise_z=flat(nz["noise_z"]),
                             generator="fp32")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    vc = clone.VoiceCloner(tts, conv)
    a = vc.speak_ids_many(requests, **nz)
    b = vc.speak_ids_many(requests, generator="fp32", **nz)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ses = [q[2] for q in requests], [q[3] for q in requests]
    waves = [x[:9000] for x in a]
    c = conv.convert_many(waves, *ses, noise=nz["noise"])
    for g in (None, "fp32"):
        d = conv.convert_many(waves, *ses, noise=nz["noise"], generator=g)
        assert all(np.array_equal(x, y) for x, y in zip(c, d)), g
    # the model seam
    gen = torch.Generator().manual_seed(2)
    spec = (torch.rand(2, 513, 40, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
    lens, nzc = torch.tensor([40, 23]).to(DEV), torch.randn(2, 192, 40, generator=gen).to(DEV)
    g1, g2 = ses[0][0], ses[1][0]
    m = conv.model
    for skip in (False, True):
        ref = m.voice_conversion(spec, lens, g1, g2, tau=0.3, noise=nzc, skip_padding=skip)[0].clone()
        for g in (None, "fp32"):
            assert torch.equal(m.voice_conversion(spec, lens, g1, g2, tau=0.3, noise=nzc, skip_padding=skip, generator=g)[0], ref)
        o16 = m.voice_conversion(spec, lens, g1, g2, tau=0.3, noise=nzc, skip_padding=skip, generator="bf16")[0]
        err = (o16 - ref).abs().max().item()
        assert 1e-5 < err <= BF16_MAX_ABS, err
    with pytest.raises(_lib.OvError, match="generator must be"):
        m.engine().voice_conversion(spec, lens, g1, g2, generator="fp16")
    with pytest.raises(_lib.OvError, match="captured graph"):
        m.voice_conversion(spec, lens, g1, g2, graph=True, generator="bf16")
