"""The cloned-voice chain on the MI355X (openvoice_amd/clone.py, csrc/clone.hip).

* ``ov_join_segments_f32`` against a numpy loop, exact: it copies and writes zeros, so there is no tolerance -- every
  sample inside a record must be the expected one, every sample outside untouched (NaN before, NaN after).
* ``VoiceCloner.speak_ids_many`` against the chain made of the public pieces (``tts_from_ids(batched=True)`` per batch of
  ``sentence_batches``, ``audio_numpy_concat`` per request, ``ToneColorConverter.convert_many``), ``np.array_equal``: the
  two run the same launches on the same numbers, the join moves float32 samples unchanged.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, audio_io, clone  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099]
GAPS = [0, 1, 3, 1102]
LD = 4101                   # not a multiple of 4: row b starts at residue b mod 4
ROWS = 40
TAIL = 37


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def _case(shift):
    """40 records, one per row: lengths cycle through LENGTHS, gaps through GAPS starting at ``shift`` (over the four
    shifts every length meets every gap), rows packed back to back in dst in a shuffled order."""
    rng = np.random.default_rng(100 + shift)
    src = np.full((ROWS, LD), np.nan, dtype=np.float32)
    ns = [LENGTHS[b % len(LENGTHS)] for b in range(ROWS)]
    gaps = [GAPS[(b // len(LENGTHS) + b + shift) % len(GAPS)] for b in range(ROWS)]
    for b, n in enumerate(ns):
        src[b, :n] = rng.standard_normal(n).astype(np.float32)          # NaN beyond n: reading past n would show
    order = rng.permutation(ROWS)
    records, at = [None] * ROWS, 0
    for b in order:
        records[b] = (b * LD, ns[b], at, gaps[b])
        at += ns[b] + gaps[b]
    want = np.full(at + TAIL, np.nan, dtype=np.float32)
    for s, n, d, g in records:
        want[d:d + n] = src.reshape(-1)[s:s + n]
        want[d + n:d + n + g] = 0.0
    return src, records, want, at


def _run(src, records, dst_elems, lead, max_span=None):
    """Launch on a dst that starts ``lead`` floats after a 16-byte boundary, pre-filled with NaN."""
    srcd = torch.from_numpy(src).to(DEV)
    buf = torch.full((lead + dst_elems,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[lead:]
    assert dst.data_ptr() % 16 == 4 * (lead % 4)
    recs = torch.tensor(records, dtype=torch.int64).to(DEV)
    span = min(max(n + g for _, n, _, g in records), 1 << 31) if max_span is None else max_span
    _lib.call("ov_join_segments_f32", srcd, srcd.numel(), recs, len(records), dst, dst.numel(), span)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), buf[:lead].cpu().numpy()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_join_kernel_is_exact_at_every_alignment(monkeypatch, binding, shift):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    src, records, want, used = _case(shift)
    # the source is misaligned against the destination in every residue, and so is the destination against 16 bytes
    assert {(s - d - shift) % 4 for s, n, d, g in records if n >= 8} == {0, 1, 2, 3}
    assert {(d + shift) % 4 for s, n, d, g in records if n >= 8} == {0, 1, 2, 3}
    got, lead = _run(src, records, want.shape[0], lead=shift)
    assert np.isnan(lead).all()
    assert not np.isnan(got[:used]).any()                      # NaN-free inside the records
    assert np.array_equal(got[:used], want[:used])
    assert np.isnan(got[used:]).all() and got[used:].shape[0] == TAIL     # the tail beyond the last record: untouched


def test_join_kernel_every_length_meets_every_gap():
    pairs = set()
    for shift in range(4):
        pairs |= {(n, g) for _, n, _, g in _case(shift)[1]}
    assert pairs >= {(n, g) for n in LENGTHS for g in GAPS}


def test_join_kernel_out_of_range_records_copy_nothing():
    src, records, want, used = _case(1)
    src_elems, dst_elems = src.size, want.shape[0]
    big = 1 << 62
    bad = [(src_elems - 2, 4, used, 0),              # would read past the source
           (-1, 2, used, 0), (0, -1, used, 2), (0, 2, used, -1), (0, 2, -1, 0),
           (0, 4, dst_elems - 3, 0),                 # would write past the destination
           (0, 0, dst_elems - 3, 4), (0, TAIL, used, 1),
           (0, big, used, big), (0, 0, used, (1 << 63) - 1), (big, 2, used, 0), (0, 2, big, 0)]
    for i in range(0, len(bad), 3):
        mixed = records[:20] + bad[i:i + 3] + records[20:]
        got, _ = _run(src, mixed, dst_elems, lead=0)
        assert np.array_equal(got, want, equal_nan=True), i          # the rest exact, the tail still NaN
    # a record that exactly fills the tail is legal
    got, _ = _run(src, records + [(0, 0, used, TAIL)], dst_elems, lead=0)
    assert np.array_equal(got[:used], want[:used]) and (got[used:] == 0).all()


def test_join_kernel_long_segment_spans_many_chunks_and_a_short_grid():
    """One segment of many chunks (grid over (record, chunk)), and the same launch with ``max_span`` understated: the
    workgroups then take further passes and the record is still joined whole."""
    rng = np.random.default_rng(7)
    n, gap = 5 * 4096 + 1021, 4096 + 3
    src = np.full((2, n + 3), np.nan, dtype=np.float32)
    src[1, :n] = rng.standard_normal(n).astype(np.float32)
    records = [(n + 3, n, 5, gap), (0, 0, 0, 5)]
    want = np.full(5 + n + gap + TAIL, np.nan, dtype=np.float32)
    want[:5] = 0.0
    want[5:5 + n] = src[1, :n]
    want[5 + n:5 + n + gap] = 0.0
    for lead in (0, 3):
        for max_span in (None, 0, 4096):
            got, _ = _run(src, records, want.shape[0], lead=lead, max_span=max_span)
            assert np.array_equal(got, want, equal_nan=True), (lead, max_span)


def test_join_segments_equals_audio_numpy_concat():
    rng = np.random.default_rng(11)
    hop, B, ld = 256, 7, 6 * 256
    frames = [3, 6, 1, 0, 5, 2, 4]
    o = np.full((B, 1, ld), np.nan, dtype=np.float32)
    for b, f in enumerate(frames):
        o[b, 0, :f * hop] = rng.standard_normal(f * hop).astype(np.float32)
    groups = [[1, 4], [3], [6, 0, 2, 5], []]
    speeds = [1.0, 0.7, 2.0, 1.0]
    gaps = [clone.gap_samples(22050, s) for s in speeds]
    od = torch.from_numpy(o).to(DEV)
    lens = torch.tensor(frames, device=DEV) * hop                       # device counts: the one small copy to the host
    got = clone.join_segments(od, lens, groups, gaps)
    got_host_lens = clone.join_segments(od[:, 0], [f * hop for f in frames], groups, gaps)
    host = clone.join_segments_host([[o[b, 0, :frames[b] * hop] for b in rows] for rows in groups], gaps)
    for rows, speed, g, g2, h in zip(groups, speeds, got, got_host_lens, host):
        want = api.BaseSpeakerTTS.audio_numpy_concat([o[b, 0, :frames[b] * hop] for b in rows], sr=22050, speed=speed)
        assert g.data_ptr() % 16 == 0
        assert np.array_equal(g.cpu().numpy(), want) and np.array_equal(g2.cpu().numpy(), want)
        assert np.array_equal(h.astype(np.float32), want)
    with pytest.raises(ValueError):
        clone.join_segments(od, lens, [[7]], 0)
    with pytest.raises(ValueError):
        clone.join_segments(od, [ld + 1] * B, [[0]], 0)


# ---- end to end ----------------------------------------------------------------------------------------------------------
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
    d = tmp_path_factory.mktemp("clone")
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1, "whispering": 2}}
    (d / "tts.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, d / "tts.pth")
    tts = api.BaseSpeakerTTS(str(d / "tts.json"), device=DEV)
    tts.load_ckpt(str(d / "tts.pth"))
    return tts, _converter(d, synth_sd, 22050), _converter(d, synth_sd, 16000)


FRAMES_PER_ID = 64          # columns of explicit noise per symbol id: far more than the duration predictor gives


def _requests(seed=5):
    """Three requests of 1, 3 and 2 sentences of 5-23 ids; request 1 at speed 1.3, request 2 wants 16 kHz."""
    gen = torch.Generator().manual_seed(seed)
    ids = [[api.intersperse(torch.randint(1, 68, (n,), generator=gen).tolist(), 0) for n in ns]
           for ns in ([11], [5, 23, 9], [17, 8])]
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV), 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV))
           for _ in ids]
    speakers, speeds, out_srs = ["default", "whispering", 1], [1.0, 1.3, 1.0], [None, None, 16000]
    requests = [(i, spk, s, t, spd, r) for i, spk, (s, t), spd, r in zip(ids, speakers, ses, speeds, out_srs)]
    return requests, _noise_for(ids, gen)


def _noise_for(ids, gen):
    noise_w = [[torch.randn(2, len(s), generator=gen) for s in req] for req in ids]
    noise_z = [[torch.randn(192, FRAMES_PER_ID * len(s), generator=gen) for s in req] for req in ids]
    noise = [torch.randn(1, 192, FRAMES_PER_ID * sum(len(s) for s in req) + 64, generator=gen) for req in ids]
    return dict(noise_w=noise_w, noise_z=noise_z, noise=noise)


def _manual_chain(tts, conv, requests, nz, middle=None, **kw):
    """The chain as a user of the public pieces writes it: host waveforms between the two models."""
    ids = [q[0] for q in requests]
    sid = lambda spk: tts.hps.speakers[spk] if isinstance(spk, str) else spk
    batches = clone.sentence_batches([[len(s) for s in req] for req in ids], [(q[4], sid(q[1])) for q in requests], 32)
    seg = {}
    for (speed, speaker), items in batches:
        audios = tts.tts_from_ids([ids[r][s] for r, s in items], speaker, speed=speed, batched=True,
                                  noise_w=[nz["noise_w"][r][s] for r, s in items],
                                  noise_z=[nz["noise_z"][r][s] for r, s in items])
        seg.update(zip(items, audios))
    sr = tts.hps.data.sampling_rate
    joined = [tts.audio_numpy_concat([seg[(r, s)] for s in range(len(q[0]))], sr=sr, speed=q[4])
              for r, q in enumerate(requests)]
    if middle is not None:
        joined, sr = [middle(x) for x in joined], None
    return conv.convert_many(joined, [q[2] for q in requests], [q[3] for q in requests], noise=nz["noise"], sr=sr,
                             out_sr=[q[5] for q in requests], **kw), batches


def test_speak_ids_many_equals_the_manual_chain_bitwise(models, tmp_path):
    tts, conv, _ = models
    requests, nz = _requests()
    vc = clone.VoiceCloner(tts, conv)
    got = vc.speak_ids_many(requests, **nz)
    want, batches = _manual_chain(tts, conv, requests, nz)
    assert vc.last_batches == batches and [len(i) for _, i in batches] == [3, 3]     # requests 0 and 2 share a launch
    assert vc.last_launches == {"infer": 2, "join": 2}
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.ndim == 1 and g.shape == w.shape and len(g) > 4000, r
        assert np.isfinite(g).all() and np.array_equal(g, w), r
    # twice: equal
    again = vc.speak_ids_many(requests, **nz)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    # files: the same bytes the manual chain writes, and the returned audio at 16 bits
    paths = [str(tmp_path / f"clone{i}.wav") for i in range(3)]
    ref_paths = [str(tmp_path / f"manual{i}.wav") for i in range(3)]
    ret = vc.speak_ids_many(requests, output_paths=paths, **nz)
    assert all(np.array_equal(a, b) for a, b in zip(got, ret))
    _manual_chain(tts, conv, requests, nz, output_paths=ref_paths)
    for p, q, g, rate in zip(paths, ref_paths, got, (22050, 22050, 16000)):
        assert open(p, "rb").read() == open(q, "rb").read()
        y, sr = audio_io.load(p, None)
        assert sr == rate and y.shape == g.shape and np.abs(y - np.clip(g, -1.0, 32767 / 32768)).max() <= 1.0 / 32768


def test_speak_ids_is_the_one_request_form(models):
    tts, conv, _ = models
    requests, nz = _requests()
    vc = clone.VoiceCloner(tts, conv)
    ids, spk, s, t, spd, r = requests[0]
    one = vc.speak_ids(ids, spk, s, t, speed=spd, out_sr=r, noise_w=nz["noise_w"][0], noise_z=nz["noise_z"][0],
                       noise=nz["noise"][0])
    many = vc.speak_ids_many(requests[:1], noise_w=nz["noise_w"][:1], noise_z=nz["noise_z"][:1], noise=nz["noise"][:1])
    assert len(many) == 1 and np.array_equal(one, many[0])
    # small batches: the same sentences one per launch -- another batch composition, the same lengths
    solo = vc.speak_ids_many(requests, max_sentences_per_launch=1, **nz)
    assert vc.last_launches == {"infer": 6, "join": 6}
    full = vc.speak_ids_many(requests, **nz)
    assert [a.shape for a in solo] == [b.shape for b in full]


def test_speak_goes_through_the_text_front_end(models):
    tts, conv, _ = models
    vc = clone.VoiceCloner(tts, conv)
    gen = torch.Generator().manual_seed(8)
    se = (0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV), 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV))
    # two sentences of more than ten words each: split_sentence keeps them apart
    text = ("Hello world, this is a test of the chain from text to a voice. "
            "Another sentence follows it so that the join has two segments to put together!")
    with pytest.raises(RuntimeError, match="no text front end registered"):
        vc.speak(text, "default", *se)
    api.BaseSpeakerTTS.text_to_sequence = staticmethod(lambda text, symbols, cleaners: [1 + (ord(c) % 67) for c in text])
    try:
        ids = tts.text_to_ids(text, "English")
        assert len(ids) >= 2
        nz = _noise_for([ids], gen)
        one = {k: v[0] for k, v in nz.items()}
        spoken = vc.speak(text, "default", *se, speed=1.1, **one)
        many = vc.speak_many([text], "default", *se, speed=1.1, **nz)
    finally:
        api.BaseSpeakerTTS.text_to_sequence = None
    from_ids = vc.speak_ids(ids, "default", *se, speed=1.1, **one)
    assert np.array_equal(spoken, from_ids) and np.array_equal(many[0], from_ids)


def test_models_at_different_rates_resample_in_the_middle(models):
    tts, _, conv16 = models
    requests, nz = _requests(seed=6)
    requests = [q[:5] + (r,) for q, r in zip(requests, (None, 22050, None))]
    vc = clone.VoiceCloner(tts, conv16)
    got = vc.speak_ids_many(requests, **nz)
    to16 = lambda x: audio_io.resample_on_device(torch.from_numpy(x).to(DEV), 22050, 16000)
    want, _ = _manual_chain(tts, conv16, requests, nz, middle=to16)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), r
    # and through convert_many's own rate handling (sr = the TTS rate)
    want2, _ = _manual_chain(tts, conv16, requests, nz)
    assert all(np.array_equal(g, w) for g, w in zip(got, want2))
