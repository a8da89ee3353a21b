"""Silence removal without a GPU (openvoice_amd/vad.py, se_extractor.split_audio_vad): the float64 host restatement of
the detector against a brute force written here with explicit loops over runs (not the scan formulation), parameter
validation, the three entry points' argument checks, and the file layout ``get_se`` leaves behind."""
import math
import os

import numpy as np
import pytest
import torch

from openvoice_amd import _lib, audio_io, se_extractor, vad

SR, H = 22050, 256
MIN_SIL, MIN_SPEECH, PAD = 87, 9, 3       # ceil(1.0 * 22050 / 256), ceil(0.1 * 22050 / 256), ceil(0.03 * 22050 / 256)


def _runs(flags, value):
    out, i = [], 0
    while i < len(flags):
        if flags[i] == value:
            j = i
            while j < len(flags) and flags[j] == value:
                j += 1
            out.append((i, j))
            i = j
        else:
            i += 1
    return out


def brute_force_mask(x, sr=SR, hop=H, range_db=35.0, floor_db=-55.0, min_silence_s=1.0, min_speech_s=0.1, pad_s=0.03):
    """The issue's six steps, one loop each, float64 energies."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    T = -(-N // hop)
    min_sil, min_speech, pad = (math.ceil(min_silence_s * sr / hop), math.ceil(min_speech_s * sr / hop),
                                math.ceil(pad_s * sr / hop))
    if T == 0:
        return np.zeros(0, dtype=bool)
    e = [float(np.mean(x[t * hop:min(N, t * hop + 2 * hop)] ** 2)) for t in range(T)]
    thr = max(10.0 ** (floor_db / 10.0), max(e) * 10.0 ** (-range_db / 10.0))
    a = [v > thr for v in e]
    for i, j in _runs(a, False):                      # close gaps between two active frames
        if i > 0 and j < T and j - i < min_sil:
            a[i:j] = [True] * (j - i)
    for i, j in _runs(a, True):                       # drop blips
        if j - i < min_speech:
            a[i:j] = [False] * (j - i)
    kept = [False] * T
    for i, j in _runs(a, True):                       # pad
        for k in range(max(0, i - pad), min(T, j + pad)):
            kept[k] = True
    return np.array(kept, dtype=bool)


def _signal(frame_flags, last_frame_samples=H, seed=0):
    """A waveform whose frame t is loud noise where frame_flags[t] and -80 dBFS noise elsewhere.  (A frame's energy
    window reaches one hop ahead, so the raw-active frames are the flagged hops and the hop before each run.)"""
    rng = np.random.default_rng(seed)
    T = len(frame_flags)
    x = 1e-4 * rng.standard_normal(T * H)
    for i, j in _runs(list(frame_flags), True):
        x[i * H:j * H] += 0.3 * rng.standard_normal((j - i) * H)
    return x[:(T - 1) * H + last_frame_samples].astype(np.float32)


def _flags(*runs):
    out = []
    for on, length in runs:
        out += [bool(on)] * length
    return out


CASES = {
    # (a run of flagged hops of length L is L + 1 raw-active frames; a gap of G unflagged hops is G - 1 silent frames)
    "gap_filled": _flags((1, 40), (0, MIN_SIL), (1, 40), (0, 5)),              # MIN_SIL - 1 silent frames
    "gap_kept": _flags((1, 40), (0, MIN_SIL + 1), (1, 40), (0, 5)),            # exactly MIN_SIL silent frames
    "blip_dropped": _flags((0, 120), (1, MIN_SPEECH - 2), (0, 120), (1, 30)),  # MIN_SPEECH - 1 active frames
    "blip_kept": _flags((0, 120), (1, MIN_SPEECH - 1), (0, 120), (1, 30)),     # exactly MIN_SPEECH active frames
    "leading_trailing": _flags((0, 50), (1, 60), (0, 70)),
    "pad_clipped": _flags((0, 2), (1, 30), (0, 100), (1, 30), (0, 1)),
    "all_active": _flags((1, 200)),
    "all_silent": _flags((0, 200)),
    "one_frame_loud": _flags((1, 1)),
    "one_frame_quiet": _flags((0, 1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("last", [H, 101, 1])
def test_host_restatement_equals_brute_force(name, last):
    x = _signal(CASES[name], last_frame_samples=last, seed=len(name))
    want = brute_force_mask(x)
    got = vad.speech_frames_host(x, SR, H)
    assert got.dtype == bool and got.shape == want.shape == (len(CASES[name]),)
    assert np.array_equal(got, want)


def test_the_hand_built_cases_exercise_what_they_claim():
    silent_runs = lambda m: [j - i for i, j in _runs(list(m), False)]
    filled = brute_force_mask(_signal(CASES["gap_filled"]))
    kept = brute_force_mask(_signal(CASES["gap_kept"]))
    assert filled[:80 + MIN_SIL].all() and not filled[-1]                    # the gap is gone, trailing silence is not
    assert (MIN_SIL - 2 * PAD) in silent_runs(kept)                          # the gap stays, less the pad on both sides
    dropped = brute_force_mask(_signal(CASES["blip_dropped"]))
    kept = brute_force_mask(_signal(CASES["blip_kept"]))
    assert not dropped[:200].any() and dropped[-20:].all()
    assert kept[:200].sum() == MIN_SPEECH + 2 * PAD
    lt = brute_force_mask(_signal(CASES["leading_trailing"]))
    assert not lt[:40].any() and not lt[-60:].any() and lt[50:109].all()
    clipped = brute_force_mask(_signal(CASES["pad_clipped"]))
    assert clipped[0] and clipped[-1]
    assert brute_force_mask(_signal(CASES["all_active"])).all()
    assert not brute_force_mask(_signal(CASES["all_silent"])).any()
    assert brute_force_mask(_signal(CASES["one_frame_loud"])).tolist() == [False]     # raw-active, but a blip
    assert brute_force_mask(_signal(CASES["one_frame_loud"]), min_speech_s=0.01).tolist() == [True]
    assert brute_force_mask(_signal(CASES["one_frame_quiet"])).tolist() == [False]


def test_host_restatement_on_random_run_patterns_and_other_parameters():
    rng = np.random.default_rng(11)
    for trial in range(60):
        runs = [(int(rng.integers(0, 2)), int(rng.choice([1, 2, 7, 8, 9, 10, 40, 86, 87, 88, 130]))) for _ in range(6)]
        x = _signal(_flags(*runs), last_frame_samples=int(rng.integers(1, H + 1)), seed=trial)
        assert np.array_equal(vad.speech_frames_host(x, SR, H), brute_force_mask(x)), runs
    kw = dict(range_db=20.0, floor_db=-40.0, min_silence_s=0.25, min_speech_s=0.05, pad_s=0.0)
    x = _signal(_flags((0, 30), (1, 3), (0, 20), (1, 50), (0, 25), (1, 50), (0, 9)), last_frame_samples=77)
    for sr, hop in ((22050, 256), (16000, 160), (48000, 512)):
        got = vad.speech_frames_host(x, sr, hop, vad.VadParams(**kw))
        assert np.array_equal(got, brute_force_mask(x, sr=sr, hop=hop, **kw))


def test_segments_and_host_removal():
    flags = CASES["gap_kept"]
    x = _signal(flags, last_frame_samples=101)
    mask = brute_force_mask(x)
    kept, segments = vad.remove_silence_host(x, SR, H)
    want_segments = [(i * H, min(len(x), j * H)) for i, j in _runs(list(mask), True)]
    assert segments == want_segments and len(segments) == 2
    assert np.array_equal(kept, np.concatenate([x[s:e] for s, e in want_segments]))
    assert kept.dtype == np.float32
    loud = _signal(CASES["all_active"], last_frame_samples=33)
    kept, segments = vad.remove_silence_host(loud, SR, H)
    assert np.array_equal(kept, loud) and segments == [(0, len(loud))]
    kept, segments = vad.remove_silence_host(_signal(CASES["all_silent"]), SR, H)
    assert len(kept) == 0 and segments == []


def test_parameter_validation():
    p = vad.VadParams()
    assert (p.range_db, p.floor_db, p.min_silence_s, p.min_speech_s, p.pad_s) == (35.0, -55.0, 1.0, 0.1, 0.03)
    assert p.frames(SR, H) == (MIN_SIL, MIN_SPEECH, PAD)
    assert p.linear() == (10.0 ** -5.5, 10.0 ** -3.5)
    for bad in (dict(range_db=0), dict(range_db=-3), dict(range_db=float("nan")), dict(floor_db=1.0),
                dict(floor_db=float("inf")), dict(min_silence_s=0), dict(min_speech_s=-0.1), dict(pad_s=-0.01),
                dict(pad_s="0.03"), dict(min_silence_s=None), dict(range_db=True)):
        with pytest.raises(ValueError):
            vad.VadParams(**bad)
    for sr, hop in ((0, 256), (22050.5, 256), (22050, 0), (22050, 255), (22050, -256)):
        with pytest.raises(ValueError):
            p.frames(sr, hop)
        with pytest.raises(ValueError):
            vad.speech_frames_host(np.zeros(10), sr, hop)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built (run __graft_entry__.build())")
def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.ov_version() >= 212
    P = 0x10000                      # never dereferenced: every call below is refused before a launch
    E = -1
    energy = lambda pool=P, n=1000, rec=P, R=1, h=256, ldt=4, e=P: lib.ov_vad_frame_energy_f32(pool, n, rec, R, h, ldt, e, None)
    assert energy(pool=None) == E and energy(rec=None) == E and energy(e=None) == E
    assert energy(R=0) == E and energy(R=-1) == E and energy(n=0) == E
    assert energy(h=0) == E and energy(h=-256) == E and energy(h=254) == E and energy(ldt=0) == E and energy(ldt=-1) == E

    def segments(e=P, rec=P, R=1, h=256, ldt=4, floor=1e-5, rng=1e-3, sil=87, sp=9, pad=3, m=P, o=P, na=P):
        return lib.ov_vad_segments_i32(e, rec, R, h, ldt, floor, rng, sil, sp, pad, m, o, na, None)
    assert segments(e=None) == E and segments(rec=None) == E and segments(m=None) == E and segments(o=None) == E
    assert segments(na=None) == E and segments(R=0) == E and segments(h=6) == E and segments(h=0) == E
    assert segments(ldt=0) == E and segments(sil=0) == E and segments(sp=0) == E and segments(sp=-2) == E
    assert segments(pad=-1) == E and segments(floor=-1.0) == E and segments(rng=float("nan")) == E

    def compact(pool=P, n=1000, rec=P, R=1, h=256, ldt=4, m=P, o=P, ob=P, out=P, on=1000):
        return lib.ov_vad_compact_f32(pool, n, rec, R, h, ldt, m, o, ob, out, on, None)
    assert compact(pool=None) == E and compact(rec=None) == E and compact(m=None) == E and compact(o=None) == E
    assert compact(ob=None) == E and compact(out=None) == E and compact(R=0) == E and compact(h=2) == E
    assert compact(h=0) == E and compact(ldt=0) == E and compact(n=0) == E and compact(on=0) == E


class _StubModel:
    """What get_se needs of a converter: version, hps.data, device and an extract_se that records its input."""
    version = "v2"
    device = "cpu"

    def __init__(self):
        from openvoice_amd.utils import default_converter_hparams
        self.hps = default_converter_hparams("v2")
        self.calls = []

    def extract_se(self, ref_wav_list, se_save_path=None):
        self.calls.append((list(ref_wav_list), se_save_path))
        return torch.zeros(1, 256, 1)


@pytest.fixture
def host_vad(monkeypatch):
    def remove_silence(wave, sr, hop, params=None):
        kept, segments = vad.remove_silence_host(wave.cpu().numpy(), sr, hop, params)
        return torch.from_numpy(np.ascontiguousarray(kept)), segments
    monkeypatch.setattr(vad, "remove_silence", remove_silence)


def _recording(tmp_path, flags, name="ref.wav"):
    x = _signal(flags, seed=5)
    audio_io.write(str(tmp_path / name), x, SR)
    decoded, _ = audio_io.load(str(tmp_path / name), SR)
    return str(tmp_path / name), decoded


def test_get_se_cuts_the_active_audio_into_the_reference_layout(tmp_path, host_vad, capsys):
    hops_per_s = SR / H
    flags = _flags((0, int(3 * hops_per_s)), (1, int(14 * hops_per_s)), (0, int(6 * hops_per_s)), (1, int(9 * hops_per_s)),
                   (0, int(4 * hops_per_s)))
    path, decoded = _recording(tmp_path, flags)
    mask = brute_force_mask(decoded)
    n_active = int(np.repeat(mask, H)[:len(decoded)].sum())
    want_pieces = int(np.round(n_active / SR / 10.0))
    assert want_pieces == 2 and int(np.round(len(decoded) / SR / 10.0)) == 4       # silence removal changes the count
    model = _StubModel()
    se, name = se_extractor.get_se(path, model, target_dir=str(tmp_path / "processed"), vad=True)
    assert se.shape == (1, 256, 1) and name.startswith("ref_v2_")
    wavs = tmp_path / "processed" / name / "wavs"
    files = sorted(os.listdir(wavs))
    assert files == [f"{name}_seg{i}.wav" for i in range(want_pieces)]
    assert model.calls == [([str(wavs / f) for f in files], str(tmp_path / "processed" / name / "se.pth"))]
    pieces = [audio_io.load(str(wavs / f), SR)[0] for f in files]
    assert sum(len(p) for p in pieces) == n_active
    assert np.array_equal(np.concatenate(pieces), decoded[np.repeat(mask, H)[:len(decoded)]])
    assert f"after vad: dur = {n_active / SR}" in capsys.readouterr().out
    # vad=False keeps the equal cut of the raw recording
    model2 = _StubModel()
    _, name2 = se_extractor.get_se(path, model2, target_dir=str(tmp_path / "raw"), vad=False)
    raw_files = sorted(os.listdir(tmp_path / "raw" / name2 / "wavs"))
    assert name2 == name and len(raw_files) == 4
    assert sum(len(audio_io.load(str(tmp_path / "raw" / name2 / "wavs" / f), SR)[0]) for f in raw_files) == len(decoded)


def test_split_audio_vad_keeps_the_reference_signature_and_refuses_short_input(tmp_path, host_vad):
    import inspect
    params = list(inspect.signature(se_extractor.split_audio_vad).parameters.values())
    assert [p.name for p in params[:6]] == ["audio_path", "audio_name", "target_dir", "split_seconds", "sampling_rate",
                                            "device"]
    assert params[3].default == 10.0 and params[4].default is None and params[5].default is None
    hops_per_s = SR / H
    path, _ = _recording(tmp_path, _flags((0, int(10 * hops_per_s)), (1, int(3 * hops_per_s)), (0, int(7 * hops_per_s))))
    with pytest.raises(AssertionError, match="input audio is too short"):
        se_extractor.split_audio_vad(path, "short", str(tmp_path / "out"), device="cpu")
    with pytest.raises(AssertionError, match="input audio is too short"):
        se_extractor.get_se(path, _StubModel(), target_dir=str(tmp_path / "out2"))
    # an all-active recording is cut exactly as split_audio_equal cuts it
    path, decoded = _recording(tmp_path, _flags((1, int(21 * hops_per_s))), name="loud.wav")
    a = se_extractor.split_audio_vad(path, "loud", str(tmp_path / "a"), sampling_rate=SR, device="cpu")
    b = se_extractor.split_audio_equal(path, "loud", str(tmp_path / "b"), SR)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["loud_seg0.wav", "loud_seg1.wav"]
    for f in os.listdir(a):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()
