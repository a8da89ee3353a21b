"""``openvoice_amd.mp3``: the from-scratch MPEG-1 Layer III decoder behind ``audio_io.load`` (reference call sites
openvoice/api.py:123,144: ``librosa.load`` on resources/*.mp3 -- BASELINE.json configs[0] as written) against golden PCM
from a real decoder: FFmpeg inside the image's bundled Chromium (oracle/make_mp3_golden.py -> tests/golden/mp3_*.npz).
The input files are stored beside their golden PCM (tests/golden/mp3_<name>.mp3, pinned by sha256): kaleido's
``invalid_keypress.mp3`` (stereo / joint stereo, short + long blocks) and the reference's own resources/*.mp3 (mono VBR
with a LAME header, 128 kbit/s joint stereo without one).  Bars: identical sample count (gapless trimming included), max-abs
1e-4 on three 8192-sample excerpts (FFmpeg's decoder here is the fixed-point one: 16-bit PCM, 1 LSB = 3.05e-5), block RMS
of the WHOLE file within 2e-5."""
import hashlib
import os

import numpy as np
import pytest

from openvoice_amd import audio_io, mp3

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {n: os.path.join(GOLDEN, f"mp3_{n}.mp3") for n in ("invalid_keypress", "example_reference", "demo_speaker0",
                                                             "demo_speaker1", "demo_speaker2")}


def _load(name):
    path = CASES[name]
    g = np.load(os.path.join(GOLDEN, f"mp3_{name}.npz"))
    with open(path, "rb") as fh:
        data = fh.read()
    assert hashlib.sha256(data).hexdigest() == str(g["sha256"]), f"{path} is not the file the golden vectors were made from"
    return data, g


@pytest.mark.parametrize("name", list(CASES))
def test_decoder_matches_ffmpeg_golden(name):
    data, g = _load(name)
    pcm, rate = mp3.decode(data)
    assert rate == int(g["rate"]) and pcm.dtype == np.float32
    assert pcm.shape == (int(g["channels"]), int(g["samples"]))          # incl. the LAME delay / padding trim
    for k, off in enumerate(g["offsets"]):
        want = g["excerpts"][k]
        got = pcm[:, off:off + want.shape[1]]
        assert np.abs(got - want[:, :got.shape[1]]).max() <= 1e-4, (name, k)
    nb = g["block_rms"].shape[1]
    rms = np.sqrt((pcm[:, :nb * 1152].reshape(pcm.shape[0], nb, 1152).astype(np.float64) ** 2).mean(-1))
    assert np.abs(rms - g["block_rms"]).max() <= 2e-5
    if g["full"].size:
        assert np.abs(pcm - g["full"]).max() <= 1e-4


def test_probe_and_gapless_fields():
    data, g = _load("invalid_keypress")
    info = mp3.probe(data)
    assert info["sample_rate"] == 44100 and info["channels"] == 2 and info["xing"] and info["frames"] == 21
    assert info["start_pad"] == 576
    raw, _ = mp3.decode(data, trim_gapless=False)
    assert raw.shape[1] == 21 * 1152                                      # the header frame itself is not audio
    cut, _ = mp3.decode(data)
    # FFmpeg's rule: skip start_pad + 528 + 1 samples, stop at frames * 1152 - end_pad + 528 + 1 (or the stream's end)
    assert cut.shape[1] == min(21 * 1152, 21 * 1152 - info["end_pad"] + 529) - (info["start_pad"] + 529) == int(g["samples"])
    assert np.array_equal(cut, np.clip(raw[:, 576 + 529:576 + 529 + cut.shape[1]], -1, 1))


def test_unsupported_streams_are_named():
    with pytest.raises(mp3.Mp3Error, match="unsupported format: no MPEG audio Layer III frame"):
        mp3.decode(b"\x00" * 4000)
    # a Layer II stream (MPEG-1, 44.1 kHz, 128 kbit/s: 417-byte frames) and a Layer I stream (32-bit slots: 384 kbit/s =
    # 104 slots = 416 bytes): named as such once a second consistent header confirms it is a stream
    for hdr, flen in ((bytes([0xFF, 0xFD, 0x80, 0x00]), 144000 * 128 // 44100), (bytes([0xFF, 0xFF, 0xC0, 0x00]), (12000 * 384 // 44100) * 4)):
        stream = b"".join(hdr + bytes(flen - 4) for _ in range(6))
        with pytest.raises(mp3.Mp3Error, match="only Layer III"):
            mp3.decode(stream)
    # ... but a lone Layer II-looking pattern in front of a Layer III stream is just junk
    data, _ = _load("invalid_keypress")
    full, _ = mp3.decode(data)
    got, _ = mp3.decode(bytes([0xFF, 0xFD, 0x80, 0x00]) + bytes(100) + data)
    assert np.array_equal(got, full)


SYN_CASES = ["mpeg1_44100_mono_reservoir", "mpeg1_48000_stereo_ms", "mpeg1_32000_mono"]


@pytest.mark.parametrize("name", SYN_CASES)
def test_synthetic_mpeg1_streams_match_ffmpeg_golden(name):
    """MPEG-1 corners the real files do not reach -- mixed blocks, random scfsi patterns, the preflag bit, both count1
    tables, a bit reservoir used to its 511-byte limit, the padding bit, 32 and 48 kHz -- on synthetic bitstreams written by
    oracle/make_mp3_synthetic_golden.py and decoded by FFmpeg (Chromium); stream + decode are in the fixture."""
    g = np.load(os.path.join(GOLDEN, f"mp3_syn_{name}.npz"))
    data, want = bytes(g["stream"]), g["pcm"]
    pcm, rate = mp3.decode(data)
    assert rate == int(g["rate"]) and pcm.shape == want.shape == (int(g["channels"]), 50 * 1152)
    assert np.abs(want).max() > 0.02 and np.abs(pcm - want).max() <= 1e-4


INTENSITY_CASES = ["mpeg1_44100_intensity", "mpeg1_32000_intensity", "mpeg2_22050_intensity", "mpeg2_16000_intensity",
                   "mpeg25_11025_intensity"]


@pytest.mark.parametrize("name", INTENSITY_CASES)
def test_intensity_stereo_streams_match_ffmpeg_golden(name, monkeypatch):
    """Joint stereo with INTENSITY coding (mode_extension bit 0), with and without MS, in every block kind incl. mixed:
    MPEG-1 (positions 0..6, tan(pos pi / 12) ratios) and LSF (the right channel's own scalefac_compress coding, intensity
    scale, 2^(-k / 4) and 2^(-k / 2) steps; positions >= 16 illegal as FFmpeg reads them).  Synthetic bitstreams again: the
    left channel's spectrum reaches far up, the right channel's ends early and its factors above are random positions,
    legal and illegal.  The fixture's decode is FFmpeg's (Chromium); a decoder that skips the intensity step is 1e-3 ..
    7e-3 off on these streams, 30 - 200 x the bar."""
    g = np.load(os.path.join(GOLDEN, f"mp3_syn_{name}.npz"))
    data, want = bytes(g["stream"]), g["pcm"]
    calls = []
    real = mp3._joint_stereo
    monkeypatch.setattr(mp3, "_joint_stereo", lambda *a: (calls.append((a[2]["block_type"], a[2]["mixed"], a[7])), real(*a))[1])
    pcm, rate = mp3.decode(data)
    assert rate == int(g["rate"]) and pcm.shape == want.shape and pcm.shape[0] == 2
    assert np.abs(want).max() > 0.02 and np.abs(pcm - want).max() <= 1e-4
    kinds = set(calls)
    assert len(calls) >= 40 and {k[0] for k in kinds} == {0, 1, 2, 3} and {k[2] for k in kinds} == {False, True}
    assert any(k[1] for k in kinds)                                       # mixed blocks too


LSF_CASES = ["mpeg2_22050_mono", "mpeg2_24000_stereo_ms", "mpeg2_16000_mono", "mpeg25_11025_stereo", "mpeg25_12000_mono"]


@pytest.mark.parametrize("name", LSF_CASES)
def test_lsf_streams_match_ffmpeg_golden(name):
    """MPEG-2 (16 / 22.05 / 24 kHz) and MPEG-2.5 (11.025 / 12 kHz) Layer III -- the LSF syntax of ISO/IEC 13818-3: one granule
    per frame, 9-bit scalefac_compress with its three ranges and the bands-per-partition table, no scfsi, its own band
    tables.  No LSF file exists in the image and nothing here encodes audio, so the vectors are SYNTHETIC BITSTREAMS written
    frame by frame by oracle/make_mp3_synthetic_golden.py (random spectra incl. escape values and count1 quadruples, scale
    factors, every block kind in legal window sequences, random region splits and table selections, MS stereo) and decoded
    by FFmpeg inside the image's Chromium; stream and decode are both in the fixture, so this runs everywhere.  Bar: 1e-4
    (FFmpeg's decoder there is the fixed-point one: 1 LSB of 16-bit PCM = 3.05e-5)."""
    g = np.load(os.path.join(GOLDEN, f"mp3_lsf_{name}.npz"))
    data, want = bytes(g["stream"]), g["pcm"]
    info = mp3.probe(data)
    assert info["lsf"] and info["sample_rate"] == int(g["rate"]) and info["channels"] == int(g["channels"])
    pcm, rate = mp3.decode(data)
    assert rate == int(g["rate"]) and pcm.shape == want.shape and pcm.shape[1] == 60 * 576
    assert np.abs(want).max() > 0.02                                      # a real signal (650+ LSB of 16-bit PCM), not silence
    assert np.abs(pcm - want).max() <= 1e-4


def test_audio_io_load_decodes_mp3_like_librosa_load(tmp_path):
    """``audio_io.load(path, sr)`` = decode, channel mean (librosa.to_mono), kaiser_best resampling to ``sr``."""
    data, g = _load("invalid_keypress")
    y, sr = audio_io.load(CASES["invalid_keypress"], 22050)
    assert sr == 22050 and y.dtype == np.float32 and y.ndim == 1
    assert len(y) == int(np.ceil(int(g["samples"]) * 22050 / 44100))
    mono = g["full"].astype(np.float64).mean(0)
    want = audio_io.resample_kaiser_best(mono, 44100, 22050)
    assert np.abs(y - want).max() <= 1e-4 and np.abs(y).max() > 0.1
    wav = tmp_path / "x.wav"                                               # and WAV still goes through the RIFF reader
    audio_io.write(str(wav), y, sr)
    z, _ = audio_io.load(str(wav), sr)
    assert np.abs(z - y).max() <= 1.0 / 32768


def test_configs0_input_decodes_to_the_model_rate():
    """BASELINE.json configs[0] names resources/example_reference.mp3: 58.8 s of mono speech at 44.1 kHz, VBR."""
    data, g = _load("example_reference")
    y, sr = audio_io.load(CASES["example_reference"], 22050)
    assert sr == 22050 and abs(len(y) / sr - int(g["samples"]) / 44100) < 1e-3
    assert 0.3 < np.abs(y).max() <= 1.0 and np.isfinite(y).all()


def test_truncated_prefixed_and_corrupted_streams_decode_without_surprises():
    """A stream cut mid-frame decodes its whole frames (bit-identical to the full decode there); junk before the first frame
    and an ID3v1 tag after the last are skipped; corrupted bytes yield finite, clipped samples, not an exception."""
    data, _ = _load("invalid_keypress")
    full, _ = mp3.decode(data)
    for cut in (len(data) - 100, len(data) // 2, 3000):
        part, _ = mp3.decode(data[:cut])
        assert 0 < part.shape[1] < full.shape[1] and np.array_equal(part, full[:, :part.shape[1]])
    wrapped, _ = mp3.decode(b"\x00\x12junk" + data + b"TAG" + bytes(125))
    assert np.array_equal(wrapped, full)
    broken = bytearray(data)
    broken[4000] ^= 0xFF
    broken[4001] ^= 0x55
    pcm, _ = mp3.decode(bytes(broken))
    assert pcm.shape == full.shape and np.isfinite(pcm).all() and np.abs(pcm).max() <= 1.0


def test_c_huffman_core_and_python_form_decode_identically(monkeypatch):
    """The Huffman decoding runs in C when ``libov_mp3.so`` is built (csrc/mp3_core.c, part of ``make`` /
    ``__graft_entry__.build()``) and in Python otherwise: same tables, same bit positions, bit-identical PCM -- on a real
    joint-stereo file and on synthetic streams with escape values, all block kinds and both count1 tables."""
    if mp3._core() is None:
        pytest.skip("libov_mp3.so is not built")
    streams = [open(p, "rb").read() for p in (CASES["invalid_keypress"],) if os.path.exists(p)]
    for name in ("mp3_syn_mpeg1_48000_stereo_ms", "mp3_lsf_mpeg25_11025_stereo", "mp3_syn_mpeg2_16000_intensity"):
        streams.append(bytes(np.load(os.path.join(GOLDEN, f"{name}.npz"))["stream"]))
    for data in streams:
        with_core, rate = mp3.decode(data)
        monkeypatch.setenv("OPENVOICE_AMD_MP3_CORE", "0")
        assert mp3._core() is None
        in_python, rate2 = mp3.decode(data)
        monkeypatch.delenv("OPENVOICE_AMD_MP3_CORE")
        assert rate == rate2 and np.array_equal(with_core, in_python)


def test_binary_trailers_damaged_headers_and_foreign_files(tmp_path):
    """a header-looking byte pattern is a frame only when the stream continues consistently behind
    it.  (a) 30 KB of random bytes after the last frame (an APEv2 tag, cover art) decode like the clean file -- FFmpeg /
    librosa accept such files; (b) one flipped byte in ANY frame header costs that frame, never the file; (c) random bytes
    and other containers (FLAC / OGG / M4A magic) get the 'unsupported format' error, not a Layer I / II message."""
    from openvoice_amd import audio_io
    data, _ = _load("invalid_keypress")
    full, rate = mp3.decode(data)
    for seed in range(10):
        rng = np.random.default_rng(seed)
        pcm, r = mp3.decode(data + rng.integers(0, 256, 30000, dtype=np.uint8).tobytes())
        assert r == rate and pcm.shape[1] >= full.shape[1] and np.array_equal(pcm[:, :full.shape[1]], full)
        assert pcm.shape[1] - full.shape[1] <= 4 * 1152          # (a chance pair of consistent headers in the noise, at most)
    first = mp3.probe(data)["first_frame"]
    headers = [p for p in range(first, len(data) - 4) if mp3._confirmed(data, p, mp3._header(data, p))
               and mp3._same_stream(mp3._header(data, p), mp3._header(data, first))]
    rng = np.random.default_rng(99)
    for _ in range(60):
        pos = int(rng.choice(headers[1:])) + int(rng.integers(0, 4))
        broken = bytearray(data)
        broken[pos] ^= 1 << int(rng.integers(0, 8))
        pcm, r = mp3.decode(bytes(broken))                        # never raises
        assert r == rate and np.isfinite(pcm).all() and abs(pcm.shape[1] - full.shape[1]) <= 2 * 1152
    for magic in (b"fLaC", b"OggS", b"\x00\x00\x00\x20ftypM4A ", b"\x1aE\xdf\xa3"):
        path = tmp_path / "x.bin"
        path.write_bytes(magic + np.random.default_rng(5).integers(0, 256, 50000, dtype=np.uint8).tobytes())
        with pytest.raises(mp3.Mp3Error, match="unsupported format"):
            audio_io.read_native(str(path))


def test_python_huffman_reads_zeros_past_the_buffer_like_the_c_core(monkeypatch):
    """corrupt big_values / linbits run past the granule's bytes; both forms read zeros there."""
    assert mp3._bit(b"\x80", 0) == 1 and mp3._bit(b"\x80", 7) == 0 and mp3._bit(b"\x80", 8) == 0 and mp3._bit(b"", 123) == 0
    data, _ = _load("invalid_keypress")
    rng = np.random.default_rng(3)
    for _ in range(8):
        broken = bytearray(data)
        for p in rng.integers(600, len(data) - 600, 12):          # side-information / main-data bytes at random
            broken[int(p)] = int(rng.integers(0, 256))
        with_core, _ = mp3.decode(bytes(broken))
        monkeypatch.setenv("OPENVOICE_AMD_MP3_CORE", "0")
        in_python, _ = mp3.decode(bytes(broken))
        monkeypatch.delenv("OPENVOICE_AMD_MP3_CORE")
        assert np.array_equal(with_core, in_python)
