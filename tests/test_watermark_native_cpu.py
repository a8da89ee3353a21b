"""The native watermark's definition (``openvoice_amd/watermark.py``) through its float64 mirror: the round trip is exact
by construction, the mirror works behind the converter's unchanged hook, the mark survives a 16-bit WAV and white noise
30 dB down, and the chips are single bits of ``noise.philox4x32_10``.  No kernel is launched."""
import numpy as np
import pytest
import torch

from openvoice_amd import api, audio_io, noise, watermark

L = 16000
PAYLOADS = [0x00000000, 0xFFFFFFFF, 0xA5A5A5A5]


def _bits(word):
    return np.array([(word >> j) & 1 for j in range(32)], dtype=np.float64)


def _inputs():
    gen = np.random.default_rng(2024)
    t = np.arange(L) / 22050.0
    return {"noise": gen.standard_normal(L), "sine": 0.3 * np.sin(2 * np.pi * 220.0 * t), "zero": np.zeros(L),
            "tiny": 1e-5 * gen.standard_normal(L)}


@pytest.mark.parametrize("payload", PAYLOADS)
@pytest.mark.parametrize("name", ["noise", "sine", "zero", "tiny"])
def test_mirror_round_trip_is_exact_by_construction(name, payload):
    """Every bit's projection reaches the level the window was marked at, b_j q_j >= a (1 - 1e-9), and reads back."""
    x = _inputs()[name]
    bits = _bits(payload)
    y = watermark.encode_host(x, bits[None])
    assert y.shape == x.shape and y.dtype == np.float64
    _, a = watermark.read_host(x)                       # the level the mark was embedded at
    q, _ = watermark.read_host(y)
    b = 2.0 * bits - 1.0
    assert np.all(b * q[0] >= a[0] * (1.0 - 1e-9)), (b * q[0] / a[0]).min()
    assert np.array_equal(watermark.decode_host(y)[0] >= 0.5, bits == 1)
    if name in ("zero", "tiny"):
        assert a[0] == watermark.DEFAULT_FLOOR           # the floor carries a window this quiet
    else:
        assert a[0] == pytest.approx(0.02 * np.sqrt(np.mean(x * x)), rel=1e-12)


def test_a_bit_the_audio_already_carries_is_left_alone_and_an_unmarked_silent_window_scores_one_half():
    x = _inputs()["noise"]
    p, a = watermark.read_host(x)
    strong = np.abs(p[0]) >= a[0]
    bits = (p[0] > 0).astype(np.float64)                # ask for the signs the window already has
    y = watermark.encode_host(x, bits[None])
    untouched = np.isin(np.arange(L) % 32, np.nonzero(strong)[0])
    assert strong.any() and np.array_equal(y[untouched], x[untouched])
    assert np.array_equal(watermark.decode_host(np.zeros(L)), np.full((1, 32), 0.5))


def test_windows_shorter_than_512_samples_and_bad_parameters_are_value_errors():
    with pytest.raises(ValueError, match="512"):
        watermark.encode_host(np.zeros(511), np.zeros((1, 32)))
    watermark.encode_host(np.zeros(512), np.zeros((1, 32)))
    with pytest.raises(ValueError, match="512"):
        watermark.check_records([(0, 0, 511, 0)], 16000, 16000)
    with pytest.raises(ValueError, match="leaves its buffer"):
        watermark.check_records([(1, 0, 16000, 0)], 16000, 16000)
    with pytest.raises(ValueError, match="leaves its buffer"):
        watermark.check_records([(0, 1, 16000, 0)], 16000, 16000)
    assert watermark.check_records([(0, 1, 16000, 0)], 16000) == [(0, 1, 16000, 0)]       # the reader ignores dst_off
    for kw in ({"key": -1}, {"key": 1 << 63}, {"key": 1.5}, {"strength": -0.1}, {"floor": 0.0}):
        with pytest.raises(ValueError):
            watermark.NativeWatermark(**kw)
    with pytest.raises(ValueError, match="no CPU path"):
        watermark.NativeWatermark().encode(torch.zeros(1, L), torch.zeros(1, 32))


# ---- behind the unchanged hook --------------------------------------------------------------------------------------
class HostModel:
    """The float64 mirror behind wavmark's interface, on host tensors."""

    def __init__(self, **kw):
        self.wm = watermark.NativeWatermark(**kw)

    def encode(self, signal, bits):
        assert signal.shape == (1, L) and bits.shape == (1, 32)
        return torch.from_numpy(self.wm.encode_host(signal.numpy(), bits.numpy())).float()

    def decode(self, signal):
        return torch.from_numpy(self.wm.decode_host(signal.numpy()))


def _converter(model):
    conv = object.__new__(api.ToneColorConverter)      # the hook needs neither weights nor a GPU
    conv.device = "cpu"
    conv.watermark_model = model
    return conv


def _marked(scale=0.1, seed=7, message="openAI!?", **kw):
    conv = _converter(HostModel(**kw))
    audio = (scale * np.random.default_rng(seed).standard_normal(80000)).astype(np.float32)
    before = audio.copy()
    assert conv.add_watermark(audio, message) is audio
    return conv, before, audio


def test_the_mirror_works_behind_the_unchanged_hook():
    assert (watermark.WINDOW, watermark.STRIDE, watermark.BITS) == (
        api.ToneColorConverter.WATERMARK_WINDOW, api.ToneColorConverter.WATERMARK_STRIDE,
        api.ToneColorConverter.WATERMARK_GROUP_BITS)
    conv, before, audio = _marked(scale=1.0)
    assert conv.detect_watermark(audio, 2) == "openAI!?"
    untouched = np.ones(80000, bool)
    untouched[0:16000] = untouched[32000:48000] = False
    assert np.array_equal(audio[untouched], before[untouched])
    assert not np.array_equal(audio[~untouched], before[~untouched])
    # another key reads something else: the chips are keyed
    assert _converter(HostModel(key=1)).detect_watermark(audio, 2) != "openAI!?"
    # the message's groups as payload words: bit j of word n is bit 32 n + j of the hook's bit string
    words = watermark.NativeWatermark.groups_of("openAI!?")
    flat = api.string_to_bits("openAI!?").reshape(-1)
    assert [[(w >> j) & 1 for j in range(32)] for w in words] == flat.reshape(2, 32).tolist()


def test_the_mark_survives_a_16_bit_wav(tmp_path):
    conv, _, audio = _marked(scale=0.1)
    path = str(tmp_path / "marked.wav")
    audio_io.write(path, audio, 22050)
    back, sr = audio_io.load(path, None)
    assert sr == 22050 and len(back) == len(audio) and not np.array_equal(back, audio)
    assert conv.detect_watermark(back, 2) == "openAI!?"
    # and a silent recording's mark, which only the floor carries
    silent = np.zeros(80000, dtype=np.float32)
    conv.add_watermark(silent, "openAI!?")
    audio_io.write(path, silent, 22050)
    assert conv.detect_watermark(audio_io.load(path, None)[0], 2) == "openAI!?"


def test_the_mark_survives_white_noise_30_db_down():
    """Noise at -30 dB of a window's rms moves a projection by rms 10^(-30/20) / sqrt(500) = 1.4e-3 rms (one standard
    deviation); the mark stands at 0.02 rms: 14 standard deviations per bit, a condition on the scheme, not a chance
    event."""
    conv, _, audio = _marked(scale=0.1)
    gen = np.random.default_rng(99)
    noisy = audio.copy()
    for lo in (0, 32000):
        rms = np.sqrt(np.mean(audio[lo:lo + L].astype(np.float64) ** 2))
        noisy[lo:lo + L] += (rms * 10.0 ** (-30.0 / 20.0) * gen.standard_normal(L)).astype(np.float32)
    assert conv.detect_watermark(noisy, 2) == "openAI!?"
    q, a = watermark.read_host(noisy[:L])
    b = 2.0 * api.string_to_bits("openAI!?").reshape(-1)[:32] - 1.0
    print(f"smallest margin after noise: {(b * q[0]).min() / a[0]:.3f} of the level")
    assert np.all(b * q[0] > 0)


# ---- the chips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [0, 1, (1 << 63) - 1, 0x123456789ABCDEF])
def test_chips_are_single_bits_of_the_projects_philox(key):
    assert noise.PURPOSE_WATERMARK == 3 and noise.PURPOSE_WATERMARK not in (
        noise.PURPOSE_POSTERIOR, noise.PURPOSE_TTS_W, noise.PURPOSE_TTS_Z)
    c = watermark.chips_host(key, L)
    assert c.shape == (L,) and set(np.unique(c)) == {-1.0, 1.0}
    for i in (0, 1, 31, 32, 127, 128, 255, 4095, 15999):
        r = noise.philox4x32_10((i // 128, 0, 0, 3), (key & 0xFFFFFFFF, key >> 32))
        bit = (int(r[(i % 128) // 32]) >> (i % 32)) & 1
        assert c[i] == (1.0 if bit else -1.0), i
    assert abs(c.mean()) < 4.0 / np.sqrt(L)             # balanced, as single bits of a good generator are
    assert np.array_equal(watermark.chips_host(key, 777), c[:777])      # a chip depends on key and i only
