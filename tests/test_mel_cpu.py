"""CPU side of the mel / general STFT surface (openvoice_amd/mel_processing.py): the alias package's imports, the Slaney
filterbank written from its definition (parity with librosa is unpinned: librosa is not a dependency), the CPU-tensor
paths, the float64 mirrors against ``torch.stft``, the packed weight table, and the ABI of the new entry points.  No
kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from openvoice_amd import _lib
from openvoice_amd import mel_processing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ov_stft_mag_f32", "ov_stft_tile_frames", "ov_mel_log_f32")
SETS = [(22050, 1024, 80, 0, None), (16000, 400, 40, 20, 7600)]


def test_alias_package_exports_the_whole_reference_module():
    from openvoice.mel_processing import (dynamic_range_compression_torch, dynamic_range_decompression_torch,  # noqa: F401
                                          mel_spectrogram_torch, spec_to_mel_torch, spectral_de_normalize_torch,
                                          spectral_normalize_torch, spectrogram_torch)
    assert mel_spectrogram_torch is mp.mel_spectrogram_torch and spectrogram_torch is mp.spectrogram_torch


def test_mel_scale_closed_form_points_and_inverse():
    """0 Hz = 0 mel, 1000 Hz = 15 mel (3 mel per 200 Hz), 6400 Hz = 15 + 27 = 42 mel (ln(6.4) / 27 per mel), and back;
    1e-9 relative, so that the helpers need not be exact."""
    hz, mel = np.array([0.0, 1000.0, 6400.0]), np.array([0.0, 15.0, 42.0])
    assert np.all(np.abs(mp.hz_to_mel(hz) - mel) <= 1e-9 * np.maximum(mel, 1))
    assert np.all(np.abs(mp.mel_to_hz(mel) - hz) <= 1e-9 * np.maximum(hz, 1))
    f = np.array([3.0, 200.0, 999.0, 1001.0, 5000.0, 11025.0])
    assert np.all(np.abs(mp.mel_to_hz(mp.hz_to_mel(f)) - f) <= 1e-9 * f)


@pytest.mark.parametrize("sr,n_fft,num_mels,fmin,fmax", SETS)
def test_mel_filterbank_shape_support_peaks_and_area(sr, n_fft, num_mels, fmin, fmax):
    fb = mp.mel_filterbank(sr, n_fft, num_mels, fmin, fmax)
    bins = n_fft // 2 + 1
    assert fb.shape == (num_mels, bins) and fb.dtype == np.float64
    assert (sr, n_fft, num_mels) != (22050, 1024, 80) or fb.shape == (80, 513)
    assert np.all(fb >= 0)
    top = sr / 2 if fmax is None else fmax
    centres = mp.mel_to_hz(np.linspace(mp.hz_to_mel(fmin), mp.hz_to_mel(top), num_mels + 2))
    width = sr / n_fft
    for m in range(num_mels):
        nz = np.flatnonzero(fb[m])
        if nz.size == 0:            # a triangle narrower than a bin can fall between two bin frequencies
            assert centres[m + 2] - centres[m] < 2 * width
            continue
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)), f"row {m}: support is not contiguous"
        row, peak = fb[m, nz[0]:nz[-1] + 1], int(np.argmax(fb[m]))
        d = np.sign(np.diff(row))
        assert np.all(d[:peak - nz[0]] > 0) and np.all(d[peak - nz[0]:] < 0), f"row {m} does not rise, then fall"
        assert abs(peak - centres[m + 1] / width) <= 1.0, f"row {m} peaks at bin {peak}, centre {centres[m + 1] / width}"
    # Slaney area normalisation: the continuous triangle has area 1, and sum_k row[k] * sr / n_fft is its trapezoid rule on
    # the bin grid.  The rule is exact on a linear piece, so the error comes from the three kinks alone, each at most
    # width^2 / 8 times its jump in slope.  With a = c1 - c0, b = c2 - c1 and the peak 2 / (a + b) the jumps are peak / a,
    # peak / a + peak / b and peak / b, which gives |area - 1| <= width^2 / (2 a b).  Measured once from this float64
    # definition over the filters wider than 8 bins: 6.9e-3 (set 1) and 7.0e-3 (set 2) at worst, 0.43 and 0.34 of the bound.
    a, b = np.diff(centres)[:-1], np.diff(centres)[1:]
    wide = (a + b) > 8 * width
    assert wide.any()
    area = fb.sum(axis=1) * width
    print(f"mel area: worst |area - 1| = {np.abs(area[wide] - 1).max():.3e}, "
          f"worst share of the bound {(np.abs(area[wide] - 1) / (width ** 2 / (2 * a * b))[wide]).max():.3f}")
    assert np.all(np.abs(area[wide] - 1) <= (width ** 2 / (2 * a * b))[wide] + 1e-12)


def test_mel_filterbank_rejects_bad_band_edges():
    with pytest.raises(ValueError):
        mp.mel_filterbank(22050, 1024, 80, 0, 12000)       # fmax > sr / 2
    with pytest.raises(ValueError):
        mp.mel_filterbank(22050, 1024, 80, 8000, 8000)     # fmin >= fmax
    with pytest.raises(ValueError):
        mp.mel_filterbank(22050, 1024, 80, 9000, 8000)


def _wave(B, N, seed=0):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(N, dtype=torch.float32) / 22050
    return 0.6 * torch.sin(2 * torch.pi * (200 + 300 * torch.arange(B)[:, None]) * t) + 0.05 * torch.randn(B, N, generator=gen)


def test_cpu_mel_spectrogram_is_the_composition():
    y = _wave(2, 5000)
    for center in (False, True):
        a = mp.mel_spectrogram_torch(y, 1024, 80, 22050, 256, 1024, 0, None, center=center)
        b = mp.spec_to_mel_torch(mp.spectrogram_torch(y, 1024, 22050, 256, 1024, center=center), 1024, 80, 22050, 0, None)
        assert a.shape == b.shape and a.shape[:2] == (2, 80)
        assert (a - b).abs().max().item() <= 1e-6
    fb = torch.from_numpy(mp.mel_filterbank(22050, 1024, 80, 0, None)).float()
    want = torch.log(torch.clamp(fb @ mp.spectrogram_torch(y, 1024, 22050, 256, 1024), min=1e-5))
    assert (mp.mel_spectrogram_torch(y, 1024, 80, 22050, 256, 1024, 0, None) - want).abs().max().item() <= 1e-6
    assert torch.equal(mp.stft_magnitude(y, 1024, 256, 1024), mp.spectrogram_torch(y, 1024, 22050, 256, 1024))


def test_normalize_round_trip_and_defaults():
    x = torch.tensor([1e-5, 3e-4, 0.5, 1.0, 77.0])
    back = mp.spectral_de_normalize_torch(mp.spectral_normalize_torch(x))
    assert torch.allclose(back, x, rtol=1e-6, atol=0)
    assert torch.equal(mp.spectral_normalize_torch(torch.zeros(3)), torch.full((3,), 1e-5).log())
    assert torch.allclose(mp.dynamic_range_compression_torch(x, C=2), torch.log(2 * x))
    assert torch.allclose(mp.dynamic_range_decompression_torch(torch.log(2 * x), C=2), x)


def test_filterbank_cache_is_not_keyed_on_fmax_alone():
    spec = mp.spectrogram_torch(_wave(1, 4000), 1024, 22050, 256, 1024)
    a = mp.spec_to_mel_torch(spec, 1024, 80, 22050, 0, 8000)
    b = mp.spec_to_mel_torch(spec, 1024, 40, 22050, 0, 8000)          # the reference would reuse the 80-row basis here
    c = mp.spec_to_mel_torch(spec, 1024, 80, 22050, 50, 8000)
    assert a.shape[1] == 80 and b.shape[1] == 40
    assert not torch.equal(a, c)
    fb = torch.from_numpy(mp.mel_filterbank(22050, 1024, 40, 0, 8000)).float()
    assert torch.equal(b, torch.log(torch.clamp(fb @ spec, min=1e-5)))


@pytest.mark.parametrize("n_fft,hop,win,center", [(64, 7, 50, True), (400, 160, 400, True), (1024, 320, 1024, False)])
def test_stft_host_mirror_is_torch_stft_in_float64(n_fft, hop, win, center):
    """Pins the double reflection (pad (n_fft - hop) / 2, then n_fft / 2 of THAT) and the centred short window.  With the
    unrounded weights the mirror and torch.stft differ by float64 rounding only; with the kernel's fp32-rounded weights
    by at most 2^-24 sum |w x| per component, which the returned bound covers n_fft + 4 times over."""
    y = _wave(2, 3001, seed=n_fft).double()
    want = mp._stft_torch(y, n_fft, hop, win, center).numpy()
    ref, lim = mp.stft_magnitude_host(y, n_fft, hop, win, center, exact_weights=True)
    assert ref.shape == want.shape == lim.shape
    assert np.abs(ref - want).max() <= 1e-10
    ref32, lim32 = mp.stft_magnitude_host(y, n_fft, hop, win, center)
    assert np.all(np.abs(ref32 - want) <= lim32 / (n_fft + 4) + 1e-12) and np.all(lim32 > 0)


def test_mel_host_mirror_and_bound():
    spec = np.abs(np.random.default_rng(0).standard_normal((2, 9, 5)))
    spec[:, :, 2] = 0
    mel = mp.mel_filterbank(16000, 16, 4, 0, None)
    ref, lim = mp.mel_log_host(spec, mel)
    assert ref.shape == lim.shape == (2, 4, 5)
    assert np.all(ref[:, :, 2] == np.log(np.float64(np.float32(1e-5))))
    assert np.allclose(ref, np.log(np.maximum(np.einsum("mf,bft->bmt", mel, spec), np.float32(1e-5))))
    assert np.all(lim >= 4 * 2.0 ** -24)
    _, wider = mp.mel_log_host(spec, mel, spec_lim=np.full_like(spec, 1e-4))
    assert np.all(wider >= lim) and np.any(wider > lim)


@pytest.mark.parametrize("n_fft,win", [(16, 16), (50, 20), (400, 400), (1024, 800)])
def test_packed_stft_weights_are_in_a_fragment_order(n_fft, win):
    """Record (bt * 2 + c) * G + g, lane l, element u holds fp32(W_c[32 bt + (l & 31)][8 g + 2 u + (l >> 5)]); rows beyond
    the bins and k beyond n_fft are zero."""
    pack = mp.pack_stft_weights(n_fft, win)
    bins, G = n_fft // 2 + 1, (n_fft + 7) // 8
    tiles = (bins + 31) // 32
    assert pack.dtype == np.float32 and pack.shape == (tiles * 2 * G * 256,)
    got = pack.reshape(tiles, 2, G, 64, 4)
    want = np.zeros((2, tiles * 32, 8 * G), dtype=np.float32)
    re, im = mp.stft_weights(n_fft, win)
    want[0, :bins, :n_fft], want[1, :bins, :n_fft] = re, im
    lane = np.arange(64)
    for bt in range(tiles):
        for c in range(2):
            for g in range(G):
                for u in range(4):
                    assert np.array_equal(got[bt, c, g, :, u], want[c, 32 * bt + (lane & 31), 8 * g + 2 * u + (lane >> 5)])
    w = mp.stft_window(n_fft, win)
    left = (n_fft - win) // 2
    assert np.allclose(w[left:left + win], torch.hann_window(win, dtype=torch.float64).numpy(), atol=1e-15)
    assert np.all(w[:left] == 0) and np.all(w[left + win:] == 0)


def test_stft_argument_checks_need_no_device():
    for bad in (dict(n_fft=4096, hop=256, win=1024), dict(n_fft=1023, hop=256, win=1023), dict(n_fft=1024, hop=256, win=1025),
                dict(n_fft=1024, hop=0, win=1024), dict(n_fft=8, hop=2, win=8), dict(n_fft=1024, hop=1025, win=1024)):
        with pytest.raises(_lib.OvError):
            mp._stft_geometry(8000, bad["n_fft"], bad["hop"], bad["win"], False)
    with pytest.raises(ValueError):
        mp._stft_geometry(384, 1024, 256, 1024, False)          # N == the reflect padding
    with pytest.raises(ValueError):
        mp._stft_geometry(32, 64, 64, 64, True)                 # the centring pad reflects 32 samples of 32
    assert mp._stft_geometry(385, 1024, 256, 1024, False) == (384, 0, 1)
    assert mp._stft_geometry(29, 64, 7, 50, True) == (28, 32, 13)


# ---- ABI: the three additive entry points -------------------------------------------------------------------------------
def test_header_declares_the_new_entry_points_and_keeps_the_version():
    header = open(os.path.join(REPO, "include", "openvoice_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"^(?:int|size_t)\s+(ov_\w+)\s*\(", code, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/openvoice_amd.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert header.count(name) >= 2, f"{name} is missing from the ABI list in the header comment"
    assert int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1)) == 212 == _lib.MIN_VERSION
    assert "mel_processing.py:40-75" in header and "mel_processing.py:122-133" in header
    assert len(_lib.SIGNATURES["ov_stft_mag_f32"][1]) == 11 and len(_lib.SIGNATURES["ov_mel_log_f32"][1]) == 12
    shim = open(os.path.join(REPO, "openvoice_amd", "csrc", "torch_shim.cpp")).read()
    for name in NEW_SYMBOLS:
        assert f"<&{name}>" in shim, f"{name} is not bound in csrc/torch_shim.cpp"


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built (run __graft_entry__.build())")
def test_library_exports_and_checks_arguments_without_a_gpu():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert hasattr(_lib.torch_ops(), name[3:])
    assert lib.ov_stft_tile_frames() == mp.TILE_FRAMES == _lib.torch_ops().stft_tile_frames()
    assert lib.ov_version() == 212
    p = 0x10000                       # never dereferenced: every call below fails a check before any launch
    E_BADARG, E_UNSUPPORTED = -1, -2
    assert lib.ov_stft_mag_f32(None, p, p, 1, 4096, 1024, 256, 1024, 0, 16, None) == E_BADARG
    assert lib.ov_stft_mag_f32(p, p, p, 1, 8192, 4096, 1024, 4096, 0, 8, None) == E_UNSUPPORTED
    assert lib.ov_stft_mag_f32(p, p, p, 1, 8192, 1023, 256, 1023, 0, 32, None) == E_UNSUPPORTED
    assert lib.ov_stft_mag_f32(p, p, p, 1, 8192, 1024, 256, 1025, 0, 32, None) == E_UNSUPPORTED
    assert lib.ov_stft_mag_f32(p, p, p, 1, 8192, 1024, 0, 1024, 0, 32, None) == E_UNSUPPORTED
    assert lib.ov_stft_mag_f32(p, p, p, 1, 384, 1024, 256, 1024, 0, 4, None) == E_BADARG       # N == pad
    assert lib.ov_stft_mag_f32(p, p, p, 1, 8192, 1024, 256, 1024, 0, 36, None) == E_BADARG     # ld != padded T = 32
    assert lib.ov_stft_mag_f32(p, p, p, 0, 8192, 1024, 256, 1024, 0, 32, None) == E_BADARG
    assert lib.ov_mel_log_f32(p, p, None, 1, 80, 513, 8, 8, 513 * 8, 8, 1e-5, None) == E_BADARG
    assert lib.ov_mel_log_f32(p, p, p, 1, 257, 513, 8, 8, 513 * 8, 8, 1e-5, None) == E_UNSUPPORTED
    assert lib.ov_mel_log_f32(p, p, p, 1, 80, 1026, 8, 8, 1026 * 8, 8, 1e-5, None) == E_UNSUPPORTED
    assert lib.ov_mel_log_f32(p, p, p, 1, 80, 513, 8, 7, 513 * 8, 8, 1e-5, None) == E_BADARG    # row stride < T
    assert lib.ov_mel_log_f32(p, p, p, 2, 80, 513, 8, 8, 100, 8, 1e-5, None) == E_BADARG        # items overlap
    assert lib.ov_mel_log_f32(p, p, p, 1, 80, 513, 8, 8, 513 * 8, 8, 0.0, None) == E_BADARG     # log(0)
