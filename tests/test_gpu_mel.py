"""The general device STFT (``ov_stft_mag_f32``) and the log-mel projection (``ov_mel_log_f32``) against their float64
mirrors (openvoice_amd/mel_processing.py: ``stft_magnitude_host``, ``mel_log_host``), element by element, with bounds that
are derived, not measured:

* each of re and im is a length-n_fft fp32 dot product of fp32-rounded weights, so ``e = (n_fft + 4) 2^-24 sum |w x|`` per
  component for any summation order, and ``|got - ref| <= hypot(e_re, e_im) + 2^-22 ref``;
* the mel products are non-negative, so ``dv = (bins + 4) 2^-24 v`` and
  ``|got - ref| <= dv / max(v - dv, clip) + 4 * 2^-24 max(1, |ref|)``; for ``mel_spectrogram_torch`` the spectrogram's own
  bound is carried through the non-negative mel weights into ``dv``.

Worst ``err / lim`` seen on an MI355X: STFT 0.154 (at 16 / 1 / 16; 0.09 at n_fft = 64, under 0.025 at n_fft >= 400: the bound is a worst case
over summation orders and grows with n_fft, a k-ordered fma chain sits far inside it), mel projection 0.59 (at the clamp,
where the bound is the 4 * 2^-24 |ref| of the logarithm alone and logf is 1.7 ulp from float64 at log(1e-5); 0.015 for sums
well above the clamp), mel spectrogram 0.010.  Each test prints its own figure.
The shapes are the smallest at which the kernels can go wrong: T = 1, 2, one tile of frames and one tile plus one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd import mel_processing as mp  # noqa: E402
from openvoice_amd.launch import padded_frames  # noqa: E402

DEV = "cuda:0"
TILE = mp.TILE_FRAMES
SHAPES = [(1024, 320, 1024, False),     # hop does not divide n_fft
          (1024, 256, 800, False),      # short window
          (1024, 256, 1024, True),      # centred
          (2048, 512, 2048, False),     # largest n_fft
          (2048, 2048, 2048, False),    # hop = n_fft
          (400, 160, 400, True),        # 201 bins, K remainder
          (64, 7, 50, True),            # tiny and odd
          (16, 1, 16, False),           # smallest n_fft, hop 1
          (1024, 96, 1024, False),      # hop a multiple of 32
          (1024, 256, 1024, False)]     # the released shape (spectrogram_torch's own kernels are not involved)


def _wave(B, N, seed=0):
    """The spectrogram test's signal: a sinusoid per item plus noise, amplitude 0.65."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(N, dtype=torch.float32) / 22050
    return 0.6 * torch.sin(2 * torch.pi * (200 + 300 * torch.arange(B)[:, None]) * t) + 0.05 * torch.randn(B, N, generator=gen)


def _samples_for(n_fft, hop, center, frames):
    """The N that gives ``frames`` frames, with a few samples to spare; where the pads alone already give more frames (a
    centred transform of the shortest waveform that can be reflected), the shortest N there is."""
    pad1, pad2 = (n_fft - hop) // 2, (n_fft // 2 if center else 0)
    N = (frames - 1) * hop + n_fft - 2 * pad1 - 2 * pad2 + min(hop - 1, 3)
    return max(N, pad1 + 1, pad2 - 2 * pad1 + 1)


def _storage(view, ld):
    B, R, _ = view.shape
    return view.as_strided((B, R, ld), (R * ld, ld, 1))


def test_tile_constant_follows_the_kernel():
    assert _lib.call("ov_stft_tile_frames") == TILE


@pytest.mark.parametrize("frames", [1, 2, TILE, TILE + 1])
@pytest.mark.parametrize("n_fft,hop,win,center", SHAPES)
def test_stft_magnitude_meets_the_derived_bound(n_fft, hop, win, center, frames):
    """B = 3 against the mirror, then every item alone (B = 1): within the bound, and bit for bit its row of the batch."""
    N = _samples_for(n_fft, hop, center, frames)
    y = _wave(3, N, seed=n_fft + hop + frames)
    ref, lim = mp.stft_magnitude_host(y, n_fft, hop, win, center)
    T = ref.shape[2]
    assert T >= frames and (T == frames or N <= max(n_fft - hop, n_fft) // 2 + 1)      # more only where the pads force it
    got = mp.stft_magnitude(y.to(DEV), n_fft, hop, win, center)
    assert got.shape == (3, n_fft // 2 + 1, T) and got.dtype == torch.float32
    assert got.stride(2) == 1 and got.stride(1) % 4 == 0 and got.stride(1) == padded_frames(T)
    assert torch.all(_storage(got, got.stride(1))[:, :, T:] == 0)
    g = got.cpu().double().numpy()
    worst = float((np.abs(g - ref) / lim).max())
    print(f"stft {n_fft}/{hop}/{win} center={center} T={T}: worst err / lim = {worst:.4f}")
    assert np.all(np.isfinite(g)) and worst <= 1.0
    for b in range(3):
        one = mp.stft_magnitude(y[b:b + 1].to(DEV), n_fft, hop, win, center)
        assert torch.equal(one[0], got[b]), f"item {b} depends on the batch"


def test_stft_writes_its_padded_columns_and_nothing_else():
    """The kernel itself on a NaN-filled buffer with a guard row behind it: columns [T, ld) are zero, every other element
    of the output is finite, the guard stays NaN."""
    n_fft, hop, N = 400, 160, _samples_for(400, 160, False, TILE + 1)
    y = _wave(2, N, seed=5).to(DEV)
    T = mp._stft_geometry(N, n_fft, hop, n_fft, False)[2]
    ld, bins = padded_frames(T), n_fft // 2 + 1
    assert T == TILE + 1 and ld == T + 3
    buf = torch.full((2 * bins * ld + ld,), float("nan"), device=DEV)
    wpack = torch.from_numpy(mp.pack_stft_weights(n_fft, n_fft)).to(DEV)
    _lib.call("ov_stft_mag_f32", y, wpack, buf, 2, N, n_fft, hop, n_fft, 0, ld)
    out = buf[:2 * bins * ld].view(2, bins, ld)
    assert torch.all(out[:, :, T:] == 0) and torch.all(torch.isfinite(out[:, :, :T])) and torch.all(torch.isnan(buf[2 * bins * ld:]))
    assert torch.equal(out[:, :, :T], mp.stft_magnitude(y, n_fft, hop, n_fft))


def test_spectrogram_torch_is_untouched_by_stft_magnitude():
    """No shared cache entry: the released shape through ``spectrogram_torch`` gives the same bits before and after
    ``stft_magnitude`` ran at that shape and at another."""
    from openvoice_amd.mel_processing import spectrogram_torch
    y = _wave(2, 5000, seed=9).to(DEV)
    before = spectrogram_torch(y, 1024, 22050, 256, 1024).clone()
    a = mp.stft_magnitude(y, 1024, 256, 1024)
    mp.stft_magnitude(y, 1024, 320, 1024)
    after = spectrogram_torch(y, 1024, 22050, 256, 1024)
    assert torch.equal(before, after)
    assert a.shape == before.shape and (a - before).abs().max().item() <= 2e-5 * max(1.0, before.abs().max().item())
    with pytest.raises(_lib.OvError):                         # still no general path behind spectrogram_torch
        spectrogram_torch(y, 1024, 22050, 320, 1024)


@pytest.mark.parametrize("num_mels", [1, 40, 80, 256])
@pytest.mark.parametrize("bins", [9, 201, 513, 1025])
def test_spec_to_mel_meets_the_derived_bound(bins, num_mels):
    """T = 1, 33 and 65; a column of zeros (log(1e-5) in every row, one value); the same spectrogram scaled by 1e-4, which
    puts a good share of the sums on either side of the clamp; rows further apart than T."""
    n_fft = 2 * (bins - 1)
    fb32 = mp.mel_filterbank(22050, n_fft, num_mels, 0, None).astype(np.float32)
    floor = float(torch.log(torch.tensor(1e-5)))
    for T in (1, TILE + 1, 2 * TILE + 1):
        gen = torch.Generator().manual_seed(bins + num_mels + T)
        store = torch.randn(3, bins, T + 5, generator=gen).abs() * 3
        store *= 10.0 ** (2 * torch.rand(3, 1, T + 5, generator=gen) - 1)      # frame levels over 20 dB either way
        zc = T // 2
        store[:, :, zc] = 0
        for scale in (1.0, 1e-4):
            spec = (store * scale)[:, :, :T]                                    # row stride T + 5, item stride bins (T + 5)
            ref, lim = mp.mel_log_host(spec, fb32)
            got = mp.spec_to_mel_torch((store * scale).to(DEV)[:, :, :T], n_fft, num_mels, 22050, 0, None)
            assert got.shape == (3, num_mels, T) and got.stride(1) == padded_frames(T)
            assert torch.all(_storage(got, got.stride(1))[:, :, T:] == 0)
            g = got.cpu().double().numpy()
            ratio = np.abs(g - ref) / lim
            worst = float(ratio.max())
            clamped = float((ref == ref.min()).mean())
            print(f"mel bins={bins} mels={num_mels} T={T} scale={scale:g}: worst err / lim = {worst:.4f} "
                  f"({float(np.delete(ratio, zc, axis=2).max()) if T > 1 else 0.0:.4f} off the zero column), "
                  f"{clamped:.2f} of the sums at the clamp")
            assert np.all(np.isfinite(g)) and worst <= 1.0
            col = got[:, :, zc]
            assert torch.all(col == col.flatten()[0]) and abs(col.flatten()[0].item() - floor) <= 2.0 ** -22 * abs(floor)
            one = mp.spec_to_mel_torch((store * scale)[1, :, :T].to(DEV), n_fft, num_mels, 22050, 0, None)   # [bins, T]
            assert torch.equal(one, got[1])


@pytest.mark.parametrize("n_fft,hop,win,center,num_mels", [(1024, 256, 1024, False, 80), (1024, 320, 1024, True, 80),
                                                           (400, 160, 400, True, 40)])
def test_mel_spectrogram_meets_the_propagated_bound(n_fft, hop, win, center, num_mels):
    N = _samples_for(n_fft, hop, center, TILE + 1)
    y = _wave(3, N, seed=n_fft + hop)
    sr = 22050 if n_fft == 1024 else 16000
    spec_ref, spec_lim = mp.stft_magnitude_host(y, n_fft, hop, win, center)
    assert spec_ref.shape[2] == TILE + 1
    fb32 = mp.mel_filterbank(sr, n_fft, num_mels, 0, None).astype(np.float32)
    ref, lim = mp.mel_log_host(spec_ref, fb32, spec_lim=spec_lim)
    got = mp.mel_spectrogram_torch(y.to(DEV), n_fft, num_mels, sr, hop, win, 0, None, center=center)
    assert got.shape == (3, num_mels, TILE + 1)
    worst = float((np.abs(got.cpu().double().numpy() - ref) / lim).max())
    print(f"mel spectrogram {n_fft}/{hop}/{win} center={center} mels={num_mels}: worst err / lim = {worst:.4f}")
    assert worst <= 1.0
    two = mp.spec_to_mel_torch(mp.stft_magnitude(y.to(DEV), n_fft, hop, win, center), n_fft, num_mels, sr, 0, None)
    assert torch.equal(got, two)


def test_unsupported_arguments_raise_and_launch_nothing():
    """Argument checks: each call raises before anything is launched."""
    y = torch.zeros(1, 8192, device=DEV)
    errors = (_lib.OvError, ValueError)
    for kw in (dict(n_fft=4096, hop_size=1024, win_size=4096), dict(n_fft=1023, hop_size=256, win_size=1023),
               dict(n_fft=1024, hop_size=256, win_size=1025), dict(n_fft=1024, hop_size=0, win_size=1024)):
        with pytest.raises(errors):
            mp.stft_magnitude(y, **kw)
    with pytest.raises(errors):
        mp.stft_magnitude(y.double(), 1024, 256, 1024)
    with pytest.raises(errors):
        mp.stft_magnitude(y[:, :384], 1024, 256, 1024)                       # N == the reflect padding
    with pytest.raises(errors):
        mp.stft_magnitude(torch.zeros(1, 32, device=DEV), 64, 64, 64, center=True)    # N == the centring pad
    with pytest.raises(errors):
        mp.mel_spectrogram_torch(y, 1024, 257, 22050, 256, 1024, 0, None)
    with pytest.raises(errors):
        mp.spec_to_mel_torch(torch.zeros(1, 513, 8, device=DEV), 1024, 257, 22050, 0, None)
    with pytest.raises(errors):
        mp.spec_to_mel_torch(torch.zeros(1, 513, 8, device=DEV, dtype=torch.float64), 1024, 80, 22050, 0, None)
    with pytest.raises(errors):
        mp.spec_to_mel_torch(torch.zeros(1, 512, 8, device=DEV), 1024, 80, 22050, 0, None)     # bins != n_fft / 2 + 1
    with pytest.raises(errors):
        _lib.call("ov_stft_mag_f32", y, torch.zeros(16, device=DEV), torch.zeros(16, device=DEV), 1, 8192, 4096, 1024, 4096, 0, 8)
    with pytest.raises(errors):
        _lib.call("ov_mel_log_f32", torch.zeros(513 * 8, device=DEV), torch.zeros(257 * 513, device=DEV),
                  torch.zeros(257 * 8, device=DEV), 1, 257, 513, 8, 8, 513 * 8, 8, 1e-5)
