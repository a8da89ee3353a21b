"""Host side of the windowed long-form / streaming conversion (openvoice_amd/longform.py): the window plan's invariants,
the conversion's receptive field (derived from the config and checked empirically on the CPU oracle), the window algebra
restated on the oracle, and argument validation of the two new C entry points.  No GPU."""
import ctypes
import os

import pytest
import torch

from openvoice_amd import _lib, longform
from openvoice_amd.hostinfo import usable_cpus
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

CFG = CONVERTER_MODEL_CONFIG


def _check_plan(T, Tw, ctx, grid):
    plan = longform.plan_windows(T, Tw, ctx, grid)
    if T <= Tw:
        assert plan == [(0, 0, T)]
        return plan
    core = longform.window_core(Tw, ctx, grid)
    assert plan[0][0] == 0 and plan[0][1] == 0
    assert plan[-1][0] + Tw == T and plan[-1][2] == T          # the last window ends exactly at T (never padded)
    edge = 0
    for i, (f0, lo, hi) in enumerate(plan):
        assert 0 <= f0 and f0 + Tw <= T                          # every window has Tw frames inside the file
        assert lo == edge and lo < hi and f0 <= lo and hi <= f0 + Tw   # cores partition [0, T) in order
        edge = hi
        if lo != 0:
            assert lo - f0 >= ctx, (T, Tw, i)                    # context before every interior core edge
        if hi != T:
            assert f0 + Tw - hi >= ctx, (T, Tw, i)               # ... and after it
        if i < len(plan) - 1:
            assert f0 == i * core and f0 % grid == 0             # regular windows on the grid
    assert edge == T
    return plan


@pytest.mark.parametrize("Tw", [255, 256, 300, 400, 512, 1000, 4096])
def test_plan_invariants_and_prefix_consistency(Tw):
    ctx, grid = 120, 15
    gen = torch.Generator().manual_seed(Tw)
    lengths = sorted(set([1, 2, Tw - 1, Tw, Tw + 1, 2 * Tw - 1, 2 * Tw, 2 * Tw + 1, 5 * Tw + 7] +
                         torch.randint(1, 20 * Tw, (60,), generator=gen).tolist()))
    plans = {T: _check_plan(T, Tw, ctx, grid) for T in lengths}
    for a in lengths:
        if a <= Tw:
            continue
        reg_a = plans[a][:-1]
        for b in lengths:
            if b > a:                      # the regular windows of a length are a prefix of any longer length's
                assert plans[b][:len(reg_a)] == reg_a, (a, b)


def test_plan_rejects_a_window_without_a_core():
    with pytest.raises(ValueError, match="no core"):
        longform.plan_windows(1000, 240, 120, 15)
    assert longform.plan_windows(1000, 255, 120, 15)[1][0] == 15


def test_context_and_grid_follow_from_the_config():
    from openvoice_amd.engine import GENERATOR_MARGIN, generator_margin_frames
    # enc_q 16 x (5 - 1) / 2 + flows 2 x 4 x 4 x (5 - 1) / 2 + generator max(16, margin) = 112 -> grid 15 -> 120
    assert generator_margin_frames(CFG) <= GENERATOR_MARGIN == 16
    assert longform.winograd_grid_frames(CFG) == 15
    assert longform.context_frames(CFG) == 120
    # stage 1's ConvTranspose: (128 x 8 phase rows + 32) x 64 T output elements reach 2^32
    assert longform.one_pass_limit_frames(CFG) == 63551 == 2**32 // (1056 * 64) + 1
    # a config with dilation 1 only: the Winograd tiles need 4 columns, stage 0 has 8 per frame -> every frame is on grid
    one = dict(CFG, resblock_dilation_sizes=[[1, 1, 1]] * 3)
    assert longform.winograd_grid_frames(one) == 1
    assert longform.context_frames(one) == 112


def _oracle_inputs(T, seed):
    gen = torch.Generator().manual_seed(seed)
    spec = torch.rand(1, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]
    g_src, g_tgt = 0.3 * torch.randn(1, 256, 1, generator=gen), 0.3 * torch.randn(1, 256, 1, generator=gen)
    return spec, g_src, g_tgt, torch.randn(1, 192, T, generator=gen)


def _oracle(sd, spec, g_src, g_tgt, noise, tau=0.3):
    from oracle import vc_oracle
    with torch.no_grad():
        return vc_oracle.voice_conversion(sd, CFG, spec, torch.tensor([spec.shape[2]]), g_src, g_tgt, tau, noise,
                                          zero_g=True)[0]


def test_empirical_reach_is_within_the_derived_context(synth_sd):
    """Perturb the spectrogram and the noise at one frame t0: every output sample outside t0 +- context frames is
    bit-identical, and the perturbation does reach beyond the generator's own margin (the derivation is not vacuous)."""
    torch.set_num_threads(usable_cpus(8))
    T, t0, ctx = 400, 200, longform.context_frames(CFG)
    spec, g_src, g_tgt, noise = _oracle_inputs(T, 7)
    a = _oracle(synth_sd, spec, g_src, g_tgt, noise)[0, 0]
    spec2, noise2 = spec.clone(), noise.clone()
    spec2[:, :, t0] += 1.0
    noise2[:, :, t0] += 1.0
    b = _oracle(synth_sd, spec2, g_src, g_tgt, noise2)[0, 0]
    lo, hi = (t0 - ctx) * 256, (t0 + ctx + 1) * 256
    assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:])
    changed = (a != b).nonzero()
    reach = max(t0 - changed.min().item() // 256, changed.max().item() // 256 - t0)
    print("empirical one-sided reach:", reach, "frames; derived context:", ctx)
    assert 32 < reach <= ctx


def test_window_algebra_on_the_oracle(synth_sd):
    """Windowed conversion restated on the CPU oracle (T = 590, windows of 360 frames: two regular windows and a last one
    shifted to end at T) reproduces the one-pass output."""
    torch.set_num_threads(usable_cpus(8))
    T, Tw = 590, 360
    ctx, grid = longform.context_frames(CFG), longform.winograd_grid_frames(CFG)
    spec, g_src, g_tgt, noise = _oracle_inputs(T, 11)
    whole = _oracle(synth_sd, spec, g_src, g_tgt, noise)[0, 0]
    plan = longform.plan_windows(T, Tw, ctx, grid)
    assert len(plan) == 3 and plan[-1][0] % grid != 0
    out = torch.full_like(whole, float("nan"))
    for f0, lo, hi in plan:
        o = _oracle(synth_sd, spec[:, :, f0:f0 + Tw], g_src, g_tgt, noise[:, :, f0:f0 + Tw])[0, 0]
        out[lo * 256:hi * 256] = o[(lo - f0) * 256:(hi - f0) * 256]
    err = (out - whole).abs().max().item()
    print("windowed vs one-pass oracle:", err)
    assert err <= 1e-5


lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")


@lib_built
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)         # never dereferenced: every call below fails validation before a launch
    hops = lib.ov_frame_hops_windows_f32
    assert hops(None, 1000, fake, 1, 256, 384, 8, 8, fake, None) == -1
    assert hops(fake, 1000, None, 1, 256, 384, 8, 8, fake, None) == -1
    assert hops(fake, 1000, fake, 1, 256, 384, 8, 8, None, None) == -1
    assert hops(fake, 0, fake, 1, 256, 384, 8, 8, fake, None) == -1          # no samples
    assert hops(fake, 384, fake, 1, 256, 384, 8, 8, fake, None) == -1        # pad >= n_samples (reflect undefined)
    assert hops(fake, 1000, fake, 0, 256, 384, 8, 8, fake, None) == -1       # no windows
    assert hops(fake, 1000, fake, 65536, 256, 384, 8, 8, fake, None) == -1   # grid.z
    assert hops(fake, 1000, fake, 1, 2048, 384, 8, 8, fake, None) == -1      # hop
    assert hops(fake, 1000, fake, 1, 256, 384, 8, 7, fake, None) == -1       # ld < U
    assert hops(fake, 1000, fake, 1, 256, 384, 7, 10, fake, None) == -3      # rows not 16-byte multiples
    assert hops(fake, 1000, fake, 1, 256, 384, 7, 8, ctypes.c_void_p(4100), None) == -3
    st = lib.ov_stitch_window_cores_f32
    assert st(None, fake, 1, 8, 256, fake, 2048, 0, None) == -1
    assert st(fake, None, 1, 8, 256, fake, 2048, 0, None) == -1
    assert st(fake, fake, 1, 8, 256, None, 2048, 0, None) == -1
    assert st(fake, fake, 0, 8, 256, fake, 2048, 0, None) == -1
    assert st(fake, fake, 1, 0, 256, fake, 2048, 0, None) == -1
    assert st(fake, fake, 1, 8, 0, fake, 2048, 0, None) == -1
    assert st(fake, fake, 1, 8, 256, fake, 0, 0, None) == -1
    assert st(fake, fake, 1, 8, 256, fake, 2048, -1, None) == -1
    assert lib.ov_version() >= 210


@lib_built
def test_torch_binding_of_the_new_entry_points_rejects_cpu_tensors():
    ops = _lib.torch_ops()
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.frame_hops_windows_f32(torch.zeros(4096), 4096, torch.zeros(1, dtype=torch.long), 1, 256, 384, 8, 8,
                                   torch.zeros(1, 256, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.stitch_window_cores_f32(torch.zeros(1, 2048), torch.zeros(1, 3, dtype=torch.long), 1, 8, 256,
                                    torch.zeros(2048), 2048, 0)


class _FakeModel(torch.nn.Module):
    """What WindowedConverter reads of a SynthesizerTrn: the config and the device of its parameters (CPU here)."""

    def __init__(self):
        super().__init__()
        self.model_cfg = dict(CFG)
        self.p = torch.nn.Parameter(torch.zeros(1))


def _recording_launch(log, n_fft=1024, hop=256, spf=256):
    """Stands in for WindowedConverter._launch on the CPU: the waveform is arange(N) as float32, so the buffer tells
    which file samples it holds; each window's reads are checked against what the buffer holds, its noise against the
    file's noise, and its core is written as absolute sample indices."""
    pad = (n_fft - hop) // 2

    def launch(self, wave, n_samples, plan_dev, firsts_dev, Tw, src_se, tgt_se, tau, nz, out, out_frame0):
        base = int(wave[0].item()) if n_samples else 0
        assert base % hop == 0 and wave.numel() >= n_samples
        for w, (f0, lo, hi) in enumerate(plan_dev.tolist()):
            assert firsts_dev[w].item() == f0
            fa = f0 + base // hop                                   # the window's absolute first frame
            first, last = fa * hop - pad, (fa + Tw - 1) * hop + n_fft - pad    # samples [first, last) it reads
            end = base + n_samples
            assert first >= base or base == 0, "a window reads samples trimmed off the buffer"
            assert last <= end or log["n"] == end, "a window reads past the buffered samples before the end is known"
            log["windows"].append((fa, lo + fa - f0, hi + fa - f0))
            if log["noise"] is not None:
                assert torch.equal(nz[w], log["noise"][0, :, fa:fa + Tw])
            s0 = (lo - out_frame0) * spf
            out[s0:s0 + (hi - lo) * spf] = torch.arange((lo + fa - f0) * spf, (hi + fa - f0) * spf, dtype=out.dtype)
    return launch


@pytest.mark.parametrize("N,Tw,sizes", [(256 * 2100 + 99, 512, [1, 3, 44100, 1001, 7, 30000, 257]),
                                        (256 * 2100 + 99, 512, [10 ** 9]),
                                        (256 * 512 + 300, 512, [5000]),       # the file ends inside the first window
                                        (256 * 3000, 600, [256, 255, 257]),
                                        (256 * 1100 + 128, 1024, [131072])])
def test_stream_schedules_the_plan_of_the_whole_input(monkeypatch, N, Tw, sizes):
    """Pushes of any sizes run exactly the windows of plan_windows(T) in order, each on samples the buffer still holds,
    with the file's noise slice, and their cores concatenate to the whole output; memory stays bounded."""
    log = {"windows": [], "noise": None, "n": N}
    monkeypatch.setattr(longform.WindowedConverter, "_launch", _recording_launch(log))
    conv = longform.WindowedConverter(_FakeModel(), window_frames=Tw, windows_per_launch=1)
    T = longform.frames_of(N, 1024, 256)
    log["noise"] = torch.randn(1, 192, T)
    st = conv.stream(None, None, noise=log["noise"])
    wave = torch.arange(N, dtype=torch.float32)
    outs, pos, i, biggest = [], 0, 0, 0
    while pos < N:
        k = sizes[i % len(sizes)]
        i += 1
        outs.append(st.push(wave[pos:pos + k]))
        pos = min(N, pos + k)
        biggest = max(biggest, st._len)
    outs.append(st.close())
    out = torch.cat(outs)
    assert log["windows"] == longform.plan_windows(T, Tw, conv.context, conv.grid)
    assert torch.equal(out, torch.arange(T * 256, dtype=torch.float32))
    assert biggest <= (Tw + conv.core + 4) * 256 + min(max(sizes), N)      # bounded by the window and one push
    # the whole-file converter runs the same plan
    log["windows"] = []
    out2 = conv.convert(wave, None, None, noise=log["noise"])
    assert log["windows"] == longform.plan_windows(T, Tw, conv.context, conv.grid)
    assert torch.equal(out2, out)
