"""The engine as four objects (``ConverterEngine``, ``launch.Launcher``, ``generator_fp32.GeneratorFp32``,
``ref_enc.ReferenceEncoder``), without a GPU: the names other code uses on the engine reach their owners, the source
digest covers every module that issues a conversion's launches, and the workspace sizes are what they were."""
import types

import pytest

from openvoice_amd import _lib, engine, generator_fp32, hostinfo
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

GENERATOR_NAMES = ("total_upsample", "stages", "fuse_pairs", "use_winograd", "use_multi_launch", "chain_streams",
                   "chain_streams_max_batch", "split_resblocks", "split3_products", "generator_margin", "frame_limits",
                   "limit_margin", "_split3_on", "_chain_scratch")
REF_ENC_NAMES = (("reference_encoder", "__call__"), ("reference_encoder_ragged", "reference_encoder_ragged"),
                 ("_reference_encoder_ragged_stack", "_reference_encoder_ragged_stack"))


class _RefEnc:
    def __call__(self, x):
        return ("dense", x)

    def reference_encoder_ragged(self, spec, frames):
        return ("ragged", spec, frames)

    def _reference_encoder_ragged_stack(self, spec, frames):
        return ("stack", spec, frames)


def _engine():
    eng = object.__new__(engine.ConverterEngine)
    eng.launcher = types.SimpleNamespace(profile=None)
    eng.generator = types.SimpleNamespace(**{n: ("generator's", n) for n in GENERATOR_NAMES})
    eng.ref_enc = _RefEnc()
    return eng


def test_forwarded_names_read_and_write_the_owners_attribute():
    eng = _engine()
    assert eng.profile is None
    records = eng.profile = []
    assert eng.launcher.profile is records and "profile" not in vars(eng)
    for n in GENERATOR_NAMES:
        assert getattr(eng, n) == ("generator's", n)
        setattr(eng, n, ("set through the engine", n))
        assert getattr(eng.generator, n) == ("set through the engine", n) and n not in vars(eng)
    assert eng.reference_encoder(1) == ("dense", 1)
    assert eng.reference_encoder_ragged(2, [3]) == ("ragged", 2, [3])
    assert eng._reference_encoder_ragged_stack(4, [5]) == ("stack", 4, [5])
    eng.ref_enc = None
    for name, _ in REF_ENC_NAMES:
        with pytest.raises(_lib.OvError, match=r"this checkpoint has no ref_enc\.\* weights"):
            getattr(eng, name)


def test_use_winograd_is_one_switch_for_the_generator_and_the_wavenet_layers(monkeypatch):
    """``eng.use_winograd = False`` reaches the generator, and the WaveNet path (``_wavenet``) reads the same value: the
    layer launches it issues for a shape that ``wn_wino_policy`` gives to the Winograd layer follow the switch."""
    eng = _engine()
    eng.generator.use_winograd = True
    eng.fuse_wn, eng.wn_row_split, eng._wn_bf16_on, eng._wn_choice = True, 0, False, None
    eng.launcher.timed = lambda tag, flops, fn, *extra: fn()
    seen = []
    monkeypatch.setattr(engine, "launch_wn_layer", lambda *a, **kw: seen.append(kw["winograd"]))
    wn = types.SimpleNamespace(hidden=192, n_layers=2, fused=True, fused_layers=[dict(K=5)] * 2)
    cond = types.SimpleNamespace(shape=(1, 768))
    ws = dict(Tp=864, h=None, h2=None, acts=None, skip=None)
    B, T = 32, 861
    assert engine.wn_wino_policy(B, T)
    eng._wavenet(wn, ws, B, T, cond, None)
    eng.use_winograd = False
    assert eng.generator.use_winograd is False
    eng._wavenet(wn, ws, B, T, cond, None)
    assert seen == [True, True, False, False]


def test_source_digest_covers_the_modules_that_issue_a_conversions_launches(monkeypatch):
    """``kernel_source_digest()`` changes with the bytes of generator_fp32.py and of launch.py, not with ref_enc.py's."""
    import builtins
    import os
    real_open = builtins.open

    def digest_with(changed):
        def reader(path, mode="r", *args, **kwargs):
            fh = real_open(path, mode, *args, **kwargs)
            if "b" in mode and os.path.basename(str(path)) == changed:
                data = fh.read() + b"\n# one more line\n"
                fh.close()
                import io
                return io.BytesIO(data)
            return fh
        monkeypatch.setattr(builtins, "open", reader)
        try:
            return hostinfo.kernel_source_digest()
        finally:
            monkeypatch.setattr(builtins, "open", real_open)

    plain = hostinfo.kernel_source_digest()
    assert digest_with("no_such_file.py") == plain
    for name in ("generator_fp32.py", "launch.py", "engine.py", "generator.py"):
        assert digest_with(name) != plain, name
    assert digest_with("ref_enc.py") == plain


@pytest.mark.parametrize("B,T,frame_rate,dec,plain,multi", [(32, 861, 56650752, 225705984, 4740722688, 8352018432),
                                                            (1, 64, 131136, 524288, 11010304, 19398912)])
def test_workspace_sizes_are_the_ones_before_the_split(B, T, frame_rate, dec, plain, multi):
    """The generator's size function (``generator_fp32.scratch_elems``) and the engine's frame-rate size sum to what
    ``workspace_bytes`` returned for the released configuration when one function computed both (the constants): with the
    _DEC_BUFFERS decoder buffers alone and with the multi launches' ``multi_launch_scratch_buffers`` more."""
    cfg = CONVERTER_MODEL_CONFIG
    pre, per_buffer = generator_fp32.scratch_elems(cfg, B, T)
    Tp, H, C = engine.padded_frames(T), cfg["hidden_channels"], cfg["inter_channels"]
    assert per_buffer == dec and pre == B * 512 * Tp
    assert engine._workspace_elems(cfg, B, T) == (B * (Tp + 4 * H * Tp + 4 * C * Tp) + pre, dec) == (frame_rate, dec)
    eng = object.__new__(engine.ConverterEngine)
    eng.cfg = cfg
    for extra, want in ((0, plain), (engine.multi_launch_scratch_buffers(cfg), multi)):
        eng.generator = types.SimpleNamespace(workspace_buffers=lambda B, T: generator_fp32._DEC_BUFFERS + extra)
        assert eng.workspace_bytes(B, T) == want
