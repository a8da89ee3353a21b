"""The engine's forwards on the device (synthetic checkpoint, B = 1, T = 32): ``profile`` and ``use_winograd`` set
through ``ConverterEngine`` reach the launcher and the generator, graph capture leaves ``profile`` alone, and a TTS
engine's core decodes through the same ``GeneratorFp32``.  The ``use_winograd`` test runs T = 544 frames: a Winograd
launch needs ``WINO_MIN_ITEMS`` = 136 work items, which stages 1-3 have from B x T / 4 = 136 on -- at T = 32 every MRF
conv is a direct launch with the switch on or off, and the test could not tell the two apart."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd.engine import WINO_MIN_ITEMS, ConverterEngine, GraphedConversion  # noqa: E402
from openvoice_amd.generator_fp32 import GeneratorFp32  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG  # noqa: E402

DEV = "cuda:0"
B, T = 1, 32


@pytest.fixture(scope="module")
def eng(synth_sd):
    return ConverterEngine(synth_sd, CFG, 513, DEV, zero_g=True)


def _convert(eng, T=T):
    gen = torch.Generator().manual_seed(7)
    spec = torch.rand(B, 513, T, generator=gen).to(DEV)
    g = 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV)
    return eng.voice_conversion(spec, torch.full((B,), T, device=DEV), g, g, tau=0.3, seed=5)[0]


def test_profile_and_use_winograd_set_on_the_engine_reach_the_launches(eng):
    def mrf_records():
        eng.profile = []
        try:
            _convert(eng, T=4 * WINO_MIN_ITEMS)
            torch.cuda.synchronize()
            assert eng.launcher.profile is eng.profile
            return [r for r in eng.profile if r[0] == "mrf"]
        finally:
            eng.profile = None

    assert eng.use_winograd is True
    first = mrf_records()
    assert first and any(len(r) == 5 for r in first)          # the fifth field: only Winograd launches append it
    eng.use_winograd = False
    try:
        assert eng.generator.use_winograd is False
        direct = mrf_records()
        assert direct and all(len(r) == 4 for r in direct)
    finally:
        eng.use_winograd = True
    again = mrf_records()
    assert [len(r) for r in again] == [len(r) for r in first]


def test_graph_capture_leaves_profile_as_it_found_it(eng):
    records = eng.profile = []
    try:
        GraphedConversion(eng, B, T, 0.3)
        assert eng.profile is records and eng.launcher.profile is records and records == []
    finally:
        eng.profile = None
    GraphedConversion(eng, B, T, 0.3)
    assert eng.profile is None


def test_a_tts_engines_core_decodes_through_its_fp32_generator(synth_tts_sd):
    from openvoice_amd.tts_engine import TtsEngine
    core = TtsEngine(synth_tts_sd, CFG, 513, DEV, 68, 10).core
    assert isinstance(core.generator, GeneratorFp32) and core.ref_enc is None
    gen = torch.Generator().manual_seed(11)
    z = torch.randn(B, core.inter, T, generator=gen).to(DEV)
    cond = core.generator.cond(0.3 * torch.randn(1, core.gin, generator=gen).to(DEV))
    a = core.decode(z, cond).clone()
    b = core.generator.decode(z, cond, core._workspace(B, T)).clone()
    assert a.shape == (B, 1, T * core.total_upsample) and torch.equal(a, b) and a.abs().max() > 0
