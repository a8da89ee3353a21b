"""Counter-based noise (openvoice_amd/noise.py), the part that needs no GPU: the float64 restatement of the definition
(Philox4x32-10 known answers, purity, moments), ``check_seed`` and the host side of ``ov_normal_philox_f32``."""
import ctypes
import os
import re

import numpy as np
import pytest

from openvoice_amd import _lib, noise

HERE = os.path.dirname(os.path.abspath(__file__))
lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")

# Random123's known-answer vectors for philox4x32_10: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,expected", KAT)
def test_philox_core_reproduces_the_known_answers(counter, key, expected):
    got = noise.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == expected


def test_known_answers_as_one_vectorised_call():
    counters = np.array([k[0] for k in KAT], dtype=np.uint64).T
    keys = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(noise.philox4x32_10(tuple(counters), tuple(keys)), axis=1)
    assert got.dtype == np.uint32 and (got == np.array([k[2] for k in KAT], dtype=np.uint32)).all()


def test_definition_spelled_out_for_one_block():
    """normal_host against the issue's formulas written out by hand for the four frames of one Philox block."""
    seed, stream, purpose, c, block = (5 << 32) | 77, 3, 2, 9, 1234
    r = [int(w) for w in noise.philox4x32_10((block, c, stream, purpose), (seed & 0xffffffff, seed >> 32))]
    got = noise.normal_host((seed, stream), 1, 4 * block, 4, purpose=purpose, c0=c)[0]
    for j in range(4):
        ra, rb = (r[0], r[1]) if j < 2 else (r[2], r[3])
        u1, u2 = ((ra >> 8) + 0.5) * 2.0 ** -24, (rb >> 8) * 2.0 ** -24
        want = np.sqrt(-2 * np.log(u1)) * (np.cos if j % 2 == 0 else np.sin)(2 * np.pi * u2)
        assert got[j] == want
    assert np.abs(got).max() <= np.sqrt(50 * np.log(2))


@pytest.mark.parametrize("f0", range(10))
def test_restatement_is_pure_in_the_first_frame(f0):
    nf, C = 13, 5
    whole = noise.normal_host(99, C, 0, f0 + nf)
    assert np.array_equal(noise.normal_host(99, C, f0, nf), whole[:, f0:])


def test_restatement_reaches_the_last_frame():
    x = noise.normal_host(1, 2, (1 << 34) - 8, 8)
    assert x.shape == (2, 8) and np.isfinite(x).all()
    with pytest.raises(ValueError):
        noise.normal_host(1, 2, (1 << 34) - 8, 9)


def test_every_coordinate_changes_every_value():
    seed, stream, purpose, c = 12345 | (7 << 32), 4, 0, 10
    base = noise.normal_host((seed, stream), 1, 0, 64, purpose=purpose, c0=c)
    others = {
        "seed bit 0": noise.normal_host((seed ^ 1, stream), 1, 0, 64, purpose=purpose, c0=c),
        "seed bit 32": noise.normal_host((seed ^ (1 << 32), stream), 1, 0, 64, purpose=purpose, c0=c),
        "stream": noise.normal_host((seed, stream + 1), 1, 0, 64, purpose=purpose, c0=c),
        "purpose": noise.normal_host((seed, stream), 1, 0, 64, purpose=purpose + 1, c0=c),
        "channel": noise.normal_host((seed, stream), 1, 0, 64, purpose=purpose, c0=c + 1),
    }
    for name, x in others.items():
        assert (x != base).all(), name


def test_moments_of_the_definition():
    """Seed 1234, stream 0, purpose 0, 192 x 4000: bars at four standard errors for N = 768 000."""
    x = noise.normal_host(1234, 192, 0, 4000)
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    mean, std = float(x.mean()), float(x.std())
    along_t, along_c = corr(x[:, :-1], x[:, 1:]), corr(x[:-1], x[1:])
    print(f"mean {mean:.2e} std {std:.5f} lag-1 frames {along_t:.2e} channels {along_c:.2e}")
    assert abs(mean) < 4.6e-3 and abs(std - 1) < 3.3e-3
    assert abs(along_t) < 4.6e-3 and abs(along_c) < 4.6e-3
    assert np.abs(x).max() <= np.sqrt(50 * np.log(2))


# ---- seeds ----------------------------------------------------------------------------------------------------------
def test_check_seed_accepts_ints_and_pairs():
    assert noise.check_seed(7) == (7, 0) and noise.check_seed(7, index=3) == (7, 3)
    assert noise.check_seed((7, 5)) == (7, 5) and noise.check_seed((7, 5), index=3) == (7, 5)
    assert noise.check_seed(np.int64(9)) == (9, 0)
    assert noise.check_seed(((1 << 63) - 1, (1 << 32) - 1)) == ((1 << 63) - 1, (1 << 32) - 1)


@pytest.mark.parametrize("bad", [True, False, -1, 1 << 63, (1, 1 << 32), (1, -1), (-1, 0), (True, 0), (1, True), 1.5,
                                 "7", None, (1, 2, 3), (1,)])
def test_check_seed_rejects(bad):
    with pytest.raises(ValueError):
        noise.check_seed(bad)


def test_per_item_rules():
    assert noise.per_item(5, 3) == [(5, 0), (5, 1), (5, 2)]
    assert noise.per_item((5, 10), 2) == [(5, 10), (5, 11)]
    assert noise.per_item([5, (6, 2)], 2) == [(5, 0), (6, 2)]
    for wrong in ([5], [5, 6, 7]):
        with pytest.raises(ValueError):
            noise.per_item(wrong, 2)
    with pytest.raises(ValueError):
        noise.per_item((5, (1 << 32) - 1), 2)          # the second item's stream would be 2^32
    assert noise.rows(5, 2) == [(5, 0, 0), (5, 1, 0)]
    assert noise.rows([(5, 0, 30), (5, 0, 60)], 2) == [(5, 0, 30), (5, 0, 60)]
    with pytest.raises(ValueError):
        noise.rows([(5, 0, 1 << 34), (5, 0, 0)], 2)


def test_seed_and_noise_together_are_rejected_before_any_device_work():
    """The API layers check this first: no model, no device and no library are needed to get the error."""
    from openvoice_amd import api, live, longform
    from openvoice_amd.engine import ConverterEngine, GraphedConversion
    from openvoice_amd.tts_engine import TtsEngine
    nz = object()
    noise.exclusive(None, noise=nz)
    noise.exclusive(3, noise=None)
    with pytest.raises(ValueError, match="mutually exclusive"):
        noise.exclusive(3, noise=nz)
    conv = api.ToneColorConverter.__new__(api.ToneColorConverter)        # no constructor: it would need a device
    with pytest.raises(ValueError, match="mutually exclusive"):
        conv.convert_batch(None, None, None, noise=nz, seed=1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        conv.convert_long(None, None, None, noise=nz, seed=1)
    tts = api.BaseSpeakerTTS.__new__(api.BaseSpeakerTTS)
    for kw in (dict(noise_w=nz), dict(noise_z=nz)):
        with pytest.raises(ValueError, match="mutually exclusive"):
            tts.tts_from_ids([[1, 2]], 0, seed=1, **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        longform._StreamState(None, None, None, noise=nz, seed=1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        live.LiveStream(None, None, None, noise=nz, seed=1)
    wc = longform.WindowedConverter.__new__(longform.WindowedConverter)
    with pytest.raises(ValueError, match="mutually exclusive"):
        wc._prepare(None, nz, None, seed=1)


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_symbol_and_keeps_the_version():
    header = open(os.path.join(HERE, "..", "include", "openvoice_amd.h")).read()
    assert "int ov_normal_philox_f32(" in header
    assert int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1)) == 212
    assert _lib.MIN_VERSION == 212 and "ov_normal_philox_f32" in _lib.SIGNATURES


@lib_built
def test_host_argument_checks_return_before_any_launch():
    lib = _lib.load()
    assert lib.ov_version() == 212
    f = lib.ov_normal_philox_f32
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails validation before a launch
    BADARG, ALIGN = -1, -3
    assert f(None, 1, 192, fake, 1024, 8, None) == BADARG            # records
    assert f(fake, 1, 192, None, 1024, 8, None) == BADARG            # dst
    assert f(fake, 0, 192, fake, 1024, 8, None) == BADARG            # R <= 0
    assert f(fake, -1, 192, fake, 1024, 8, None) == BADARG
    assert f(fake, 65536, 192, fake, 1024, 8, None) == BADARG        # R > 65535
    assert f(fake, 1, 0, fake, 1024, 8, None) == BADARG              # C <= 0
    assert f(fake, 1, -2, fake, 1024, 8, None) == BADARG
    assert f(fake, 1, 192, fake, 0, 8, None) == BADARG               # dst_elems <= 0
    assert f(fake, 1, 192, fake, -5, 8, None) == BADARG
    assert f(fake, 1, 192, fake, 1024, -1, None) == BADARG           # max_frames < 0
    for low_bits in (1, 2, 3):
        assert f(fake, 1, 192, ctypes.c_void_p(4096 + low_bits), 1024, 8, None) == ALIGN
