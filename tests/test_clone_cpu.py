"""Host side of the cloned-voice chain (openvoice_amd/clone.py), no GPU: the join plan against a brute-force loop, the
float64 restatement against ``BaseSpeakerTTS.audio_numpy_concat``, the batching rule, the symbol's declarations and the
argument checks of ``VoiceCloner``."""
import os
import types

import numpy as np
import pytest

from openvoice_amd import _lib, api, clone

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTH_SETS = [
    [[5]],
    [[0]],
    [[0, 0, 3]],
    [[256, 0, 512], [1], [], [4099, 7, 0, 0, 1024]],
    [[1, 2, 3, 4, 5, 6, 7], [768] * 5],
]


@pytest.mark.parametrize("gap", [0, 1, 1102])
@pytest.mark.parametrize("lengths", LENGTH_SETS)
def test_join_plan_against_a_brute_force_loop(lengths, gap):
    records, totals = clone.join_plan(lengths, gap)
    assert len(records) == len(totals) == len(lengths)
    for segs, recs, total in zip(lengths, records, totals):
        # brute force: walk the utterance sample by sample, as the reference's list of samples grows
        owner, at = [], 0
        for s, n in enumerate(segs):
            owner += [("seg", s)] * n + [("gap", s)] * gap
        assert total == len(owner) == sum(segs) + gap * len(segs)
        assert len(recs) == len(segs)
        covered = np.zeros(total, dtype=np.int64)
        for s, (n, off, g) in enumerate(recs):
            assert (n, g) == (segs[s], gap) and 0 <= off and off + n + g <= total
            assert all(o == ("seg", s) for o in owner[off:off + n])
            assert all(o == ("gap", s) for o in owner[off + n:off + n + g])
            covered[off:off + n + g] += 1
        assert (covered == 1).all()                 # no overlap, no hole: the records tile the utterance


def test_join_plan_takes_a_gap_per_utterance_and_rejects_bad_arguments():
    records, totals = clone.join_plan([[10, 20], [30]], [3, 0])
    assert records == [[(10, 0, 3), (20, 13, 3)], [(30, 0, 0)]] and totals == [36, 30]
    with pytest.raises(ValueError):
        clone.join_plan([[1]], [1, 2])
    with pytest.raises(ValueError):
        clone.join_plan([[1]], -1)
    with pytest.raises(ValueError):
        clone.join_plan([[-1]], 0)


@pytest.mark.parametrize("speed", [0.7, 1.0, 2.0])
def test_join_segments_host_equals_audio_numpy_concat(speed):
    rng = np.random.default_rng(int(speed * 10))
    sr = 22050
    utterances = [[rng.standard_normal(n).astype(np.float32) for n in segs] for segs in ([256, 768], [0, 5], [1024])]
    gap = clone.gap_samples(sr, speed)
    assert gap == int((sr * 0.05) / speed)
    got = clone.join_segments_host(utterances, gap)
    for segs, g in zip(utterances, got):
        want = api.BaseSpeakerTTS.audio_numpy_concat(segs, sr=sr, speed=speed)
        assert g.dtype == np.float64 and np.array_equal(g.astype(np.float32), want)
    assert clone.join_segments_host([[]], gap)[0].shape == (0,)


def _check_batches(lengths, keys, m):
    batches = clone.sentence_batches(lengths, keys, m)
    seen = [item for _, items in batches for item in items]
    assert sorted(seen) == sorted((r, s) for r, lens in enumerate(lengths) for s in range(len(lens)))
    assert len(seen) == len(set(seen))                                  # every sentence exactly once
    for key, items in batches:
        assert 1 <= len(items) <= m
        assert all(keys[r] == key for r, _ in items)                    # speeds (and speakers) never mixed
    return batches


def test_sentence_batches_partition_is_deterministic_and_never_mixes_keys():
    rng = np.random.default_rng(3)
    lengths = [list(rng.integers(1, 120, size=int(k))) for k in rng.integers(1, 7, size=23)]
    keys = [((1.0, 1), (1.3, 1), (1.0, 2))[int(i)] for i in rng.integers(0, 3, size=23)]
    for m in (1, 2, 5, 32, 1000):
        batches = _check_batches(lengths, keys, m)
        assert batches == clone.sentence_batches([list(l) for l in lengths], list(keys), m)
        for key in set(keys):        # longest first inside a key: only its last batch may be short, padding stays small
            own = [items for k, items in batches if k == key]
            assert all(len(items) == m for items in own[:-1])
            flat = [lengths[r][s] for items in own for r, s in items]
            assert flat == sorted(flat, reverse=True)
    assert clone.sentence_batches([], [], 4) == []
    with pytest.raises(ValueError):
        clone.sentence_batches([[1]], [(1.0, 0)], 0)
    with pytest.raises(ValueError):
        clone.sentence_batches([[1]], [], 4)


def test_sentence_batches_of_the_documented_example():
    # requests of 1, 3 and 2 sentences, the second at its own speed
    batches = clone.sentence_batches([[11], [5, 23, 9], [17, 17]], [(1.0, 1), (1.3, 1), (1.0, 1)], 32)
    assert batches == [((1.0, 1), [(2, 0), (2, 1), (0, 0)]), ((1.3, 1), [(1, 1), (1, 2), (1, 0)])]
    assert [len(i) for _, i in clone.sentence_batches([[11], [5, 23, 9], [17, 17]], [(1.0, 1)] * 3, 4)] == [4, 2]


def test_symbol_is_declared_in_the_header_and_both_bindings():
    name = "ov_join_segments_f32"
    with open(os.path.join(REPO, "include", "openvoice_amd.h")) as fh:
        header = fh.read()
    assert f"int {name}(const float* src, int64_t src_elems, const int64_t* records, int R, float* dst," in header
    assert "openvoice/api.py:56-63" in header            # the reference lines it replaces
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 8
    with open(os.path.join(REPO, "openvoice_amd", "csrc", "torch_shim.cpp")) as fh:
        assert f'bind_device<&{name}>(m, "{name[3:]}")' in fh.read()
    with open(os.path.join(REPO, "openvoice_amd", "csrc", "Makefile")) as fh:
        assert "clone.hip" in fh.read()
    with open(os.path.join(REPO, "openvoice_amd", "csrc", "clone.hip")) as fh:
        assert f'extern "C" int {name}(' in fh.read()
    assert _lib.MIN_VERSION == 212                        # additive: found by name, no version change


def _stub(device, sr=22050):
    hps = types.SimpleNamespace(data=types.SimpleNamespace(sampling_rate=sr, hop_length=256),
                                speakers={"default": 1, "whispering": 2})
    return types.SimpleNamespace(device=device, hps=hps, watermark_model=None)


def test_voice_cloner_argument_errors():
    with pytest.raises(ValueError, match="one device"):
        clone.VoiceCloner(_stub("cuda:0"), _stub("cuda:1"))
    vc = clone.VoiceCloner(_stub("cuda"), _stub("cuda:0", sr=16000))     # "cuda" is device 0; rates may differ
    assert vc.tts_sr == 22050 and vc.hop == 256
    se = np.zeros((1, 256, 1), dtype=np.float32)
    two = ([[1, 2, 3], [4, 5]], "default", se, se)
    z = np.zeros((2, 3), dtype=np.float32)
    # every check below fails before any device work (the stubs have no model)
    with pytest.raises(ValueError, match="one list per request"):
        vc.speak_ids_many([two], noise_w=[[z, z], [z]])
    with pytest.raises(ValueError, match="one tensor per sentence"):
        vc.speak_ids_many([two], noise_w=[[z]])
    with pytest.raises(ValueError, match="one tensor per sentence"):
        vc.speak_ids_many([two], noise_z=[[z, z, z]])
    with pytest.raises(ValueError, match="per request"):
        vc.speak_ids_many([two], noise=[z, z])
    with pytest.raises(ValueError, match="output_paths"):
        vc.speak_ids_many([two], output_paths=["a.wav", "b.wav"])
    with pytest.raises(ValueError, match="at least one sentence"):
        vc.speak_ids_many([([], "default", se, se)])
    with pytest.raises(ValueError, match="at least one sentence"):
        vc.speak_ids_many([([[1], []], "default", se, se)])
    with pytest.raises(ValueError, match="speed"):
        vc.speak_ids_many([two + (0.0,)])
    with pytest.raises(ValueError, match="out_sr"):
        vc.speak_ids_many([two + (1.0, 0)])
    with pytest.raises(KeyError):
        vc.speak_ids_many([([[1]], "nobody", se, se)])
    with pytest.raises(ValueError):
        vc.speak_ids_many([two[:3]])
    assert vc.speak_ids_many([]) == []
    assert vc._speaker_id("whispering") == 2 and vc._speaker_id(7) == 7


def test_speak_raises_without_a_text_front_end():
    tts = _stub("cuda:0")
    tts.hps.symbols, tts.hps.data.add_blank, tts.hps.data.text_cleaners = ["a"], True, ["x"]
    for name in ("language_marks", "split_sentences_into_pieces", "get_text"):
        setattr(tts, name, getattr(api.BaseSpeakerTTS, name))
    tts.text_to_ids = types.MethodType(api.BaseSpeakerTTS.text_to_ids, tts)
    vc = clone.VoiceCloner(tts, _stub("cuda:0"))
    assert api.BaseSpeakerTTS.text_to_sequence is None
    with pytest.raises(RuntimeError, match="no text front end registered"):
        vc.speak("Hello there.", "default", None, None)
    with pytest.raises(RuntimeError, match="no text front end registered"):
        vc.speak_many(["Hello there."], "default", None, None)


def test_join_entry_point_rejects_bad_arguments_without_a_gpu():
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_float * 8)()
    rec = (ctypes.c_int64 * 4)(0, 4, 0, 0)
    p, r = ctypes.addressof(buf), ctypes.addressof(rec)
    bad = [(None, 8, r, 1, p, 8, 4), (p, 8, None, 1, p, 8, 4), (p, 8, r, 1, None, 8, 4), (p, 8, r, 0, p, 8, 4),
           (p, 8, r, 65536, p, 8, 4), (p, 0, r, 1, p, 8, 4), (p, 8, r, 1, p, 0, 4), (p, 8, r, 1, p, 8, -1)]
    for args in bad:
        assert lib.ov_join_segments_f32(*args, None) == -1, args          # OV_E_BADARG, nothing launched
    assert lib.ov_join_segments_f32(p + 2, 4, r, 1, p, 8, 4, None) == -3   # OV_E_ALIGN
