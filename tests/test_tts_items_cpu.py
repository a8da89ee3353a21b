"""Per-item synthesis controls, the parts that need no GPU: the mixed pooling of ``clone.sentence_batches``, the
argument checks of the two ``_items`` C entry points, and the validation of the Python layers
(``tts_engine.item_controls``, ``BaseSpeakerTTS.per_sentence``)."""
import os

import numpy as np
import pytest
import torch

from openvoice_amd import _lib, api, clone, tts_engine

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason="libopenvoice_amd.so not built (run __graft_entry__.build())")


# ---- clone.sentence_batches(mixed=True) --------------------------------------------------------------------------------
def _case(seed, n_requests):
    rng = np.random.default_rng(seed)
    lengths = [[int(n) for n in rng.integers(1, 9, rng.integers(1, 5))] for _ in range(n_requests)]   # many ties
    keys = [(float(rng.choice([0.8, 1.0, 1.3])), int(rng.integers(0, 3))) for _ in range(n_requests)]
    return lengths, keys


@pytest.mark.parametrize("seed,n_requests,cap", [(0, 1, 32), (1, 7, 4), (2, 12, 5), (3, 9, 1), (4, 6, 32)])
def test_mixed_batches_hold_every_sentence_once_longest_first_within_the_cap(seed, n_requests, cap):
    lengths, keys = _case(seed, n_requests)
    batches = clone.sentence_batches(lengths, keys, cap, mixed=True)
    assert all(key is None for key, _ in batches)
    flat = [item for _, items in batches for item in items]
    every = [(r, s) for r, lens in enumerate(lengths) for s in range(len(lens))]
    assert sorted(flat) == every and len(set(flat)) == len(flat)
    # one pool, longest first; ties by request, then sentence -- the rule of the keyed pools
    assert flat == sorted(every, key=lambda rs: (-lengths[rs[0]][rs[1]], rs[0], rs[1]))
    # cut at the cap: every batch full but the last
    sizes = [len(items) for _, items in batches]
    assert all(n == cap for n in sizes[:-1]) and 1 <= sizes[-1] <= cap
    assert batches == clone.sentence_batches([list(l) for l in lengths], list(keys), cap, mixed=True)


def test_mixed_false_is_the_keyed_partition():
    for seed, n_requests, cap in [(0, 1, 32), (1, 7, 4), (2, 12, 5), (3, 9, 1)]:
        lengths, keys = _case(seed, n_requests)
        keyed = clone.sentence_batches(lengths, keys, cap)
        assert clone.sentence_batches(lengths, keys, cap, mixed=False) == keyed
        assert all(key in keys for key, _ in keyed)
    assert clone.sentence_batches([[3, 1]], [(1.0, 0)]) == clone.sentence_batches([[3, 1]], [(1.0, 0)], mixed=False)


def test_mixed_batches_of_a_small_example_and_bad_arguments():
    # requests of three keys; the 17s tie: request 2 before request 3, sentence order inside request 2
    got = clone.sentence_batches([[11], [5, 23, 9], [17, 17], [17]], [(1.0, 1), (1.3, 1), (1.0, 2), (0.8, 1)], 4, mixed=True)
    assert got == [(None, [(1, 1), (2, 0), (2, 1), (3, 0)]), (None, [(0, 0), (1, 2), (1, 0)])]
    assert clone.sentence_batches([], [], 4, mixed=True) == []
    with pytest.raises(ValueError):
        clone.sentence_batches([[1]], [(1.0, 0)], 0, mixed=True)
    with pytest.raises(ValueError):
        clone.sentence_batches([[1]], [], 4, mixed=True)


# ---- the C entry points reject bad arguments before any launch ----------------------------------------------------------
@needs_lib
def test_items_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    bufs = {k: torch.zeros(64) for k in ("z", "dp", "mask", "logw", "ratio", "scale")}
    bufs["cum"], bufs["ylen"] = torch.zeros(64, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    p = {k: v.data_ptr() for k, v in bufs.items()}

    def duration(B=1, T=8, ld=8, **null):
        q = dict(p, **{k: None for k in null})
        return lib.ov_duration_items_f32(q["z"], 2 * ld, 0.1, -0.2, q["dp"], 32 * ld, q["mask"], q["logw"], q["cum"],
                                         q["ylen"], B, T, ld, q["ratio"], q["scale"], None)

    for name in ("z", "dp", "mask", "logw", "cum", "ylen", "ratio", "scale"):
        assert duration(**{name: True}) == -1, name
    assert duration(B=0) == -1 and duration(B=-1) == -1 and duration(T=0) == -1 and duration(T=8, ld=7) == -1

    ebufs = {k: torch.zeros(64) for k in ("m", "logs", "noise", "zp", "mp", "lp", "attn", "ns")}
    ebufs["cum"] = torch.zeros(64, dtype=torch.int32)
    ebufs["xlen"], ebufs["ylen"] = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    e = {k: v.data_ptr() for k, v in ebufs.items()}

    def expand(B=1, C=2, Tx=4, Ty=4, ldx=4, ldy=4, ldn=4, tok_bstride=None, **null):
        q = dict(e, **{k: None for k in null})
        return lib.ov_expand_prior_items_f32(q["m"], q["logs"], 2 * C * ldx if tok_bstride is None else tok_bstride, ldx,
                                             q["cum"], q["xlen"], q["ylen"], q["noise"], C * ldn, ldn, q["zp"], q["mp"],
                                             q["lp"], q["attn"], B, C, Tx, Ty, ldy, q["ns"], None)

    for name in ("m", "logs", "cum", "xlen", "ylen", "noise", "zp", "ns"):
        assert expand(**{name: True}) == -1, name
    for bad in (dict(B=0), dict(C=0), dict(Tx=0), dict(Ty=0), dict(Tx=5), dict(Ty=5), dict(Ty=4, ldn=3), dict(B=65536),
                dict(tok_bstride=7)):
        assert expand(**bad) == -1, bad


# ---- tts_engine.item_controls -------------------------------------------------------------------------------------------
def test_item_controls_plain_numbers_are_the_scalar_path():
    assert tts_engine.item_controls(3, 0.667, 1.0, 0.6, 0.2) is None
    assert tts_engine.item_controls(3, 1, np.float32(1.25), torch.tensor(0.6), np.float64(0.2)) is None


def test_item_controls_broadcast_and_accept_sequences_and_tensors():
    got = tts_engine.item_controls(3, 0.667, [1.25, 1.0, 0.5], torch.tensor([0.6, 0.0, 1.0]), np.array([0.0, 0.2, 1.0]))
    assert list(got) == list(tts_engine.CONTROLS)
    assert got["noise_scale"] == [0.667] * 3 and got["length_scale"] == [1.25, 1.0, 0.5]
    assert got["noise_scale_w"] == pytest.approx([0.6, 0.0, 1.0]) and got["sdp_ratio"] == [0.0, 0.2, 1.0]
    # sdp_ratio is not confined to [0, 1]: the reference extrapolates
    assert tts_engine.item_controls(2, 1.0, 1.0, 1.0, (-0.5, 1.5))["sdp_ratio"] == [-0.5, 1.5]


@pytest.mark.parametrize("kw", [dict(length_scale=[1.0, 1.0]), dict(noise_scale=[0.5] * 4), dict(sdp_ratio=torch.zeros(2)),
                                dict(length_scale=[1.0, 0.0, 1.0]), dict(length_scale=[1.0, -2.0, 1.0]),
                                dict(length_scale=[1.0, float("nan"), 1.0]), dict(noise_scale=[0.1, float("inf"), 0.1]),
                                dict(noise_scale_w=torch.tensor([0.1, float("nan"), 0.1])),
                                dict(sdp_ratio=[0.2, float("-inf"), 0.2])])
def test_item_controls_reject_wrong_lengths_and_values(kw):
    args = dict(noise_scale=0.667, length_scale=1.0, noise_scale_w=0.6, sdp_ratio=0.2)
    args.update(kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        tts_engine.item_controls(3, **args)


# ---- BaseSpeakerTTS.per_sentence ----------------------------------------------------------------------------------------
def test_per_sentence_one_value_or_one_per_sentence():
    per = api.BaseSpeakerTTS.per_sentence
    assert per("speed", 1.3, 3, positive=True) == (False, 1.3)
    assert per("speaker_id", 7, 3, integer=True) == (False, 7)
    assert per("speed", np.float64(1.3), 3) == (False, 1.3)
    assert per("speed", [0.8, 1.0, 1.3], 3, positive=True) == (True, [0.8, 1.0, 1.3])
    assert per("speaker_id", torch.tensor([0, 3, 7]), 3, integer=True) == (True, [0, 3, 7])
    assert per("speaker_id", np.array([0, 3, 7]), 3, integer=True) == (True, [0, 3, 7])
    assert per("noise_scale", (0.0, 0.667, 1.0), 3) == (True, [0.0, 0.667, 1.0])


@pytest.mark.parametrize("name,value,kw", [("speed", [1.0, 1.0], dict(positive=True)),
                                           ("speaker_id", [0, 1, 2, 3], dict(integer=True)),
                                           ("speed", [1.0, 0.0, 1.0], dict(positive=True)),
                                           ("speed", [1.0, -1.0, 1.0], dict(positive=True)),
                                           ("speed", [1.0, float("nan"), 1.0], dict(positive=True)),
                                           ("noise_scale", [0.5, float("inf"), 0.5], {})])
def test_per_sentence_rejects_wrong_lengths_and_values(name, value, kw):
    with pytest.raises(ValueError, match=name):
        api.BaseSpeakerTTS.per_sentence(name, value, 3, **kw)


def test_public_entry_points_take_the_new_arguments():
    """The signatures the feature adds: ``mixed=False`` on the cloner, nothing new on ``tts``."""
    import inspect
    for fn in (clone.VoiceCloner.synthesize_many, clone.VoiceCloner.speak_ids_many, clone.VoiceCloner.speak_many,
               clone.VoiceCloner.speak_ids, clone.sentence_batches):
        assert inspect.signature(fn).parameters["mixed"].default is False, fn
    assert list(inspect.signature(api.BaseSpeakerTTS.tts).parameters) == [
        "self", "text", "output_path", "speaker", "language", "speed", "batched", "seed", "generator"]
