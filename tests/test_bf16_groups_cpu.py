"""Host side of the length-grouped bf16 generator (openvoice_amd/bf16.py ``plan_groups`` / ``group_records``, the
``generator=`` keyword, and the host checks of csrc/ragged_bf16.hip).  No GPU: the planner is pure Python, the record
layouts have host mirrors, the entry points refuse bad arguments before any launch."""
import ctypes
import itertools
import os
import random

import pytest
import torch

from openvoice_amd import _lib, bf16
from openvoice_amd.bf16 import group_records, pack_groups_host, plan_cost, plan_groups, unpack_groups_host

lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason="libopenvoice_amd.so not built (run __graft_entry__.build())")
MARGIN = 16


def _cases(n_cases=60, max_items=24):
    rng = random.Random(7)
    for _ in range(n_cases):
        B = rng.randint(1, max_items)
        Td = rng.randint(1, 300)
        lens = [rng.randint(0, Td) for _ in range(B)]
        if rng.random() < 0.5:
            lens[rng.randrange(B)] = Td                        # as in infer: Td is the longest item's length
        if rng.random() < 0.2:
            lens = [lens[0]] * B
        yield lens, Td, rng.randint(1, 9), rng.choice([0, 1, 37, 64, 500, 10 ** 6])


# ---- the planner -----------------------------------------------------------------------------------------------------
def test_plan_is_a_partition_that_covers_every_item_within_max_groups():
    for lens, Td, G, gc in _cases():
        plan = plan_groups(lens, Td, MARGIN, G, gc)
        assert sorted(b for idx, _ in plan for b in idx) == list(range(len(lens)))
        assert 1 <= len(plan) <= G
        for idx, L in plan:
            assert idx and 1 <= L <= Td
            for b in idx:
                assert L >= min(Td, lens[b] + MARGIN), (lens, Td, G, gc, plan)
            assert L == max(1, min(Td, max(lens[b] for b in idx) + MARGIN))
        # ascending by length, ties in batch order (a stable sort)
        flat = [b for idx, _ in plan for b in idx]
        assert flat == sorted(range(len(lens)), key=lambda b: lens[b])
        assert [L for _, L in plan] == sorted(L for _, L in plan)


def test_plan_costs_no_more_than_one_group_and_is_deterministic():
    for lens, Td, G, gc in _cases():
        plan = plan_groups(lens, Td, MARGIN, G, gc)
        one = plan_groups(lens, Td, MARGIN, 1, gc)
        assert len(one) == 1 and plan_cost(plan, gc) <= plan_cost(one, gc)
        assert plan_groups(list(lens), Td, MARGIN, G, gc) == plan
        assert plan_groups(tuple(lens), Td, MARGIN, G, float(gc)) == plan


def test_plan_cost_equals_brute_force_over_all_contiguous_cuts():
    rng = random.Random(11)
    for _ in range(300):
        B = rng.randint(1, 7)
        Td = rng.randint(1, 120)
        lens = [rng.randint(0, Td) for _ in range(B)]
        G, gc = rng.randint(1, 7), rng.choice([0, 1, 5, 16, 40, 200])
        order = sorted(range(B), key=lambda b: lens[b])
        best = None
        for k in range(0, min(G, B)):                         # k cuts -> k + 1 groups
            for cuts in itertools.combinations(range(1, B), k):
                edges = [0, *cuts, B]
                cost = sum((e - s) * max(1, min(Td, lens[order[e - 1]] + MARGIN)) + gc for s, e in zip(edges, edges[1:]))
                best = cost if best is None else min(best, cost)
        plan = plan_groups(lens, Td, MARGIN, G, gc)
        assert plan_cost(plan, gc) == best, (lens, Td, G, gc, plan)


def test_one_group_is_the_padded_run():
    for lens, Td, _, gc in _cases():
        (idx, L), = plan_groups(lens, Td, MARGIN, 1, gc)
        assert sorted(idx) == list(range(len(lens)))
        assert L == min(Td, max(lens) + MARGIN)
        if max(lens) == Td:                                    # infer's case: Td IS the longest length
            assert L == Td
    assert plan_groups([3, 20, 21, 47, 64], 64, MARGIN, 1, 64) == [([0, 1, 2, 3, 4], 64)]
    # equal lengths plan one group whatever max_groups allows; a huge group cost does too
    assert plan_groups([40] * 6, 40, MARGIN, 8, 0) == [(list(range(6)), 40)]
    assert len(plan_groups([3, 20, 21, 47, 64], 64, MARGIN, 8, 10 ** 9)) == 1
    # free groups: one per distinct computed length
    assert [L for _, L in plan_groups([3, 20, 21, 47, 64], 64, MARGIN, 8, 0)] == [19, 36, 37, 63, 64]
    assert plan_groups([], 10, MARGIN, 3, 5) == []
    for bad in (dict(Td=0), dict(margin=-1), dict(max_groups=0), dict(group_cost=-1)):
        kw = dict(Td=10, margin=MARGIN, max_groups=2, group_cost=4, **{})
        kw.update(bad)
        with pytest.raises(ValueError):
            plan_groups([1, 2], **kw)


def test_defaults_are_bounded():
    assert 1 <= bf16.DEFAULT_MAX_GROUPS <= bf16.MAX_GROUPS_CAP == 8 and bf16.DEFAULT_GROUP_COST >= 0


# ---- the record layouts ----------------------------------------------------------------------------------------------
def test_host_mirror_of_the_two_record_layouts_round_trips():
    C, spf = 16, 4
    for case, (lens, Td, G, gc) in enumerate(_cases(25, 9)):
        B, ld = len(lens), Td + 3
        plan = plan_groups(lens, Td, MARGIN, G, gc)
        pack, unpack, x_off, o_off, x_elems, o_elems = group_records(plan, lens, Td, C, ld, spf)
        assert len(pack) == len(unpack) == B and all(len(r) == bf16.PACK_FIELDS for r in pack)
        assert all(len(r) == bf16.UNPACK_FIELDS for r in unpack)
        # the groups tile the two arenas exactly, without overlap
        spans = sorted((r[2], r[2] + r[4] * C) for r in pack)
        assert spans[0][0] == 0 and spans[-1][1] == x_elems and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        rows = sorted((r[1], r[1] + r[3]) for r in unpack)
        assert rows == [(b * Td * spf, (b + 1) * Td * spf) for b in range(B)]
        gen = torch.Generator().manual_seed(case)
        z = torch.randn(B, C, ld, generator=gen)
        for b, n in enumerate(lens):
            z[b, :, n:] = float("nan")                          # never read
        x = pack_groups_host(z.reshape(-1), pack, C, torch.full((x_elems + 5,), float("nan"), dtype=torch.bfloat16))
        assert torch.isnan(x[x_elems:].float()).all() and not torch.isnan(x[:x_elems].float()).any()
        # a stand-in for the generator: every frame's first channel, spf times
        o_groups = torch.full((o_elems,), float("nan"))
        for (idx, L), xo, oo in zip(plan, x_off, o_off):
            xg = x[xo:xo + len(idx) * L * C].view(len(idx), L, C).float()
            o_groups[oo:oo + len(idx) * L * spf] = xg[:, :, 0].repeat_interleave(spf, dim=1).reshape(-1)
        o = unpack_groups_host(o_groups, unpack, torch.full((B * Td * spf,), float("nan"))).view(B, Td * spf)
        for b, n in enumerate(lens):
            want = z[b, 0, :n].to(torch.bfloat16).float().repeat_interleave(spf)
            assert torch.equal(o[b, :n * spf], want) and (o[b, n * spf:] == 0).all()


def test_host_mirrors_skip_records_the_kernels_skip():
    C = 8
    src = torch.arange(C * 10, dtype=torch.float32)
    dst = torch.full((64,), 7.0, dtype=torch.bfloat16)
    bad = [(0, 10, 0, 5, 4), (0, 10, 0, -1, 4), (-1, 10, 0, 1, 4), (0, 10, 40, 2, 4), (0, 10, 0, 2, 0), (75, 10, 0, 6, 8)]
    assert torch.equal(pack_groups_host(src, bad, C, dst.clone()), dst)
    d32 = torch.full((16,), 7.0)
    assert torch.equal(unpack_groups_host(src, [(0, 0, 5, 4), (78, 0, 3, 4), (0, 14, 1, 3), (-1, 0, 1, 1)], d32.clone()), d32)


# ---- the keyword ---------------------------------------------------------------------------------------------------------
def test_generator_keyword_is_checked_at_every_public_entry():
    from openvoice_amd import api, clone, longform, models
    assert _lib.check_generator("fp32") == "fp32" and _lib.check_generator("bf16") == "bf16"
    assert _lib.check_generator(None, optional=True) is None
    for bad in ("fp16", None, 32, ""):
        with pytest.raises(_lib.OvError, match="generator must be"):
            _lib.check_generator(bad)
    bare = lambda cls: object.__new__(cls)          # the check comes first: no attribute of the object is touched
    model, tts, conv = bare(models.SynthesizerTrn), bare(api.BaseSpeakerTTS), bare(api.ToneColorConverter)
    win, vc = bare(longform.WindowedConverter), bare(clone.VoiceCloner)
    calls = [
        lambda g: models.SynthesizerTrn.infer(model, None, None, generator=g),
        lambda g: models.SynthesizerTrn.voice_conversion(model, None, None, None, None, generator=g),
        lambda g: tts.infer_padded([[1, 2]], 0, generator=g),
        lambda g: tts.tts_from_ids([[1, 2]], 0, generator=g),
        lambda g: tts.tts_from_ids([[1, 2]], 0, batched=True, generator=g),
        lambda g: tts.tts("text", None, "default", generator=g),
        lambda g: conv.convert_many([], None, None, generator=g),
        lambda g: win.convert_many([], [], [], generator=g),
        lambda g: vc.synthesize_many([], generator=g),
        lambda g: vc.speak_ids_many([], generator=g),
        lambda g: vc.speak_ids([[1]], 0, None, None, generator=g),
        lambda g: vc.speak_many(["text"], 0, None, None, generator=g),
        lambda g: vc.speak("text", 0, None, None, generator=g),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.OvError, match="generator must be"):
            call("fp16")
        with pytest.raises(_lib.OvError, match="generator must be"):
            call("BF16")
    import inspect
    from openvoice_amd import engine, tts_engine
    assert inspect.signature(tts_engine.TtsEngine.infer).parameters["generator"].default == "fp32"
    for fn in (engine.ConverterEngine.voice_conversion, models.SynthesizerTrn.voice_conversion,
               api.ToneColorConverter.convert_many, longform.WindowedConverter.convert_many):
        p = inspect.signature(fn).parameters["generator"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


# ---- the entry points ----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_built():
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "openvoice_amd.h")).read()
    for name in ("ov_pack_groups_cl_bf16", "ov_unpack_groups_f32"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert "models.py:272-291" in header[header.index("ragged_bf16.hip"):header.index("int ov_pack_groups_cl_bf16(")]
    assert "ragged_bf16.hip" in open(os.path.join(here, "..", "openvoice_amd", "csrc", "Makefile")).read()
    shim = open(os.path.join(here, "..", "openvoice_amd", "csrc", "torch_shim.cpp")).read()
    assert '"pack_groups_cl_bf16"' in shim and '"unpack_groups_f32"' in shim


@lib_built
def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails validation before a launch
    BADARG, ALIGN = -1, -3
    f = lib.ov_pack_groups_cl_bf16
    assert f(None, 1000, fake, 1, 192, fake, 1000, None) == BADARG
    assert f(fake, 1000, None, 1, 192, fake, 1000, None) == BADARG
    assert f(fake, 1000, fake, 1, 192, None, 1000, None) == BADARG
    assert f(fake, 1000, fake, -1, 192, fake, 1000, None) == BADARG
    assert f(fake, 1000, fake, 65536, 192, fake, 1000, None) == BADARG
    for C in (0, -8, 4, 12, 190, 193):
        assert f(fake, 1000, fake, 1, C, fake, 1000, None) == BADARG, C
    assert f(fake, 0, fake, 1, 192, fake, 1000, None) == BADARG
    assert f(fake, 1000, fake, 1, 192, fake, 0, None) == BADARG
    assert f(ctypes.c_void_p(4098), 1000, fake, 1, 192, fake, 1000, None) == ALIGN
    assert f(fake, 1000, fake, 1, 192, ctypes.c_void_p(4097), 1000, None) == ALIGN
    assert f(fake, 1000, fake, 0, 192, fake, 1000, None) == 0              # nothing to do, nothing launched
    u = lib.ov_unpack_groups_f32
    assert u(None, 1000, fake, 1, fake, 1000, None) == BADARG
    assert u(fake, 1000, None, 1, fake, 1000, None) == BADARG
    assert u(fake, 1000, fake, 1, None, 1000, None) == BADARG
    assert u(fake, 1000, fake, -1, fake, 1000, None) == BADARG
    assert u(fake, 1000, fake, 65536, fake, 1000, None) == BADARG
    assert u(fake, 0, fake, 1, fake, 1000, None) == BADARG
    assert u(fake, 1000, fake, 1, fake, -5, None) == BADARG
    assert u(ctypes.c_void_p(4098), 1000, fake, 1, fake, 1000, None) == ALIGN
    assert u(fake, 1000, fake, 1, ctypes.c_void_p(4098), 1000, None) == ALIGN
    assert u(fake, 1000, fake, 0, fake, 1000, None) == 0
