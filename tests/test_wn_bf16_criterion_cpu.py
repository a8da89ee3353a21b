"""CPU gate of the bf16 WaveNet layer's acceptance criterion (tests/wn_bf16_ref.py): it accepts an honest fp32
restatement of ``ov_wn_layer_bf16`` (bf16-rounded operands, fp32 PyTorch convs and gate, one ``.bfloat16()`` of acts), it
rejects every one-line mistake a kernel of this kind can make, and the inputs the GPU tests use keep the share of
``acts`` elements that may legitimately round either way small.  No GPU, no kernel: reference against reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wn_bf16_ref as R  # noqa: E402

CASES = [(1, 17, dict()), (3, 130, dict()), (3, 129, dict(first=True)), (3, 16, dict(last=True)),
         (1, 15, dict(first=True, last=True)), (3, 3, dict(cond=None)), (3, 2, dict(cond="broadcast")), (1, 1, dict())]


def test_g_is_four_times_the_measured_gate_error():
    """G's provenance (tests/wn_bf16_ref.py): 4 x the largest |fp32 tanh * sigmoid - float64| over the parametrised
    cases and five seeds, and of the size of the header's prior for the hardware gate (<= 4e-7 absolute)."""
    worst = max(R.measure_g().values())
    print(f"[wn bf16 criterion] gate fp32 against float64: largest {worst:.3e}; G = {R.G:.3e}")
    assert 4 * worst <= R.G * 1.001 and R.G <= 4 * worst * 1.02
    assert 0.5 * 4e-7 <= R.G <= 2 * 4e-7


@pytest.mark.parametrize("B,T,kw", CASES)
def test_accepts_the_fp32_restatement(B, T, kw):
    worst = 0.0
    for seed in range(R.SEEDS):
        c = R.case(B, T, seed, **kw)
        got = R.layer(c, dtype=torch.float32)
        worst = max(worst, R.check(got["out"], got["skip"], R.layer(c), f"stand-in B={B} T={T} {kw} seed={seed}"))
    print(f"[wn bf16 criterion] fp32 stand-in B={B} T={T} {kw}: worst err / lim {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_rejects_the_mutant(mutant):
    kw = dict(first=True) if mutant == "first_ignored" else dict(last=True) if mutant == "last_writes_out" else {}
    c = R.case(3, 130, 0, **kw)
    ref = R.layer(c)
    got = R.layer(c, dtype=torch.float32, mutant=mutant)
    before = torch.full_like(c["x"], float("nan"))           # what the out buffer held before a last layer
    with pytest.raises(AssertionError):
        R.check(got["out"], got["skip"], ref, mutant, out_before=before)
    good = R.layer(c, dtype=torch.float32)                   # ... and the same case passes unbroken
    assert R.check(good["out"], good["skip"], ref, "unbroken", out_before=before) <= 1.0


def test_ambiguous_share_of_acts_stays_small():
    """A condition on the INPUTS, checked with the reference alone: at most 2 % of ``acts`` lie so close to a bf16
    rounding midpoint that fp32 and float64 may round them differently (beyond that, ``flip`` would excuse too much)."""
    worst = 0.0
    for B in R.BATCHES:
        for T in R.LENGTHS:
            for seed in range(R.SEEDS):
                worst = max(worst, R.layer(R.case(B, T, seed))["share"])
    print(f"[wn bf16 criterion] largest ambiguous share of acts {100 * worst:.2f} %")
    assert worst <= 0.02


def test_acts_of_the_stand_in_are_within_half_a_bf16_ulp():
    """The intermediate itself, with the generator criterion's ``limit``: bf16(fp32 gate) against the float64 gate."""
    c = R.case(3, 130, 1)
    r = lambda v: v.to(torch.bfloat16).float()
    pre = torch.nn.functional.conv1d(r(c["x"]), r(c["w_in"]), c["b_in"], padding=2) + c["g"][:, :, None]
    a32 = r(torch.tanh(pre[:, :R.H]) * torch.sigmoid(pre[:, R.H:]))
    pre64 = torch.nn.functional.conv1d(r(c["x"]).double(), r(c["w_in"]).double(), c["b_in"].double(), padding=2) + c["g"].double()[:, :, None]
    a64 = torch.tanh(pre64[:, :R.H]) * torch.sigmoid(pre64[:, R.H:])
    absacc = torch.nn.functional.conv1d(r(c["x"]).double().abs(), r(c["w_in"]).double().abs(), c["b_in"].double().abs(), padding=2) \
        + c["g"].double().abs()[:, :, None]
    lim = R.limit(a64, absacc[:, :R.H] + absacc[:, R.H:] + R.G / R.S)
    R.assert_within(a32, a64, lim, "acts of the stand-in")


def test_e2e_bar_is_the_measured_deviation(synth_sd):
    """Provenance of the end-to-end bar of tests/test_gpu_wavenet_bf16_e2e.py: the fp32 oracle with the kernel's operand
    roundings hooked into its WaveNet layers against the unmodified oracle, B = 2, T = 40 and 64, five seeds."""
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    got = R.measure_e2e(synth_sd, CONVERTER_MODEL_CONFIG)
    print("[wn bf16 criterion] e2e deviations " + ", ".join(f"{k} {v:.3e}" for k, v in got.items()))
    for name, v in got.items():
        assert abs(v - R.E2E_MEASURED[name]) <= 2e-2 * R.E2E_MEASURED[name], (name, v)
