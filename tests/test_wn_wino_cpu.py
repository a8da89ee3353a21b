"""CPU gate of the Winograd-domain WaveNet layer (csrc/wn_layer_wino.hip): the k = 5 gate conv as the F(4, 3) nesting
(w0 w1 w2)(w3 w4 0) -- 11 products per 4 outputs, the (group 1, point infinity) product dropped -- emulated in fp32
(transforms as the kernel's fma sequences, the point GEMMs as k-ordered fp32 fma chains, which is what the fp32 MFMA
computes), carried through the gate non-linearity and the 1x1 res/skip conv, against float64.  The same layer with the
gate conv in the direct form (one fp32 fma chain over (tap, ci)) gives the error the fused direct kernel has on the same
inputs.  Bar (the rule of tests/test_gpu_wino.py): e_wino <= max(16 e_direct, 1e-6).

Weights: the calibrated synthetic set's WN layers (enc_q and a flow coupling); 'stress' runs the layer at the input
magnitude of the gain-4 stress model (params.stress_state_dict scales the latents that feed the flow's WaveNets 4-fold;
the WN weights themselves are the same tensors)."""
import numpy as np
import pytest
import torch

from openvoice_amd import wino
from openvoice_amd.params import effective_weight

H, K, T = 192, 5, 40
F32 = np.float32


def fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def chain(a, b, init):
    """out[m][n] = init + sum_k a[m][k] b[k][n] as ONE fp32 fma chain in k order (v_mfma_f32_*_f32 numerics)."""
    acc = np.broadcast_to(init, (a.shape[0], b.shape[1])).astype(F32).copy()
    for k in range(a.shape[1]):
        acc = fma(a[:, k:k + 1], b[k:k + 1, :], acc)
    return acc


def gate_conv_direct(w, x, bias):
    """[2H][T]: k-steps ordered (tap, ci) over a zero-padded row, as the direct kernel walks them per chunk."""
    xp = np.pad(x, ((0, 0), (2, 2)))
    a = np.concatenate([w[:, :, t] for t in range(K)], axis=1)
    b = np.concatenate([xp[:, t:t + x.shape[1]] for t in range(K)], axis=0)
    return chain(a, b, bias[:, None])


def wino_weights(w):
    """U[p][co][g][ci] in float64, rounded once (the packer): taps (w0 w1 w2)(w3 w4 0)."""
    G = np.array(wino.G, np.float64)
    w6 = np.concatenate([w.astype(np.float64), np.zeros(w.shape[:2] + (1,))], axis=2).reshape(w.shape[0], w.shape[1], 2, 3)
    return np.einsum("pk,oigk->pogi", G, w6).astype(F32)


def gate_conv_wino(w, x, bias):
    U = wino_weights(w)
    assert not U[5, :, 1].any()                      # the dropped product's weight is identically zero
    nt = (x.shape[1] + 3) // 4
    xp = np.pad(x, ((0, 0), (2, 4 * nt - x.shape[1] + 6)))
    d = np.stack([xp[:, m:m + 4 * nt:4] for m in range(9)])          # d[m][ci][tile] = x[4 tile + m - 2]
    Y = [np.zeros((w.shape[0], nt), F32) for _ in range(6)]
    Y[1] = np.broadcast_to(bias[:, None], Y[1].shape).astype(F32)    # At column of point 1 is (1, 1, 1, 1)
    for g in range(2):
        d0, d1, d2, d3, d4, d5 = (d[3 * g + m] for m in range(6))
        t1, t2, t3, t4 = fma(F32(-4), d2, d4), fma(F32(-4), d1, d3), d4 - d2, d3 - d1
        V = [fma(F32(4), d0, fma(F32(-5), d2, d4)), t1 + t2, t1 - t2, fma(F32(2), t4, t3), fma(F32(-2), t4, t3),
             fma(F32(4), d1, fma(F32(-5), d3, d5))]
        for p in range(6):
            if g == 1 and p == 5:
                continue
            Y[p] = chain(U[p, :, g], V[p], Y[p])
    s1, e1, s2, e2 = Y[1] + Y[2], Y[1] - Y[2], Y[3] + Y[4], Y[3] - Y[4]
    o = np.stack([(Y[0] + s1) + s2, fma(F32(2), e2, e1), fma(F32(4), s2, s1), fma(F32(8), e2, e1) + Y[5]], axis=2)
    return o.reshape(w.shape[0], 4 * nt)[:, :x.shape[1]]


def layer_tail(x_in, x, skip, w_rs, b_rs):
    acts = (np.tanh(x_in[:H]) * (F32(1) / (F32(1) + np.exp(-x_in[H:])))).astype(F32)
    rs = chain(w_rs[:, :, 0], acts, b_rs[:, None])
    return np.concatenate([x + rs[:H], skip + rs[H:]])


def reference(w_in, b_in, w_rs, b_rs, x, skip):
    f = lambda a: torch.from_numpy(np.asarray(a)).double()
    x_in = torch.nn.functional.conv1d(f(x)[None], f(w_in), f(b_in), padding=2)[0]
    acts = torch.tanh(x_in[:H]) * torch.sigmoid(x_in[H:])
    rs = torch.nn.functional.conv1d(acts[None], f(w_rs), f(b_rs))[0]
    return torch.cat([f(x) + rs[:H], f(skip) + rs[H:]]).numpy()


@pytest.mark.parametrize("prefix", ["enc_q.enc", "flow.flows.0.enc"])
@pytest.mark.parametrize("scale", [1.0, 4.0], ids=["calibrated", "stress"])
def test_wino_layer_error_is_within_16x_the_direct_form(synth_sd, prefix, scale):
    n = lambda t: t.detach().float().numpy()
    w_in, b_in = n(effective_weight(synth_sd, f"{prefix}.in_layers.1")), n(synth_sd[f"{prefix}.in_layers.1.bias"])
    w_rs, b_rs = n(effective_weight(synth_sd, f"{prefix}.res_skip_layers.1")), n(synth_sd[f"{prefix}.res_skip_layers.1.bias"])
    assert w_in.shape == (2 * H, H, K) and w_rs.shape == (2 * H, H, 1)
    rng = np.random.default_rng(7)
    x = (scale * rng.standard_normal((H, T))).astype(F32)
    skip = rng.standard_normal((H, T)).astype(F32)
    ref = reference(w_in, b_in, w_rs, b_rs, x, skip)
    e_d = np.abs(layer_tail(gate_conv_direct(w_in, x, b_in), x, skip, w_rs, b_rs) - ref).max()
    e_w = np.abs(layer_tail(gate_conv_wino(w_in, x, b_in), x, skip, w_rs, b_rs) - ref).max()
    print(f"{prefix} x{scale}: e_wino {e_w:.3e}  e_direct {e_d:.3e}  ratio {e_w / e_d:.2f}")
    assert e_w <= max(16 * e_d, 1e-6), (e_w, e_d)


def test_only_the_second_group_exercises_the_dropped_product():
    """Weights with w0 = w1 = w2 = 0: the whole conv goes through group 1, whose point-infinity product is never issued."""
    rng = np.random.default_rng(3)
    w = np.zeros((2 * H, H, K), F32)
    w[:, :, 3:] = rng.standard_normal((2 * H, H, 2)).astype(F32) * (2 * H) ** -0.5
    x, b = rng.standard_normal((H, T)).astype(F32), np.zeros(2 * H, F32)
    ref = torch.nn.functional.conv1d(torch.from_numpy(x).double()[None], torch.from_numpy(w).double(), padding=2)[0].numpy()
    e_d = np.abs(gate_conv_direct(w, x, b) - ref).max()
    e_w = np.abs(gate_conv_wino(w, x, b) - ref).max()
    assert e_w <= max(16 * e_d, 1e-6), (e_w, e_d)
