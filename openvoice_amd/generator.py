"""Geometry of the HiFi-GAN generator (reference: openvoice/models.py:225-291) as a function of the configuration: the
stage table, the ResBlock conv walk, the receptive-field bound and the ConvTranspose phase split.  Pure host code, no
device work; the fp32 engine, the bf16 generator, the live units and the long-form planner all read it from here."""
import collections
import math

import torch

# Length-aware work lists (``skip_padding``): the generator's one-sided receptive field is 13.3 frames -- conv_pre 3,
# the four transposed convs 1 + 1/8 + 1/64 + 1/128, the MRF 60 samples per stage (k = 11: dilations 1, 3, 5 + three
# dilation-1 convs = 5 * (1 + 3 + 5 + 3)) at 8 / 64 / 128 / 256 samples per frame, conv_post 3 samples (reference:
# openvoice/models.py:225-291, modules.py:221-309) -- so computing length + 16 frames leaves the first ``length``
# frames bit-identical to the full computation.
GENERATOR_MARGIN = 16   # the released configuration's; every engine computes its own (generator_margin_frames)
LRELU_SLOPE = 0.1       # reference: openvoice/modules.py:14
FINAL_LRELU_SLOPE = 0.01  # F.leaky_relu default at openvoice/models.py:287

Stage = collections.namedtuple("Stage", "index cin ch stride rate_in rate_out last")
ResblockConv = collections.namedtuple("ResblockConv", "stage j n ch K dil prefix")


def generator_stages(cfg):
    """One record per upsampling stage (models.py:244-256, :278-286): ``cin`` -> ``ch`` channels through a ConvTranspose
    of ``stride``, ``rate_in`` / ``rate_out`` columns per frame before / after it, ``last`` on the stage conv_post reads."""
    rates = list(cfg["upsample_rates"])
    ch, rate, stages = cfg["upsample_initial_channel"], 1, []
    for i, u in enumerate(rates):
        stages.append(Stage(i, ch, ch // 2, u, rate, rate * u, i == len(rates) - 1))
        ch, rate = ch // 2, rate * u
    return stages


def samples_per_frame(cfg):
    return generator_stages(cfg)[-1].rate_out


def scratch_per_frame(cfg):
    """Elements per frame of the largest stage tensor (``ch * rate_out``): what sizes the decoder scratch."""
    return max(st.ch * st.rate_out for st in generator_stages(cfg))


def resblock_convs(cfg):
    """The ResBlock1 (dilated conv, plain conv) pairs in checkpoint order: stage, ResBlock ``j`` of the stage, pair ``n``
    of the ResBlock, with the channels, kernel size and dilation of the dilated conv.  ``prefix`` is the ResBlock's
    (``dec.resblocks.R``, R = stage * kernels + j): the pair's weights are ``{prefix}.convs1.{n}`` (dilation ``dil``) and
    ``{prefix}.convs2.{n}`` (dilation 1)."""
    kernels, dils = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    for st in generator_stages(cfg):
        for j, (K, rd) in enumerate(zip(kernels, dils)):
            for n, d in enumerate(rd):
                yield ResblockConv(st.index, j, n, st.ch, K, d, f"dec.resblocks.{st.index * len(kernels) + j}")


def generator_margin_frames(cfg, conv_pre_kernel=7, conv_post_kernel=7, chain_reach=None):
    """Frames beyond an utterance's end that can still influence its last sample: an UPPER BOUND of the generator's
    one-sided receptive field from the configuration (reference: openvoice/models.py:225-291 -- conv_pre, per stage a
    ConvTranspose1d of kernel k_u and stride u followed by the MRF whose widest ResBlock1 reaches
    (k - 1) / 2 * (sum(dilations) + len(dilations)) samples (modules.py:221-309: one dilated and one plain conv per
    dilation), conv_post), rounded up plus one frame of slack.  The transposed-conv term charges (k_u - u + 1) / spf
    frames per stage, more than the ceil((k_u - u) / 2 / u) + 1 inputs a stage really reaches back: the bound is loose
    by design.  15 for the released V1 / V2 configurations (``ConverterEngine`` uses max(GENERATOR_MARGIN = 16, this):
    tests/test_host_algebra_cpu.py::test_generator_margin_released_configs).  ``chain_reach(i, k, dilations)``, when
    given, replaces the ResBlock term by the samples one chain of stage ``i`` really reaches forward with the kernels that
    run it (``limit_margin_frames``)."""
    reach, spf = (conv_pre_kernel - 1) / 2.0, 1              # frames
    if chain_reach is None:
        chain_reach = lambda i, k, d: (k - 1) // 2 * (sum(d) + len(d))
    for st, ku in zip(generator_stages(cfg), cfg["upsample_kernel_sizes"]):
        spf = st.rate_out                                    # samples per frame after the stage
        reach += (ku - st.stride + 1) / 2.0 / spf * 2        # a transposed conv reaches ceil((k_u - u) / 2) + 1 inputs back
        widest = max(chain_reach(st.index, k, list(d)) for k, d in
                     zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
        reach += widest / spf
    reach += (conv_post_kernel - 1) / 2.0 / spf
    return int(math.ceil(reach)) + 1


def conv_transpose_as_conv(w, stride):
    """ConvTranspose1d(k = 2*stride, padding = stride/2) as a 3-tap stride-1 conv producing
    ``stride`` output phases per input frame.  y[s*q + p] = sum_i x[i] * w[:, :, s*q + p + pad - s*i]
    has exactly two non-zero taps per phase (i = q and i = q-1 or q+1); row = cout*stride + phase.
    ``w`` is [Cin, Cout, k] (torch ConvTranspose1d layout, reference: openvoice/models.py:244-256)."""
    cin, cout, k = w.shape
    s = stride
    pad = (k - s) // 2
    assert k == 2 * s and (k - s) % 2 == 0
    wc = torch.zeros(cout * s, cin, 3, dtype=w.dtype)
    for p in range(s):
        rows = torch.arange(cout) * s + p
        wc[rows, :, 1] = w[:, :, p + pad].t()                 # x[q]
        if p + pad < s:
            wc[rows, :, 0] = w[:, :, p + pad + s].t()         # x[q-1]
        else:
            wc[rows, :, 2] = w[:, :, p + pad - s].t()         # x[q+1]
    return wc
