#!/usr/bin/env python3
"""Throughput of the tone-colour-converter hot path on MI355X.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1] / configs[2]): per GPU a batch of 32 synthetic 10 s utterances at
22.05 kHz (220 500 samples -> T = 861 frames), converter model of the released hyper-parameters
with calibrated random weights, fp32.  One step = waveform already resident in HBM -> linear
spectrogram -> posterior encoder -> flow (src forward, tgt reverse) -> HiFi-GAN generator -> waveform
in HBM, including the per-batch RCCL broadcast of the packed src/tgt speaker embeddings when N > 1.
Prints ONE JSON line on rank 0 (contract in the task statement): value = aggregate real-time factor
(audio seconds produced per wall second over all GPUs).

A plain run only sets up, warms up, times the --steps steps (--dump-outputs DIR: writes what the last one returned)
and prints the line.  --full adds everything else after the timed region: roofline and per-kernel-group times, the
PCIe-inclusive rate, the opt-in split-precision line, configs[3] / [4], the oracle self-check and the CPU baseline.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FP32_MFMA_PEAK_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak, same guide (power-limited to ~1.7-1.8 PF/s on real operands)
PMC_TRAFFIC_FILE = os.path.join(REPO, "profiles", "pmc_traffic_latest.json")


def mrf_alg_bytes_per_launch(cfg, B, frames, fused=()):
    """Algorithmic HBM bytes of the average MRF launch: per ResBlock pair as two launches conv1
    reads x and writes t (2 tensor passes), conv2 reads t and the residual and writes (3); as ONE fused launch
    (``fused`` = the (channels, kernel) set the engine fuses) x is read and the output written (2); the last pair of
    ResBlocks 2 and 3 also reads the running MRF sum (+1 each); tensor = B * C * L * 4 bytes per stage."""
    ch, L, total, launches = cfg["upsample_initial_channel"], frames, 0.0, 0
    kernels, nd = cfg["resblock_kernel_sizes"], len(cfg["resblock_dilation_sizes"][0])
    for u in cfg["upsample_rates"]:
        ch //= 2
        L *= u
        for j, k in enumerate(kernels):
            one = (ch, k) in fused
            passes = nd * (2 if one else 5) + (1 if j > 0 else 0)
            total += passes * 4.0 * B * ch * L
            launches += nd * (1 if one else 2)
    return total / launches


def pmc_traffic(batch, frames, fuse_pairs, pair_policy, launches_per_step, chain_streams=1):
    """HBM bytes per MRF launch measured with rocprofv3 PMC counters in a separate run of this same command
    (scripts/gpu_r4_profile.sh, tools/pmc_traffic.py).  Reported only when the record was taken on the SAME kernel
    sources, workload shape and fusion policy as this run (``launch_config_digest``) AND counted the same number of
    MRF launches per step as this run just issued; otherwise None plus the reason -- a figure measured on another
    launch sequence is not a measurement of this one."""
    from openvoice_amd.hostinfo import launch_config_digest
    try:
        with open(PMC_TRAFFIC_FILE) as fh:
            rec = json.load(fh)
        have = rec.get("launch_config_digest")
        want = launch_config_digest(batch, frames, fuse_pairs, pair_policy, chain_streams)
        if have != want:
            return None, (f"profiles/pmc_traffic_latest.json was measured on launch configuration {have} "
                          f"(kernel sources {rec.get('kernel_source_digest')}), this run is {want}")
        if rec.get("launches_per_step") != launches_per_step:
            return None, (f"profiles/pmc_traffic_latest.json counted {rec.get('launches_per_step')} MRF launches per "
                          f"step, this run issued {launches_per_step}")
        return (rec.get("calibrated", rec["nominal"])["bytes_per_launch"],
                f"PMC passes of launch configuration {have}, {launches_per_step} MRF launches per step")
    except (OSError, KeyError, ValueError):
        return None, "no PMC record committed"


def bf16_counter_record(batch, frames):
    """The committed rocprofv3 counter record of the opt-in bf16 generator (tools/bf16_counters.py ->
    profiles/bf16_counters_latest.json): HBM traffic per pass, matrix-busy fraction, shader clock.  Returned only when
    it was taken on the running tree's bf16 kernel sources at this batch / frame count."""
    from openvoice_amd.hostinfo import bf16_source_digest
    path = os.path.join(REPO, "profiles", "bf16_counters_latest.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
    except (OSError, ValueError):
        return None, "no bf16 counter record committed (algorithmic bytes reported)"
    if rec.get("bf16_source_digest") != bf16_source_digest():
        return None, (f"profiles/bf16_counters_latest.json was measured on bf16 sources {rec.get('bf16_source_digest')}, this "
                      f"tree is {bf16_source_digest()} (algorithmic bytes reported)")
    if (rec.get("batch"), rec.get("frames")) != (batch, frames):
        return None, (f"profiles/bf16_counters_latest.json is for batch {rec.get('batch')} x {rec.get('frames')} frames, this run "
                      f"is {batch} x {frames} (algorithmic bytes reported)")
    return rec, "rocprofv3 PMC passes, profiles/bf16_counters_latest.json (FETCH_SIZE x 2 + WRITE_SIZE, calibrated)"


def split_traffic_record(batch, frames, products):
    """The committed PMC traffic record of the split-precision conv launches (tools/pmc_traffic_split.py ->
    profiles/split3_traffic_latest.json), returned only when it was taken on the running tree's split kernel sources at
    this batch / frame count / product count."""
    from openvoice_amd.hostinfo import split3_source_digest
    path = os.path.join(REPO, "profiles", "split3_traffic_latest.json")
    try:
        with open(path) as fh:
            rec = json.load(fh)
    except (OSError, ValueError):
        return None, "no split-conv traffic record committed"
    if rec.get("split3_source_digest") != split3_source_digest():
        return None, (f"profiles/split3_traffic_latest.json was measured on split kernel sources "
                      f"{rec.get('split3_source_digest')}, this tree is {split3_source_digest()}")
    if (rec.get("batch"), rec.get("frames")) != (batch, frames):
        return None, f"profiles/split3_traffic_latest.json is for batch {rec.get('batch')} x {rec.get('frames')} frames"
    if any(i.get("products") != products for i in rec.get("instances", [])):
        return None, "profiles/split3_traffic_latest.json was measured with another product count"
    return rec, "rocprofv3 PMC passes of bench.py --split-bf16x3, profiles/split3_traffic_latest.json"


SAMPLE_RATE = 22050


def synth_wave(batch, samples, seed, device):
    """Sum of 5 random sinusoids (80-4000 Hz) + 0.01 N(0,1), peak 0.9."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    freqs = 80.0 + 3920.0 * torch.rand(batch, 5, 1, generator=gen)
    phases = 2 * torch.pi * torch.rand(batch, 5, 1, generator=gen)
    amps = 0.2 + torch.rand(batch, 5, 1, generator=gen)
    t = torch.arange(samples, dtype=torch.float32)[None, None, :] / SAMPLE_RATE
    wave = (amps * torch.sin(2 * torch.pi * freqs * t + phases)).sum(1)
    wave = wave + 0.01 * torch.randn(batch, samples, generator=gen)
    wave = 0.9 * wave / wave.abs().amax(dim=1, keepdim=True)
    return wave.to(device)


def _reference_model(sd, cfg):
    """The UNMODIFIED reference ``SynthesizerTrn`` (weight-norm left in place, re-evaluated every forward, as the
    reference runs it: openvoice/models.py:492-499) with our synthetic weights -- only where /root/reference exists
    (the build container; the GPU box has no copy).  Returns None when it cannot be imported."""
    try:
        from oracle.make_golden import REFERENCE, import_reference
        if not os.path.isdir(REFERENCE):
            return None
        import warnings
        warnings.filterwarnings("ignore")
        ref_models, ref_spectrogram = import_reference()
        model = ref_models.SynthesizerTrn(0, 513, n_speakers=0, **cfg).eval()
        model.load_state_dict(sd, strict=True)
        model.zero_g = True
        return model, ref_spectrogram
    except Exception:   # noqa: BLE001 -- any import problem means "not available here"
        return None


def cpu_baseline(sd, cfg, seconds, budget_s=20.0, want_reference=True, batch32=None):
    """CPU fp32 baseline on this box's host cores: the unmodified
    reference (``kind = "reference"``) where /root/reference is importable, else the oracle -- the CPU restatement
    of the same path in the same torch operators (``kind = "port"``; pinned to reference outputs by
    tests/test_oracle_golden.py).  Bounded sample: B = 1 utterances on all usable threads for ~budget_s (the
    headline ``value``), then one B = 1 run on ONE thread, then ONE B = 32 run of the whole benchmark batch on all threads
    when one timed B = 4 run estimates it at <= 60 s (``batch32``: None = that rule, True = ``--cpu-batch32`` forces it up to
    4 x budget, False = ``--no-cpu-batch32``); next to the reference's figure on the same host in
    profiles/r02_cpu_reference_vs_port_build_container.json."""
    from oracle import vc_oracle
    from openvoice_amd.hostinfo import cpu_model, usable_cpus
    cores = usable_cpus(32)
    samples = int(seconds * SAMPLE_RATE)
    gen = torch.Generator().manual_seed(8)
    g_src, g_tgt = 0.1 * torch.randn(1, 256, 1, generator=gen), 0.1 * torch.randn(1, 256, 1, generator=gen)
    ref = _reference_model(sd, cfg) if want_reference else None
    kind = "reference" if ref is not None else "port"

    def convert(wave):
        with torch.no_grad():
            if ref is not None:
                model, ref_spectrogram = ref
                spec = ref_spectrogram(wave, 1024, SAMPLE_RATE, 256, 1024, center=False)
                lengths = torch.full((wave.shape[0],), spec.shape[2], dtype=torch.int64)
                return model.voice_conversion(spec, lengths, g_src, g_tgt, tau=0.3)[0]
            spec = vc_oracle.spectrogram(wave)
            noise = torch.randn(wave.shape[0], cfg["inter_channels"], spec.shape[2], generator=gen)
            lengths = torch.full((wave.shape[0],), spec.shape[2], dtype=torch.int64)
            return vc_oracle.voice_conversion(sd, cfg, spec, lengths, g_src, g_tgt, 0.3, noise, zero_g=True)[0]

    wave1 = synth_wave(1, samples, 7, "cpu")
    torch.set_num_threads(cores)
    convert(wave1)   # warm-up (weight-norm is re-evaluated per call by both the reference and the port)
    n, t0 = 0, time.perf_counter()
    while True:
        convert(wave1)
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s * 0.45 or n >= 16:
            break
    out = dict(value=round(n * seconds / el, 3), unit="x real-time (audio s / wall s)", cores=cores, kind=kind,
               cpu_model=cpu_model(), utterances_per_s=round(n / el, 4))
    sample = [f"{n} x (B=1, {seconds:g} s) on {cores} threads, {el:.1f} s wall"]
    # one thread, B = 1
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    convert(wave1)
    el1 = time.perf_counter() - t0
    out["one_thread"] = dict(value=round(seconds / el1, 3), utterances_per_s=round(1.0 / el1, 4), cores=1)
    sample.append(f"1 x (B=1) on 1 thread, {el1:.1f} s")
    # the benchmark batch, B = 32 x `seconds` (SURVEY.md section 8d's CPU leg; reference: openvoice/models.py:492-499 on the
    # padded batch): run whenever the B = 4 run estimates it at <= 60 s (`batch32` None = that rule, True = also up to
    # 4 x budget_s, False = never); otherwise the bounded stand-in below
    torch.set_num_threads(cores)
    # Estimate of the B = 32 leg from ONE timed B = 4 run: the batched convs are far slower per utterance than B = 1
    # (the padded batch streams its activations through the same caches -- rounds 4 / 5 measured
    # 42-48 s where 32 x the B = 1 time said 14-19 s); from B = 4 on the per-utterance cost falls slowly again (round 6, this
    # box class: B = 4 7.0 s, B = 32 45 s = 6.4 x), hence 6.5 x the B = 4 time.
    est32_from_b1 = 32.0 * el / n
    est32 = est32_from_b1
    if batch32 is not False and seconds >= 2.0 and 4.0 * el / n <= 12.0:
        wave4 = synth_wave(4, samples, 9, "cpu")
        t0 = time.perf_counter()
        convert(wave4)
        el4 = time.perf_counter() - t0
        est32 = 6.5 * el4
        out["batch4"] = dict(value=round(4 * seconds / el4, 3), utterances_per_s=round(4.0 / el4, 4), cores=cores,
                             wall_s=round(el4, 2))
        sample.append(f"1 x (B=4) on {cores} threads, {el4:.1f} s")
    limit = 60.0 if batch32 is None else (max(60.0, 4.0 * budget_s) if batch32 else -1.0)
    out["batch32"] = None
    if est32 <= limit:
        wave32 = synth_wave(32, samples, 9, "cpu")
        t0 = time.perf_counter()
        convert(wave32)
        el32 = time.perf_counter() - t0
        out["batch32"] = dict(value=round(32 * seconds / el32, 3), utterances_per_s=round(32.0 / el32, 4), cores=cores,
                              wall_s=round(el32, 2), estimated_s=round(est32, 1), estimated_from_b1_s=round(est32_from_b1, 1))
        sample.append(f"1 x (B=32 x {seconds:g} s) on {cores} threads, {el32:.1f} s (estimated from the B=4 run: {est32:.0f} s; "
                      f"32 x the B=1 time: {est32_from_b1:.0f} s)")
    else:
        # bounded stand-in: a batch of 32 SHORT utterances (a tenth of the workload's length, >= 0.5 s) -- the same
        # batched operators and thread count, a few seconds of CPU
        short_s = max(0.5, seconds / 10.0)
        if seconds >= 2.0 and est32 * short_s / seconds <= 12.0:
            wave32 = synth_wave(32, int(short_s * SAMPLE_RATE), 9, "cpu")
            t0 = time.perf_counter()
            convert(wave32)
            el32 = time.perf_counter() - t0
            out["batch32_short"] = dict(value=round(32 * short_s / el32, 3), utterances_per_s=round(32.0 / el32, 4),
                                        utterance_s=short_s, cores=cores)
            sample.append(f"1 x (B=32 x {short_s:.1f} s) on {cores} threads, {el32:.1f} s; the full B=32 x {seconds:.0f} s "
                          f"leg not run (estimated {est32:.0f} s > {limit:.0f} s)")
        else:
            sample.append(f"B=32 not run (estimated {est32:.0f} s > {limit:.0f} s)")
    what = ("UNMODIFIED reference SynthesizerTrn.voice_conversion + spectrogram_torch imported from /root/reference"
            if kind == "reference" else
            "oracle voice_conversion (CPU restatement of the reference in the same torch ops; /root/reference is not "
            "on this box)")
    out["sample"] = f"{what}, torch CPU fp32, weight-norm re-evaluated per call: " + "; ".join(sample)
    return out


def self_launch(n):
    """``python bench.py --gpus N`` (N > 1) started WITHOUT torch.distributed.run -- the way the driver starts the
    1-GPU line: run this same command line under ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N``
    on a free local port, one rank per GPU, instead of failing on the launch convention, and return its exit code.
    The launcher is a fresh child process (this one has already asked the HIP runtime for the device count, so it is
    not replaced in place).  The torchrun path itself (WORLD_SIZE set by the launcher) never comes here."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: --gpus {n} without a launcher; re-executing under torch.distributed.run on port {port}",
          file=sys.stderr, flush=True)
    sys.stdout.flush()
    return subprocess.call(cmd)


def distributed_environment(gpu):
    """What a post-mortem of an unattended N-GPU run needs: the collective library's version and the environment switches
    that decide whether its transports come up (the host driver of this pool only supports dmabuf IPC)."""
    env = {k: os.environ.get(k) for k in ("HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG", "NCCL_DEBUG_SUBSYS", "NCCL_SOCKET_IFNAME",
                                          "RCCL_MSCCL_ENABLE", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "MASTER_ADDR")}
    ver = None
    if gpu:
        try:
            v = torch.cuda.nccl.version()
            ver = ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
        except Exception as exc:   # noqa: BLE001
            ver = f"unavailable ({exc!r})"[:120]
    return {"rccl_version": ver, "env": env, "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}


def gather_rank_diagnostics(mine, world, group):
    """Every rank's own figures (ms of its MRF launches in the event-bracketed step, HBM bytes resident, device) on rank 0's
    line: a slow rank is attributable to a kernel group or to memory pressure.  A collective when a group exists."""
    import torch.distributed as dist
    if not group:
        return [mine]
    every = [None] * world
    dist.all_gather_object(every, mine)
    return every


def init_ranks(args, backend):
    """One process per GPU (torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*); returns
    (world, rank, local_rank, device).  ``backend`` "nccl" = RCCL on the GPUs, "gloo" = the CPU rehearsal."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gpu = backend == "nccl"
    if args.gpus > 1 or world > 1 or args.force_dist:
        assert world == args.gpus, f"launch with torch.distributed.run --nproc-per-node {args.gpus}"
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if "MASTER_ADDR" not in os.environ:        # --force-dist without torch.distributed.run: a 1-rank rendezvous
            import socket
            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                port = sock.getsockname()[1]
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        if gpu:
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group("gloo")
    dev = torch.device(f"cuda:{local_rank}") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(dev)
    return world, rank, local_rank, dev


def timed_steps(step, args, world, dev):
    """``args.warmup`` untimed steps, then EXACTLY ``args.steps`` steps bracketed by a barrier + device synchronise on
    both sides; returns (seconds = max over ranks, every rank's own seconds, last step's result).  With a process
    group (N > 1, or N = 1 under --force-dist) the barriers and the all-gather of the ranks' times are real
    collectives of the backend in use."""
    import torch.distributed as dist
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    group = dist.is_available() and dist.is_initialized()

    def barrier():
        if group:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    sync()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        result = step()
    sync()
    own = time.perf_counter() - t0      # this rank's own time to finish its steps: shows a straggler
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank = [own]
    if group:
        mine = torch.tensor([elapsed, own], dtype=torch.float64, device=dev)
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        elapsed = max(t[0].item() for t in every)
        per_rank = [t[1].item() for t in every]
    return elapsed, per_rank, result


def rank_stats(per_rank_s, steps):
    """Each rank's own ms per step (device-synchronised, before the closing barrier): min / max show a straggler."""
    ms = [round(t / steps * 1e3, 3) for t in per_rank_s]
    return {"min": min(ms), "max": max(ms), "ranks": ms}


PARITY_TOLERANCE = 1e-3      # BASELINE.json north_star: "output within 1e-3 max-abs of reference fp32"
DUMP_BUDGET_BYTES = 64 * 10**6
NOISE_SEED = 2024


def dump_outputs(outdir, arrays, budget=DUMP_BUDGET_BYTES):
    """``--dump-outputs DIR``: the arrays the timed path returned in its last step, each as DIR/<name>.npy in float32,
    so that two builds can be compared output for output.  When together they exceed ``budget`` bytes, every array is
    cut to the same fraction of its elements, chosen by a fixed seed (the same positions on every run with the same
    arguments, flattened in C order)."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    host = {name: t.detach().float().cpu().numpy() for name, t in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    budget -= 256 * len(host)                     # room for the .npy headers
    for k, (name, a) in enumerate(host.items()):
        if total > budget:
            keep = max(1, a.size * budget // total)
            idx = np.sort(np.random.default_rng(k).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(outdir, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def parity_of_item(model, sd, cfg, wave, se, tau, hop_cfg, item=0, seed=77):
    """Self-check of the measured configuration: ONE more step of the timed batch with an explicit, seeded noise
    tensor (the timed steps draw theirs on the device), and the CPU oracle -- spectrogram included -- on ``item`` of
    that batch with the same noise.  Utterances are independent at full length, so the oracle runs B = 1."""
    from openvoice_amd.mel_processing import spectrogram_torch
    from oracle import vc_oracle
    dev = wave.device
    d = hop_cfg
    spec = spectrogram_torch(wave, d.filter_length, d.sampling_rate, d.hop_length, d.win_length, center=False)
    B, _, T = spec.shape
    noise = torch.randn(B, cfg["inter_channels"], T, generator=torch.Generator().manual_seed(seed))
    lengths = torch.full((B,), T, dtype=torch.int64, device=dev)
    o_hat = model.voice_conversion(spec, lengths, se[0].to(dev), se[1].to(dev), tau=tau, noise=noise.to(dev))[0]
    got = o_hat[item, 0].cpu()
    with torch.no_grad():
        spec1 = vc_oracle.spectrogram(wave[item:item + 1].cpu())
        want = vc_oracle.voice_conversion(sd, cfg, spec1, torch.tensor([T]), se[0], se[1], tau, noise[item:item + 1],
                                          zero_g=bool(model.zero_g))[0][0, 0]
    err = float((got - want).abs().max())
    return {"max_abs_vs_oracle": err, "tolerance": PARITY_TOLERANCE, "item": item, "ok": bool(err <= PARITY_TOLERANCE),
            "oracle_peak": round(float(want.abs().max()), 4),
            "what": f"o_hat[{item}] of the timed batch (one extra step, seeded noise) vs oracle/vc_oracle.py on CPU, "
                    f"waveform -> spectrogram -> voice_conversion"}


def split_opt_in(engine, step, model, sd, cfg, wave, se, hop_cfg, B, seconds, no_parity=False, steps=3):
    """The same step with the MRF stages that have split-precision instances on ``ov_conv1d_split3`` (opt-in,
    ``ConverterEngine.use_split_bf16x3``): 1 warm-up + ``steps`` timed steps, one event-bracketed step for the split
    kernels' own rate, and the oracle self-check of the timed batch at the fp32 bar.  Reported beside the contract line,
    never as it."""
    engine.use_split_bf16x3(True)
    try:
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        engine.profile = []
        step()
        torch.cuda.synchronize()
        prof, engine.profile = engine.profile, None
        n_s = sum(1 for r in prof if r[0] == "mrf_split")
        f_s = sum(r[1] for r in prof if r[0] == "mrf_split")
        t_s = sum(r[2].elapsed_time(r[3]) for r in prof if r[0] == "mrf_split") * 1e-3
        t_l = sum(r[2].elapsed_time(r[3]) for r in prof if r[0] == "split_layout") * 1e-3
        out = {"ms_per_step": round(ms, 3), "value": round(B * seconds / (ms * 1e-3), 2),
               "unit": "x real-time (audio s / wall s)", "steps": steps,
               "dtype": "f32 (enc_q, flow, C=32 stage) + bf16x3 split-precision MRF stages (6 bf16 plane products per fp32 "
                        "product, fp32 accumulation)",
               "split_stages": [i for i, st in enumerate(engine.split_resblocks) if st is not None],
               "roofline": {"bound": "mfma", "achieved": round(6 * f_s / t_s / 1e12, 1), "peak": BF16_MFMA_PEAK_TFLOPS,
                            "unit": "TFLOP/s", "frac": round(6 * f_s / t_s / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
                            "what": "6 x the algorithmic fp32 FLOPs of the split-precision convs / their HIP-event time vs the "
                                    "dense bf16 MFMA peak", "launches_per_step": n_s,
                            "fp32_equivalent_tflops": round(f_s / t_s / 1e12, 2), "layout_kernels_ms": round(t_l * 1e3, 3)},
               "note": "opt-in (ConverterEngine.use_split_bf16x3 / bench.py --split-bf16x3); the contract line above is the "
                       "fp32 MFMA path"}
        T = int(wave.shape[1]) // int(hop_cfg.hop_length)
        rec, why = split_traffic_record(B, T, engine.split3_products)
        roof = out["roofline"]
        roof["traffic_source"] = why
        if rec and rec.get("launches_per_step") == n_s:
            # the HBM side of the same launches: PMC bytes per conversion against the 6-bytes-per-element streams
            roof.update(traffic=rec["bytes_per_step"], traffic_unit="HBM bytes per conversion over the split-precision launches",
                        alg_bytes_per_step=rec["algorithmic_bytes_per_step"],
                        traffic_over_algorithmic=rec["traffic_over_algorithmic"],
                        hbm_tb_per_s=round(rec["bytes_per_step"] / t_s / 1e12, 3),
                        hbm_frac_of_8_tb_per_s=round(rec["bytes_per_step"] / t_s / 8e12, 4))
        else:
            roof["traffic"] = None
            if rec:
                roof["traffic_source"] = (f"profiles/split3_traffic_latest.json counted {rec.get('launches_per_step')} split "
                                          f"launches per step, this run issues {n_s}")
        if not no_parity:
            par = parity_of_item(model, sd, cfg, wave, se, 0.3, hop_cfg)
            par["fp32_bar"] = 1e-4
            par["ok_at_fp32_bar"] = bool(par["max_abs_vs_oracle"] <= 1e-4)
            out["parity"] = par
        return out
    finally:
        engine.use_split_bf16x3(False)


def config_tts_v1(dev, steps=3, batch=16, tokens=100):
    """BASELINE.json configs[3] inside the driver's line: V1 base-speaker ``SynthesizerTrn.infer`` (text encoder with
    relative attention, both duration predictors, RQ-spline flows, reverse flow, generator; reference:
    openvoice/models.py:467-490), batch 16 x 100 symbols, length-aware generator work lists -- 1 warm-up + ``steps`` timed
    calls, and item 0 against oracle/tts_oracle.py on the CPU with the same recorded noise.  Never ``value``."""
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.params import synthetic_tts_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    from oracle import tts_oracle
    sd = synthetic_tts_state_dict(CFG)
    model = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator().manual_seed(0)
    B, Tx = batch, tokens
    tok = torch.randint(0, 68, (B, Tx), generator=gen).to(dev)
    lengths = torch.full((B,), Tx, dtype=torch.long, device=dev)
    sid = (torch.arange(B) % 10).to(dev)
    noise_w = torch.randn(B, 2, Tx, generator=gen).to(dev)
    noise_z = torch.randn(B, 192, 16 * Tx, generator=gen).to(dev)

    def call():
        return model.infer(tok, lengths, sid=sid, noise_scale=0.667, noise_scale_w=0.6, length_scale=1.0,
                           noise_w=noise_w, noise_z=noise_z, skip_padding=True)

    o, _, y_mask, _ = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        o, _, y_mask, _ = call()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    per_utt = y_mask[:, 0].sum(1)
    Ty = int(y_mask.shape[2])
    audio_s = float(per_utt.sum()) * 256 / SAMPLE_RATE
    gen_frames = float(torch.clamp(per_utt + 16, max=Ty).sum())
    flops = 614.8e6 * gen_frames + 4 * 3.54e6 * B * Ty + (4.4e9 + 0.33e9 + 0.21e9) * B * Tx / 100.0
    a = lambda t: t[:1].cpu()
    with torch.no_grad():
        o_c = tts_oracle.infer(sd, CFG, a(tok), a(lengths), a(sid), a(noise_w), a(noise_z), 0.667, 1.0, 0.6)[0]
    n0 = 256 * int(per_utt[0])
    # the generator is unmasked: in a padded batch the last ~13 frames of an item see its neighbours' padding, so the
    # comparison with the B = 1 oracle stops 20 frames before the item's end
    err = float((o[0, 0, :n0 - 5120].cpu() - o_c[0, 0, :n0 - 5120]).abs().max())
    return {"workload": f"BASELINE.json configs[3]: V1 BaseSpeakerTTS SynthesizerTrn.infer, batch {B} x {Tx} symbols, fp32, "
                        f"calibrated random weights, length-aware generator work lists",
            "ms_per_batch": round(dt * 1e3, 3), "steps": steps, "utterances_per_s": round(B / dt, 2),
            "audio_s_per_batch": round(audio_s, 2), "value": round(audio_s / dt, 1), "unit": "x real-time (audio s / wall s)",
            "frames_per_utterance": round(float(per_utt.float().mean()), 1), "padded_frames": Ty,
            "roofline": {"bound": "mfma", "achieved": round(flops / dt / 1e12, 2), "peak": FP32_MFMA_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(flops / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                         "alg_tflop_per_batch": round(flops / 1e12, 3),
                         "what": "ALGORITHMIC conv FLOPs of the frames actually computed / wall time of the whole infer() incl. "
                                 "its host sync and the token-rate kernels (the Winograd-domain launches execute fewer)"},
            "parity": {"max_abs_vs_oracle": err, "tolerance": PARITY_TOLERANCE, "ok": bool(err <= PARITY_TOLERANCE), "item": 0,
                       "what": "o[0] vs oracle/tts_oracle.py (B = 1, same recorded noise), excluding the last 20 frames"}}


def config_bf16_decoder(dev, steps=3, batch=64, frames=861):
    """BASELINE.json configs[4] inside the driver's line: the HiFi-GAN generator with bf16 activations (reference:
    openvoice/models.py:272-291), batch 64 x 861 frames -- 1 warm-up + ``steps`` timed passes; both roofs from the
    digest-gated counter record (profiles/bf16_counters_latest.json) where it belongs to these sources, else the algorithmic
    bytes; item 0 against the fp32 oracle generator on the CPU.  Never ``value``."""
    from openvoice_amd.bf16 import GeneratorBf16, generator_alg_bytes
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    from oracle import vc_oracle
    sd = synthetic_state_dict(CFG, 513, seed=1234)
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(batch, 192, frames, generator=gen).to(dev)
    g = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev)
    dec = GeneratorBf16(sd, CFG, dev)
    o = dec.decode(z, g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        o = dec.decode(z, g)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    gen_bytes = generator_alg_bytes(CFG, batch, frames)
    gen_flops = 529.44e9 * batch * frames / 861.0
    rec, rec_note = bf16_counter_record(batch, frames)
    traffic_b = rec["traffic_GB_per_pass"] * 1e9 if rec else None
    with torch.no_grad():
        want = vc_oracle.generator(sd, z[:1].cpu(), g.cpu(), CFG)[0, 0]
    diff = o[0, 0].cpu() - want
    return {"workload": f"BASELINE.json configs[4]: HiFi-GAN generator, bf16 activations / fp32 accumulation, batch {batch} x "
                        f"{frames} frames (10 s), calibrated random weights",
            "ms_per_batch": round(dt * 1e3, 3), "steps": steps, "utterances_per_s": round(batch / dt, 1),
            "value": round(batch * frames * 256 / SAMPLE_RATE / dt, 1), "unit": "x real-time (audio s / wall s)",
            "roofline": {"bound": "hbm", "achieved": round((traffic_b or gen_bytes) / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                         "frac": round((traffic_b or gen_bytes) / dt / 8e12, 4),
                         "frac_of_achievable_6300": round((traffic_b or gen_bytes) / dt / 6.3e12, 4),
                         "traffic": traffic_b, "traffic_source": rec_note, "alg_bytes": round(gen_bytes),
                         "mfma": {"achieved_tflops": round(gen_flops / dt / 1e12, 1), "peak_tflops": BF16_MFMA_PEAK_TFLOPS,
                                  "frac": round(gen_flops / dt / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
                                  "mfma_busy": rec.get("mfma_busy") if rec else None,
                                  "shader_clock_ghz": rec.get("shader_clock_ghz") if rec else None}},
            "parity": {"max_abs_vs_fp32_oracle": round(float(diff.abs().max()), 5),
                       "rel_rms_vs_fp32_oracle": round(float(diff.pow(2).mean().sqrt() / want.pow(2).mean().sqrt()), 5),
                       "tolerance": {"max_abs": 3e-2, "rel_rms": 1.5e-2}, "item": 0,
                       "ok": bool(diff.abs().max() <= 3e-2),
                       "what": "o[0] vs oracle/vc_oracle.generator (fp32, CPU) on the same z: bf16 storage rounding, stated "
                               "tolerance of tests/test_gpu_bf16.py"}}


def dry_run(args):
    """bench.py's multi-rank control flow on CPU + gloo (see --dry-run)."""
    import torch.distributed as dist
    from openvoice_amd.parallel import broadcast_speaker_embeddings
    world, rank, _, dev = init_ranks(args, "gloo")
    gen = torch.Generator().manual_seed(1)
    se = (0.1 * torch.randn(1, 256, 1, generator=gen), 0.1 * torch.randn(1, 256, 1, generator=gen))
    B = args.batch
    wave = torch.full((B, 64), float(rank))

    def step():
        src_se, tgt_se = broadcast_speaker_embeddings(se[0] if rank == 0 else None, se[1] if rank == 0 else None,
                                                      256, dev)      # a collective whenever a group exists
        return wave * (src_se.sum() - tgt_se.sum()), 1      # stand-in for the conversion

    elapsed, per_rank, (o, _) = timed_steps(step, args, world, dev)
    ok = bool(torch.allclose(o, wave * (se[0].sum() - se[1].sum())))   # every rank saw rank 0's embeddings
    if dist.is_initialized():
        flag = torch.tensor([1.0 if ok else 0.0])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item() == 1.0)
    names = [f"cpu (rank {rank})"]
    dist_on = dist.is_initialized()
    if dist_on:
        names = [None] * world
        dist.all_gather_object(names, f"cpu (rank {rank})")
    # the per-rank diagnostics of the measured --full run, with stand-in figures (same collective, same shape)
    diag = None
    if args.full:
        diag = gather_rank_diagnostics({"rank": rank, "mrf_ms": float(rank), "hbm_resident_bytes": 0,
                                        "device": f"cpu (rank {rank})"}, world, dist_on)
    line = None
    if rank == 0:
        line = {"metric": "real_time_factor", "value": None, "unit": "x real-time (audio s / wall s)",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                "per_rank_ms_per_step": rank_stats(per_rank, args.steps), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "dry_run": True, "broadcast_consistent": ok,
                "distributed": dict({"process_group": dist_on, "backend": dist.get_backend() if dist_on else None,
                                     "rccl_ranks": 0, "devices": names}, **distributed_environment(False)),
                "config": {"workload": "control-flow rehearsal on CPU + gloo, no conversion",
                           "batch_per_gpu": B, "global_batch": B * world}}
        if args.full:
            line["distributed"]["per_rank"] = diag
            # the shape of the measured line's roofline object; no kernel ran, so no figures
            line["roofline"] = {"bound": "mfma", "achieved": None, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": None, "traffic": None}
    if dist_on:
        dist.destroy_process_group()
    if rank == 0:
        # rank 0's CPU-baseline leg exactly where the measured run has it -- after the group is gone -- on a
        # 0.25 s utterance so that the rehearsal stays a rehearsal
        if args.full and not args.no_cpu_baseline:
            from openvoice_amd.params import synthetic_state_dict
            from openvoice_amd.utils import default_converter_hparams
            hps = default_converter_hparams("v2")
            cfg = dict(hps.model.items())
            sd = synthetic_state_dict(cfg, hps.data.filter_length // 2 + 1, seed=1234)
            line["cpu_baseline"] = dict(cpu_baseline(sd, cfg, 0.25, budget_s=0.5, want_reference=False), dry_run=True)
        print(json.dumps(line), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="utterances per GPU")
    ap.add_argument("--seconds", type=float, default=10.0, help="utterance length")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure (off by default: a plain run sets up, warms up, times "
                         "--steps steps and prints the line): the MFMA roofline and per-kernel-group times of one extra "
                         "event-bracketed step, the PCIe-inclusive rate, the opt-in split-precision line, BASELINE.json "
                         "configs[3] / [4], the oracle self-check and the CPU baseline; the --no-* options below thin it")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one returned (o_hat, y_mask, z, z_p, z_hat) as "
                         "DIR/<name>.npy in float32, at most 64 MB in all (a fixed, seeded sample beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=20.0,
                    help="seconds of CPU baseline sampling at B = 1 on all threads (plus one 1-thread utterance)")
    ap.add_argument("--cpu-batch32", action="store_true", default=None,
                    help="time ONE B = 32 conversion of the whole batch on the CPU even when the timed B = 4 run estimates it "
                         "above 60 s (default: run it when the estimate is <= 60 s)")
    ap.add_argument("--no-cpu-batch32", dest="cpu_batch32", action="store_false",
                    help="never run the B = 32 CPU leg (a short-utterance stand-in is timed instead)")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle self-check of the timed batch")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (backend nccl = RCCL) and issue the per-step speaker-embedding "
                         "broadcast, the barriers and the all-gather of the ranks' times even at --gpus 1, so the "
                         "multi-GPU code path runs on a one-GPU box (tests/test_gpu_dist.py)")
    ap.add_argument("--bf16-generator", action="store_true",
                    help="NOT the contract configuration: run the generator on the opt-in bf16 kernels "
                         "(BASELINE.json configs[4]); the JSON line is marked accordingly")
    ap.add_argument("--split-bf16x3", action="store_true",
                    help="NOT the contract configuration: run the MRF stages with split-precision instances on "
                         "ov_conv1d_split3 (three bf16 planes per fp32 operand, six plane products, fp32 accumulation: "
                         "fp32-level results on the bf16 matrix pipe); the JSON line is marked accordingly and its "
                         "roofline is stated against the 2.5 PFLOP/s bf16 peak on products x the algorithmic FLOPs")
    ap.add_argument("--split-products", type=int, default=6, choices=(6, 3),
                    help="plane products per fp32 product with --split-bf16x3: 6 (fp32 level) or 3 (16-bit operands)")
    ap.add_argument("--no-opt-in", action="store_true",
                    help="skip the short measurements the --full line carries beside the contract figures: 'opt_in_split_bf16x3', "
                         "'config_tts_v1' (BASELINE.json configs[3]) and 'config_bf16_decoder' (configs[4])")
    ap.add_argument("--pmc-calibration", action="store_true",
                    help="after the timed region, run three 1 GiB device-to-device copies (a known byte count) "
                         "so a rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE pass can be calibrated")
    ap.add_argument("--dry-run", action="store_true",
                    help="control-flow rehearsal without a GPU (tests/test_bench_dry_run.py): gloo instead of RCCL, CPU "
                         "tensors, the conversion replaced by a stand-in; everything else -- rendezvous, the per-step "
                         "speaker-embedding broadcast, barriers, max-over-ranks timing, one JSON line on rank 0 -- is "
                         "the code the N-GPU run executes.  The line is marked dry_run and carries no measurement")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and not args.dry_run:
        # the first N-GPU run happens with nobody watching: a box with fewer devices than ranks says so in ONE JSON line
        # and a non-zero exit code, before any launcher or rendezvous is started
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            if int(os.environ.get("RANK", "0")) == 0:
                print(json.dumps({"metric": "real_time_factor", "value": None, "n_gpus": args.gpus,
                                  "error": f"--gpus {args.gpus} but torch.cuda.device_count() = {have} on this node",
                                  "visible_devices": {k: os.environ.get(k) for k in
                                                      ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}}),
                      flush=True)
            return 4
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)
    if args.dry_run:
        return dry_run(args)

    import torch.distributed as dist
    from openvoice_amd.mel_processing import spectrogram_torch
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.parallel import broadcast_speaker_embeddings
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import default_converter_hparams

    world, rank, local_rank, dev = init_ranks(args, "nccl")

    hps = default_converter_hparams("v2")
    cfg = dict(hps.model.items())
    sd = synthetic_state_dict(cfg, hps.data.filter_length // 2 + 1, seed=1234)
    model = SynthesizerTrn(0, hps.data.filter_length // 2 + 1, n_speakers=0, **cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    engine = model.engine()
    if args.bf16_generator:
        engine.use_bf16_generator(True)
    if args.split_bf16x3:
        engine.use_split_bf16x3(True, products=args.split_products)

    B = args.batch
    samples = int(args.seconds * SAMPLE_RATE)
    wave = synth_wave(B, samples, 1000 + rank, dev)           # resident in HBM before timing starts
    gen = torch.Generator().manual_seed(1)
    se = (0.1 * torch.randn(1, 256, 1, generator=gen), 0.1 * torch.randn(1, 256, 1, generator=gen))
    d = hps.data
    n_frames = (samples + 2 * ((d.filter_length - d.hop_length) // 2) - d.filter_length) // d.hop_length + 1
    lengths = torch.full((B,), n_frames, dtype=torch.int64, device=dev)      # resident, like the waveforms

    def step():
        # a real RCCL broadcast whenever a process group exists (N > 1, or N = 1 under --force-dist); else a copy
        src_se, tgt_se = broadcast_speaker_embeddings(se[0] if rank == 0 else None, se[1] if rank == 0 else None,
                                                      256, dev)
        spec = spectrogram_torch(wave, d.filter_length, d.sampling_rate, d.hop_length, d.win_length, center=False)
        assert spec.shape[2] == n_frames
        o_hat, y_mask, (z, z_p, z_hat) = model.voice_conversion(spec, lengths, src_se, tgt_se, tau=0.3)
        return o_hat, spec.shape[2], (y_mask, z, z_p, z_hat)

    # every step draws its noise from torch's generator on the device: seeded here, outside the timed region, so that
    # the same arguments give the same outputs from run to run (--dump-outputs)
    torch.cuda.manual_seed(NOISE_SEED)
    elapsed, per_rank, (o_hat, frames, rest) = timed_steps(step, args, world, dev)
    if args.dump_outputs and rank == 0:
        # before any other step: the engine reuses its buffers
        dump_outputs(args.dump_outputs, dict(zip(("o_hat", "y_mask", "z", "z_p", "z_hat"), (o_hat,) + rest)))
    dist_on = dist.is_available() and dist.is_initialized()
    devices = [torch.cuda.get_device_name(dev)]
    if dist_on:                      # every rank's device, gathered over the process group (a collective: all ranks)
        devices = [None] * world
        dist.all_gather_object(devices, torch.cuda.get_device_name(dev))
    assert o_hat.shape == (B, 1, frames * engine.total_upsample) and bool(torch.isfinite(o_hat).all())

    # ---- --full only from here to the line: what the headline figure does not need ----
    if args.full:
        # PCIe-inclusive rate, reported beside `value` (never as it): the same step with the waveforms coming from
        # pinned host memory and the converted audio returned to pinned host memory, as a caller holding host buffers
        # sees it.  Two steps, after the timed region; any failure here leaves the contract line untouched.
        pcie = None
        try:
            if world > 1:       # N = 1 only: a one-sided failure here must never strand the other ranks in a collective
                raise RuntimeError("measured at --gpus 1 only")
            host_in = wave.cpu().pin_memory()
            host_out = torch.empty(o_hat.shape, dtype=o_hat.dtype).pin_memory()
            dev_wave = wave

            def pcie_step():
                dev_wave.copy_(host_in, non_blocking=True)
                o = step()[0]
                host_out.copy_(o, non_blocking=True)

            pcie_step()
            torch.cuda.synchronize()
            tp = time.perf_counter()
            for _ in range(2):
                pcie_step()
            torch.cuda.synchronize()
            pcie_ms = (time.perf_counter() - tp) / 2 * 1e3
            pcie = {"ms_per_step": round(pcie_ms, 3), "value": round(B * args.seconds / (pcie_ms * 1e-3), 2),
                    "host_bytes_per_step": int(host_in.numel() * 4 + host_out.numel() * 4),
                    "note": "per rank; pinned host -> HBM -> convert -> pinned host, copies on the compute stream"}
        except Exception as exc:   # noqa: BLE001 -- diagnostics only
            pcie = {"error": repr(exc)[:200]}

        # ---- roofline of the dominant kernel: the MFMA conv family on the 72 MRF (ResBlock) convs ----
        engine.profile = []
        step()
        torch.cuda.synchronize()
        prof, engine.profile = engine.profile, None
        by_tag = {}
        wino_n, wino_alg, wino_s = 0, 0.0, 0.0
        for r in prof:
            tag, flops, e0, e1 = r[:4]
            rec = by_tag.setdefault(tag, [0, 0.0, 0.0, 0.0])
            dt = e0.elapsed_time(e1) * 1e-3
            rec[0] += 1
            rec[1] += flops
            rec[2] += dt
            rec[3] += r[4] if len(r) > 4 else flops      # FLOPs the kernels EXECUTE (Winograd-domain launches: fewer)
            if len(r) > 4:
                wino_n, wino_alg, wino_s = wino_n + 1, wino_alg + flops, wino_s + dt
        if args.bf16_generator:
            from openvoice_amd.bf16 import generator_alg_bytes
            n_mrf, f_mrf, t_mrf, x_mrf = by_tag["gen_bf16"][0], 0.0, by_tag["gen_bf16"][2], 0.0
            gen_bytes = generator_alg_bytes(cfg, B, frames)
        else:
            n_mrf, f_mrf, t_mrf, x_mrf = by_tag["mrf"]
        # priced on the FLOPs the matrix pipe executes: the Winograd-domain launches execute 6 / 16 / 23 of the 12 / 28 / 44 products of their
        # algorithmic FLOPs, so the fraction of the fp32 MFMA peak stays a utilisation (<= 1); what the same time would
        # mean for the direct form is `algorithmic_equivalent_tflops`
        achieved = x_mrf / t_mrf / 1e12
        alg_equiv = f_mrf / t_mrf / 1e12
        from openvoice_amd.engine import PAIR_POLICY
        fused_set = PAIR_POLICY if engine.fuse_pairs else ()
        traffic, traffic_note = pmc_traffic(B, frames, engine.fuse_pairs, PAIR_POLICY, n_mrf, engine.chain_streams)
        alg_bytes = mrf_alg_bytes_per_launch(cfg, B, frames, fused_set)
        all_flops = sum(r[1] for r in by_tag.values())
        all_conv_s = sum(r[2] for r in by_tag.values())
        # every rank's own figures on rank 0's line (a collective when a group exists: all ranks come through here)
        rank_diag = gather_rank_diagnostics(
            {"rank": rank, "device": torch.cuda.get_device_name(dev), "mrf_ms": round(t_mrf * 1e3, 3),
             "by_kernel_group_ms": {k: round(v[2] * 1e3, 3) for k, v in sorted(by_tag.items())},
             "hbm_resident_bytes": int(torch.cuda.memory_allocated(dev)), "hbm_reserved_bytes": int(torch.cuda.memory_reserved(dev)),
             "hbm_total_bytes": int(torch.cuda.get_device_properties(dev).total_memory)}, world, dist_on)

    # ---- opt-in split-precision MRF (never `value`): 3 timed steps + the oracle self-check, after the contract region ----
    opt_in = None
    if args.full and rank == 0 and world == 1 and not (args.split_bf16x3 or args.bf16_generator or args.no_opt_in):
        try:
            opt_in = split_opt_in(engine, step, model, sd, cfg, wave, se, d, B, args.seconds, no_parity=args.no_parity)
        except Exception as exc:   # noqa: BLE001 -- diagnostics only; the contract line stands on its own
            opt_in = {"error": repr(exc)[:300]}
            engine.use_split_bf16x3(False)

    # ---- BASELINE.json configs[3] and configs[4], bounded, after the contract region (never inside it, never `value`) ----
    extra_cfgs = {}
    if args.full and rank == 0 and world == 1 and not (args.split_bf16x3 or args.bf16_generator or args.no_opt_in):
        for key, fn in (("config_tts_v1", config_tts_v1), ("config_bf16_decoder", config_bf16_decoder)):
            t_cfg = time.perf_counter()
            try:
                extra_cfgs[key] = fn(dev)
            except Exception as exc:   # noqa: BLE001 -- diagnostics only; the contract line stands on its own
                extra_cfgs[key] = {"error": repr(exc)[:300]}
            extra_cfgs[key]["wall_s_incl_setup"] = round(time.perf_counter() - t_cfg, 2)

    if args.pmc_calibration:
        src = torch.zeros(1 << 28, dtype=torch.float32, device=dev)   # 1 GiB
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        del src, dst

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        utt_s = world * B * args.steps / elapsed
        out = {
            "metric": "real_time_factor",
            "value": round(utt_s * args.seconds, 2),
            "unit": "x real-time (audio s / wall s)",
            "utterances_per_s": round(utt_s, 3),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
            "per_rank_ms_per_step": rank_stats(per_rank, args.steps),
            "distributed": dict({"process_group": dist_on, "backend": dist.get_backend() if dist_on else None,
                                 "rccl_ranks": world if dist_on else 0, "devices": devices,
                                 "collectives_per_step": "1 broadcast of [2,256] fp32 (src/tgt se)" if dist_on else "none",
                                 "binding": __import__("openvoice_amd._lib", fromlist=["binding"]).binding()},
                                **distributed_environment(True)),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (enc_q, flow) + bf16 generator, fp32 accumulation" if args.bf16_generator else "f32",
            "data": "synthetic",
            "config": {"workload": f"ToneColorConverter.convert path, {B} x {args.seconds:g} s @ 22.05 kHz per GPU "
                                   f"(T={frames} frames), fp32, calibrated random weights",
                       "batch_per_gpu": B, "global_batch": B * world, "utterance_s": args.seconds,
                       "parallelism": f"dp{world} (utterance sharding, RCCL broadcast of src/tgt se)"},
            "per_batch_latency_rtf": round(args.seconds / (ms * 1e-3), 2),
        }
        if args.full:
            out["distributed"]["per_rank"] = rank_diag
            out.update({
                "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": FP32_MFMA_PEAK_TFLOPS,
                             "unit": "TFLOP/s", "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                             "traffic_unit": "HBM bytes per MRF launch (rocprofv3 PMC, profiles/pmc_traffic_latest.json)",
                             "traffic_source": traffic_note,
                             "alg_bytes_per_launch": round(alg_bytes),
                             "achieved_is": "EXECUTED matrix FLOPs of the MRF launches / their HIP-event time",
                             "algorithmic_equivalent_tflops": round(alg_equiv, 2),
                             "executed_over_algorithmic_flops": round(x_mrf / f_mrf, 4) if f_mrf else None,
                             "winograd": {"launches_per_step": wino_n,
                                          "share_of_mrf_alg_flops": round(wino_alg / f_mrf, 4) if f_mrf else None,
                                          "ms_per_step": round(wino_s * 1e3, 3),
                                          "which": "ResBlock convs with C >= 64 (k = 3 / 7 / 11, dilations 1 / 3 / 5) and the dilation-1 "
                                                   "k = 11 convs at C = 32 (ov_conv1d_wino_f32: nested F(4,3), fp32 MFMA; "
                                                   "engine.wino_policy); every other conv runs the direct implicit GEMM"}
                             if wino_n else None,
                             "kernel": "ovkw::conv1d_wino_kernel (Winograd-domain, where it has an instance) + ovk::conv1d_mfma_kernel "
                                       "(+ ovk::respair_mfma_kernel where a ResBlock pair is one launch) on the MRF ResBlock convs",
                             "fused_pairs": sorted(f"C={c} k={k}" for c, k in fused_set),
                             "launches_per_step": n_mrf, "avg_launch_ms": round(t_mrf / n_mrf * 1e3, 4),
                             "alg_gflop_per_launch": round(f_mrf / n_mrf / 1e9, 2),
                             "all_conv_alg_tflop_per_step": round(all_flops / 1e12, 3),
                             "all_conv_ms_per_step": round(all_conv_s * 1e3, 2),
                             "whole_step_tflops": round(all_flops / (ms * 1e-3) / 1e12, 2)},
                "by_kernel_group_ms": {k: round(v[2] * 1e3, 3) for k, v in sorted(by_tag.items())},
                "pcie_inclusive": pcie,
            })
        if opt_in is not None:
            out["opt_in_split_bf16x3"] = opt_in
        out.update(extra_cfgs)
        if args.split_bf16x3:
            out["dtype"] = (f"f32 (enc_q, flow, C=32 stage) + bf16x3 split-precision MRF stages ({args.split_products} bf16 plane "
                            f"products per fp32 product, fp32 accumulation)")
            out["note"] = "opt-in configuration (--split-bf16x3), not the contract line"
        if args.bf16_generator:
            out["note"] = "opt-in configuration (--bf16-generator), not the contract line"
        if args.full and args.split_bf16x3:
            n_s, f_s, t_s = by_tag["mrf_split"][:3]
            pf = args.split_products * f_s / t_s / 1e15
            out["roofline"] = {"bound": "mfma", "achieved": round(pf * 1e3, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(pf * 1e3 / BF16_MFMA_PEAK_TFLOPS, 4), "traffic": None,
                               "kernel": "ovks3::conv1d_split3_kernel (v_mfma_f32_16x16x32_bf16) on the MRF convs of the "
                                         "stages with split-precision instances",
                               "what": f"{args.split_products} x the algorithmic fp32 FLOPs of those convs (every fp32 product = "
                                       f"{args.split_products} bf16 plane products) / their HIP-event time, against the dense "
                                       f"bf16 MFMA peak -- NOT against the 157.3 TFLOP/s fp32 peak",
                               "launches_per_step": n_s, "avg_launch_ms": round(t_s / n_s * 1e3, 4),
                               "fp32_equivalent_tflops": round(f_s / t_s / 1e12, 2),
                               "alg_tflop_per_step_split_stages": round(f_s / 1e12, 3),
                               "fp32_stage_launches": n_mrf, "fp32_stage_tflops": round(achieved, 2),
                               "layout_kernels_ms": round(by_tag.get("split_layout", [0, 0, 0.0])[2] * 1e3, 3)}
            rec, why = split_traffic_record(B, frames, args.split_products)
            out["roofline"]["traffic_source"] = why
            if rec and rec.get("launches_per_step") == n_s:
                out["roofline"].update(
                    traffic=rec["bytes_per_step"], traffic_unit="HBM bytes per conversion over the split-precision launches",
                    alg_bytes_per_step=rec["algorithmic_bytes_per_step"],
                    traffic_over_algorithmic=rec["traffic_over_algorithmic"],
                    hbm_tb_per_s=round(rec["bytes_per_step"] / t_s / 1e12, 3),
                    hbm_frac_of_8_tb_per_s=round(rec["bytes_per_step"] / t_s / 8e12, 4))
        if args.full and args.bf16_generator:
            # this configuration is judged against BOTH roofs -- HBM bytes (PMC-measured where a
            # counter record of THESE kernel sources at this shape is committed, algorithmic otherwise) / 6.3 and 8.0
            # TB/s, and the generator's FLOPs / the dense bf16 MFMA peak
            gen_flops = 529.44e9 * B * frames / 861.0
            rec, rec_note = bf16_counter_record(B, frames)
            traffic_b = rec["traffic_GB_per_pass"] * 1e9 if rec else None
            out["roofline"] = {"bound": "hbm", "achieved": round((traffic_b or gen_bytes) / t_mrf / 1e9, 1), "peak": 8000.0,
                               "unit": "GB/s", "frac": round((traffic_b or gen_bytes) / t_mrf / 8e12, 4),
                               "frac_of_achievable_6300": round((traffic_b or gen_bytes) / t_mrf / 6.3e12, 4),
                               "traffic": traffic_b, "traffic_source": rec_note,
                               "alg_bytes": round(gen_bytes), "alg_GBps": round(gen_bytes / t_mrf / 1e9, 1),
                               "mfma": {"achieved_tflops": round(gen_flops / t_mrf / 1e12, 1), "peak_tflops": BF16_MFMA_PEAK_TFLOPS,
                                        "frac": round(gen_flops / t_mrf / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
                                        "mfma_busy": rec.get("mfma_busy") if rec else None,
                                        "shader_clock_ghz": rec.get("shader_clock_ghz") if rec else None},
                               "kernel": "ovk16q::respair2_bf16_kernel + ovk16::conv1d_bf16cl_kernel (whole bf16 generator)",
                               "generator_ms": round(t_mrf * 1e3, 3)}
        rc = 0
        if args.full and not args.no_parity and not args.bf16_generator:   # (--split-bf16x3: the split path vs the oracle)
            try:
                out["parity"] = parity_of_item(model, sd, cfg, wave, se, 0.3, d)
                rc = 0 if out["parity"]["ok"] else 3
            except Exception as exc:   # noqa: BLE001 -- an unverifiable line must not look verified
                out["parity"] = {"error": repr(exc)[:300], "ok": False, "tolerance": PARITY_TOLERANCE}
                rc = 3
    else:
        rc, out = 0, None
    # The process group is torn down BEFORE the CPU baseline: the other ranks are done and exit, nobody waits in a
    # collective while rank 0 spends ~20 s on the host cores.  The line is printed last, complete, once.
    if dist_on:
        dist.destroy_process_group()
    if rank == 0:
        if args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(sd, cfg, args.seconds, args.cpu_budget, batch32=args.cpu_batch32)
        print(json.dumps(out), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
