#!/usr/bin/env python3
"""Benchmark of the whisper-burn hot path on MI355X: real-time factor of
waveform -> token ids (mel frontend + encoder + KV-cached decode + stitch).

    python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)
    python bench.py --gpus N --steps K --warmup W --full             (+ every extra leg, check and roofline)
    python bench.py --gpus N --steps K --warmup W --dump-outputs DIR (+ the last timed step's outputs as .npy)

A plain run sets up, warms up, times the K steps and prints the headline line.  Everything else the
script measures or checks -- the host-PCM leg, the profiled per-kernel / per-stage passes and the
roofline figures built on them, the frontend-alone leg, the CPU baseline, the beam-5 and large-v2
legs, the token comparison with the committed oracle rows -- runs only with `--full`.

One "step" = one pass of the hot path over one batch of synthetic input: `--seconds` (30) seconds
of seeded synthetic 16 kHz audio PER GPU, cut into the reference's windows (14.9 s, 3 s overlap,
/root/reference/src/transcribe.rs:32-34, :120-123), mel + encoder once per window, greedy
(beam_size = 1 = the live beam search of transcribe.rs:232 with k = 1) up to max_depth = 100
tokens, token rows all-gathered over RCCL (N > 1) and stitched on the host.  Inputs (PCM,
weights) are resident in HBM when the timed region starts.  Metric: real-time factor =
audio seconds processed by the whole job / wall seconds (BASELINE.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "whisper-burn_amd")]

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFLOPS = {"f32": 157.3,                    # dense peak of the exact-f32 MFMA, same guide
                    "f16x3": 2500.0 / 3.0}           # split precision: three fp16 MFMAs (2.5 PF dense) per f32-grade product


def e2e_roofline_ms(dims, lens, n_steps, dtype, clip=1490, gen_lens=None, prompt_steps=3, encoder_peak=None):
    """Roofline time of one bench step from the algorithmic work of every stage: mel = 960 B
    per frame over HBM, encoder + cross-K/V projection = dense FLOPs over the MFMA peak of the path's dtype,
    decode = weights + cached cross-K/V streamed once per step over HBM.  `gen_lens` (tokens each window generated):
    only the NECESSARY bytes are counted -- a window's cached K/V for the steps in which it is still live, and no step
    after the last window has ended (the engine marks finished rows dead and stops)."""
    d, L, V = dims["n_text_state"], dims["n_text_layer"], dims["n_vocab"]
    s = 4.0
    frames = [int(n) // 160 for n in lens]
    T = [min(f, clip) + 10 for f in frames]
    C = [(t - 1) // 2 + 1 for t in T]
    mel_ms = 960.0 * sum(frames) / (HBM_PEAK_GBS * 1e9) * 1e3
    enc_flops = sum(2 * 80 * d * 3 * t + 2 * d * d * 3 * c + L * (8 * c * d * d + 4 * c * c * d + 16 * c * d * d)
                    for t, c in zip(T, C))
    ckv_flops = sum(L * 4 * c * d * d for c in C)
    enc_ms = (enc_flops + ckv_flops) / (MFMA_PEAK_TFLOPS[encoder_peak or dtype] * 1e12) * 1e3
    w_bytes = s * (V * d + L * 14 * d * d)                                    # decoder weights + E^T, once per step
    if gen_lens is None:
        dec_bytes = n_steps * (w_bytes + 4.0 * L * 2 * d * sum(C))           # cached K/V stay f32
    else:
        live_steps = [prompt_steps + int(g) for g in gen_lens]               # prompt prefill + one step per token
        dec_bytes = max(live_steps, default=0) * w_bytes + sum(4.0 * L * 2 * d * c * n for c, n in zip(C, live_steps))
    dec_ms = dec_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
    return {"mel": mel_ms, "encoder_and_cross_kv": enc_ms, "decode": dec_ms, "total": mel_ms + enc_ms + dec_ms,
            "_work": {"encoder_flops": float(enc_flops + ckv_flops), "decode_bytes": float(dec_bytes)}}


CPU_BASELINE_DEPTH = 32     # decode depth of the CPU leg's REPEATED sample (second field); `value` is one run at the GPU's depth


def run_cpu_baseline(weights, st, audio, sr, wlen, beam, depth, geometry, model_name, reps=3, full_depth=True):
    """The `cpu_baseline` leg: the oracle (kind "port": the PyTorch-CPU fp32 restatement of the reference algorithm as
    written -- dense-DFT mel, no KV cache, full-prefix decoder re-run per step) on a BOUNDED sample of the workload: ONE
    window on the host cores PyTorch uses.

    `value` is LIKE-FOR-LIKE with the GPU figure: one timed run at the GPU run's own decode depth (the reference re-runs
    the whole prefix per token, transcribe.rs:253-307, so its cost per token grows with the depth and a shallower sample
    would flatter it).  `depth32` keeps the cheaper repeated sample of the earlier rounds (one
    warm-up, `reps` runs, median; every run listed) with the mel / encoder stages timed on their own.
    Runs without a GPU (tests call it on a micro model)."""
    import statistics

    import torch
    from oracle import mel as omel
    from oracle import transcribe as otr
    from oracle.model import OracleWhisper
    ow = OracleWhisper(weights, frame_limit_x2=geometry == "whisper30")
    ost = otr.SpecialTokens(st.start_of_transcript, st.language, st.transcribe, st.no_timestamps,
                            st.end_of_text, st.is_special.astype(bool))
    n_cpu = min(len(audio), int(wlen))                               # bounded sample: ONE window
    clip = audio[:n_cpu]
    cpu_depth = min(int(depth), CPU_BASELINE_DEPTH)
    otr.waveform_to_tokens(ow, ost, clip, sr, beam, min(cpu_depth, 4))   # warm-up: thread pool, allocator, code paths
    runs = []
    for _ in range(max(1, reps)):
        t0 = time.perf_counter()
        otr.waveform_to_tokens(ow, ost, clip, sr, beam, cpu_depth)        # the whole path, as it comes
        runs.append(time.perf_counter() - t0)
    cpu_dt = statistics.median(runs)
    full_dt = cpu_dt
    if full_depth and cpu_depth != int(depth):
        t0 = time.perf_counter()
        otr.waveform_to_tokens(ow, ost, clip, sr, beam, int(depth))       # ONE run at the GPU run's depth: the like-for-like figure
        full_dt = time.perf_counter() - t0
    t_mels, t_encs = [], []
    for _ in range(max(1, reps)):                                        # ... then the two front stages on their own
        t0 = time.perf_counter()
        mel = omel.prep_audio(torch.from_numpy(np.ascontiguousarray(clip))[None], float(sr))
        t_mels.append(time.perf_counter() - t0)
        keep = min(mel.shape[2], ow.encoder_ctx_size() - 10)
        melp = torch.cat([mel[:, :, :keep], torch.zeros(1, mel.shape[1], 10)], 2)
        t0 = time.perf_counter()
        ow.forward_encoder(melp)
        t_encs.append(time.perf_counter() - t0)
    t_mel, t_enc = statistics.median(t_mels), statistics.median(t_encs)
    t_mel, t_enc = min(t_mel, cpu_dt), min(t_enc, max(cpu_dt - min(t_mel, cpu_dt), 0.0))
    like = full_depth or cpu_depth == int(depth)
    return {"value": round((n_cpu / sr) / full_dt, 3), "unit": "x real-time", "cores": torch.get_num_threads(),
            "kind": "port",
            "sample": f"1 window ({n_cpu / sr:.1f} s, {geometry} geometry), {model_name}, beam {beam}, "
                      f"depth {int(depth) if like else cpu_depth}" + ("" if like else f" (GPU run: {depth})") +
                      f", PyTorch-CPU fp32 restatement of the reference algorithm as "
                      f"written (dense-DFT mel, no KV cache); " +
                      (f"ONE run at the GPU run's depth: {full_dt:.2f} s wall" if like and cpu_depth != int(depth)
                       else f"1 warm-up + {len(runs)} runs, median {cpu_dt:.2f} s wall"),
            "depth": int(depth) if like else cpu_depth,
            "depth32": {"value": round((n_cpu / sr) / cpu_dt, 3), "depth": cpu_depth,
                        "note": f"same window at depth {cpu_depth}: 1 warm-up + {len(runs)} runs, median {cpu_dt:.2f} s wall; "
                                f"NOT like-for-like with the GPU figure (shallower decode)",
                        "runs_s": [round(r, 3) for r in runs],
                        "stages_s": {"mel": round(t_mel, 3), "encoder": round(t_enc, 3),
                                     "decode": round(cpu_dt - t_mel - t_enc, 3), "total": round(cpu_dt, 3)}},
            "runs_s": [round(full_dt, 3)] if like and cpu_depth != int(depth) else [round(r, 3) for r in runs],
            "stages_s": {"mel": round(t_mel, 3), "encoder": round(t_enc, 3),
                         "decode": round(full_dt - t_mel - t_enc, 3), "total": round(full_dt, 3)},
            "host_cpus": os.cpu_count()}


GOLDEN_NPZ = os.path.join(ROOT, "tests", "golden", "oracle_outputs.npz")


def check_against_golden(rows, name, world, select=None):
    """Compare a leg's per-window token rows with the committed oracle rows of parity workload `name`
    (tests/golden/oracle_outputs.npz: frozen outputs of the oracle's LITERAL decode loop from raw PCM, tests/workloads.py;
    data, not oracle code -- nothing under oracle/ is imported here).  Runs OUTSIDE every timed region.  `select`: the window
    indices the golden holds (None = all).  A mismatch raises: a fast run that decodes other tokens is not a result.
    The goldens are rows of the 1-GPU audio (synth_audio is not prefix-stable, so the N-GPU clip is another signal): at
    N > 1 the leg reports tokens_checked = null."""
    if os.environ.get("WHISPER_BENCH_SKIP_TOKEN_CHECK") == "1":      # developer builds that decode garbage on purpose (the "dry" K10)
        return {"tokens_checked": False, "why": "WHISPER_BENCH_SKIP_TOKEN_CHECK=1: NOT a result"}
    if world != 1:
        return {"tokens_checked": None, "why": "golden rows exist for the 1-GPU clip only (tests/workloads.py)"}
    g = np.load(GOLDEN_NPZ)
    toks, lens = g[f"{name}_tokens"], g[f"{name}_lens"]
    want = [toks[i, :lens[i]].tolist() for i in range(len(lens))]
    sel = list(range(len(rows))) if select is None else list(select)
    assert len(sel) == len(want), (name, len(sel), len(want))
    n_tok = 0
    for wi, ref in zip(sel, want):
        got = [int(t) for t in rows[wi]]
        if got != ref:
            bad = next((j for j, (a, b) in enumerate(zip(got, ref)) if a != b), min(len(got), len(ref)))
            raise SystemExit(f"bench.py: leg `{name}` window {wi} differs from the oracle's committed row at position {bad} "
                             f"(got {got[bad:bad + 4]}, oracle {ref[bad:bad + 4]}): not reporting a figure for wrong tokens")
        n_tok += len(ref)
    return {"tokens_checked": True, "golden": f"tests/golden/oracle_outputs.npz:{name}", "windows_compared": sel,
            "tokens_compared": n_tok}


def kernel_table(kstats, pmc_bytes=lambda name: None):
    """Per-kernel-class rows of the profiled passes (attached HIP events per launch + algorithmic bytes): sorted by total
    time; the first row is the dominant kernel."""
    tot_ms = sum(k["total_ms"] for k in kstats) or 1.0
    rows = []
    for k in sorted(kstats, key=lambda k: -k["total_ms"]):
        avg_s = k["total_ms"] / k["calls"] * 1e-3
        per_launch = k["algo_bytes"] / k["calls"]
        ach = per_launch / avg_s / 1e9
        rows.append({"kernel": k["name"], "share_of_decode_kernel_time": round(k["total_ms"] / tot_ms, 4),
                     "launches_timed": k["calls"], "avg_launch_us": round(avg_s * 1e6, 2),
                     "algorithmic_bytes_per_launch": int(per_launch), "achieved_GBps": round(ach, 1),
                     "frac_of_hbm_peak": round(ach / HBM_PEAK_GBS, 4),
                     "traffic": pmc_bytes(k["name"])})
    return rows


def roofline_of(k0, traffic_source=None):
    return {"kernel": k0["kernel"], "bound": "hbm", "achieved": k0["achieved_GBps"], "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": k0["frac_of_hbm_peak"], "traffic": k0["traffic"],
            "traffic_source": traffic_source if k0["traffic"] is not None else None,
            "algorithmic_bytes_per_launch": k0["algorithmic_bytes_per_launch"],
            "avg_launch_us": k0["avg_launch_us"], "launches_timed": k0["launches_timed"],
            "share_of_decode_kernel_time": k0["share_of_decode_kernel_time"],
            "note": "dominant decode-step kernel by total duration; `kernels` lists every class"}


def profiled_passes(lib, _lib, decode_fn, n_prof):
    """`n_prof` extra passes with every decode-step launch carrying its own start / stop HIP events on the engine's stream
    (the dispatch's begin -> end, what `rocprofv3 --kernel-trace` reports).  Returns (stage milliseconds + counters, per-class stats)."""
    lib.wb_profile_enable(1)
    buf = np.zeros(8, dtype=np.float64)
    lib.wb_profile_read(buf.ctypes.data_as(_lib.c_double_p), 1)
    _lib.profile_kernels(reset=True)
    for _ in range(n_prof):
        decode_fn()
    lib.wb_profile_read(buf.ctypes.data_as(_lib.c_double_p), 1)
    kstats = _lib.profile_kernels(reset=True)
    lib.wb_profile_enable(0)
    return [float(x) for x in buf], kstats


def dump_outputs(dirname, tokens, per_window):
    """--dump-outputs: what the timed path handed its caller in the last timed step -- the stitched token ids
    (tokens.npy) and every window's token row (window_tokens.npy, -1 past window_lens.npy) -- as float64 arrays
    (token ids are exact there), so two builds can be compared output for output on the same seeded inputs."""
    os.makedirs(dirname, exist_ok=True)
    rows = [[int(t) for t in r] for r in per_window]
    win = np.full((len(rows), max((len(r) for r in rows), default=0)), -1.0, dtype=np.float64)
    for i, r in enumerate(rows):
        win[i, :len(r)] = r
    np.save(os.path.join(dirname, "tokens.npy"), np.asarray([int(t) for t in tokens], dtype=np.float64))
    np.save(os.path.join(dirname, "window_tokens.npy"), win)
    np.save(os.path.join(dirname, "window_lens.npy"), np.asarray([len(r) for r in rows], dtype=np.float64))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (default: a timed region of ~5 s)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run every extra leg, check and roofline (host-PCM leg, profiled passes, frontend leg, CPU "
                         "baseline, beam-5 and large-v2 legs, comparison with the committed oracle rows); off: the "
                         "headline figure only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (stitched token ids, per-window token rows) as DIR/<name>.npy")
    ap.add_argument("--model", default="tiny.en")
    ap.add_argument("--seconds", type=float, default=None,
                    help="audio seconds per GPU per step (default 30; one full window = 29.91 with --geometry whisper30)")
    ap.add_argument("--geometry", default="reference", choices=["reference", "whisper30"],
                    help="reference = the reference's windows (<= n_audio_ctx mel FRAMES = 14.9 s, mod.rs:236-241; the judged "
                         "configuration); whisper30 = the opt-in perf geometry of SURVEY 8d config 2(b): one window of "
                         "T = 2990 + 10 frames, C = 1500 encoder positions (wb_model_set_frame_limit)")
    ap.add_argument("--beam", type=int, default=1)
    ap.add_argument("--max-depth", type=int, default=100)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline leg")
    ap.add_argument("--mel-windows", type=int, default=256,
                    help="batched windows of the frontend-alone leg (--full; mel-frames/s; SURVEY 8d: >= 100)")
    ap.add_argument("--large-v2-leg", default="auto", choices=["auto", "on", "off"],
                    help="extra timed leg of --full: large-v2, --large-v2-seconds of audio per GPU (BASELINE.json's 8-GPU "
                         "headline is large-v2).  auto = with the greedy tiny.en reference-geometry run; "
                         "`value` stays the tiny.en figure in every case")
    ap.add_argument("--beam5-leg", default="auto", choices=["auto", "on", "off"],
                    help="extra timed leg of --full: the same workload with the reference's live beam_size 5 (auto: with "
                         "the greedy reference-geometry run)")
    ap.add_argument("--large-v2-seconds", type=float, default=450.0,
                    help="audio per GPU of the large-v2 leg (450 s = 38 windows = one GPU's share of the 8-GPU hour)")
    ap.add_argument("--dtype", default="f32", choices=["f32"],
                    help="the arithmetic type of the path's results (f32, as the reference's TchBackend<f32>); the bf16 speed "
                         "path of rounds 1-3 was retired")
    ap.add_argument("--encoder", default=None, choices=["f32", "split"],
                    help="encoder-side GEMMs of the f32 path: f32 = exact-f32 MFMA (default), split = three fp16 MFMAs per "
                         "product (f32-grade results, ~1.9x the rate); default: the library's (WHISPER_HIP_ENCODER_SPLIT)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.encoder is not None:                     # (read once per process by the library, at model load)
        os.environ["WHISPER_HIP_ENCODER_SPLIT"] = "1" if args.encoder == "split" else "0"
    if args.seconds is None:
        args.seconds = 478559 / 16000.0 if args.geometry == "whisper30" else 30.0

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU over RCCL, same flags
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.execvp(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                   f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
                                   "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:])

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)

    import whisper_burn_amd as wb
    from whisper_burn_amd import _lib, shard, synth

    lib = _lib.load()
    weights = synth.synth_preset(args.model)
    eng = wb.Whisper.from_tensors(weights, device=local_rank)
    if args.geometry == "whisper30":
        eng.set_frame_limit(True)
    V = eng.dims["n_vocab"]
    enc_gemm = eng.encoder_gemm()
    st = wb.SpecialTokens.for_vocab(V)
    params = wb.decode_params(st, beam_size=args.beam, max_depth=args.max_depth)

    sr = 16000
    n_total = int(round(args.seconds * sr)) * world
    audio = synth.synth_audio(n_total, synth.BENCH_AUDIO_SEED)         # seed 1234 + config#
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - params.padding)
    starts, lens = wb.window_extents(n_total, sr, wlen, params.overlap_seconds)
    n_win = len(starts)
    row_stride = 4 + args.max_depth + 4
    local_win = shard.partition_windows(n_win, rank, world)
    n_frames_local = int(sum(int(l) // 160 for l in lens[slice(*local_win)]))
    # a rank holds only the PCM span its own windows cover (resident in HBM before the timed region)
    span = shard.rank_pcm_span(starts, lens, *local_win)
    pcm_dev = torch.from_numpy(np.ascontiguousarray(audio[span[0]:span[1]])).to(dev)
    n_local = span[1] - span[0]

    def decode_local(lo, hi):
        # (lo, hi) are this rank's GLOBAL window indices; inside the span they are windows 0 .. hi - lo
        assert (lo, hi) == local_win
        return wb.waveform_to_tokens(eng, st, None, sr, params=params, win_begin=0, win_end=hi - lo,
                                     device_ptr=pcm_dev.data_ptr(), n_samples=n_local)[1]

    def step():
        return shard.transcribe_sharded(decode_local, wb.stitch_windows, n_win, rank, world, row_stride,
                                        device=dev if world > 1 else None)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    tokens = None
    for _ in range(args.warmup):
        tokens, _ = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tokens, per_window = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tokens, per_window)

    # what the process group actually looks like (so the driver's first SCALE line is self-checking): world size as
    # torch.distributed reports it, and every rank's device
    if world > 1:
        mine = torch.tensor([rank, local_rank, torch.cuda.current_device()], dtype=torch.int64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        ranks_observed = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                          "rank_local_rank_device": [[int(x) for x in t.tolist()] for t in allr]}
    else:
        ranks_observed = {"backend": None, "world_size": 1, "rank_local_rank_device": [[0, local_rank, torch.cuda.current_device()]]}

    # ---- the same step from HOST PCM (SURVEY 8d words the metric "PCM in host memory -> token ids on host"): the contract's
    # `value` is measured with the inputs resident in HBM; this leg hands the library the host buffer and lets it upload the
    # rank's span inside the timed region, so the PCIe-inclusive figure stands next to it
    from_host = None
    if args.full and args.steps >= 2:
        host_pcm = np.ascontiguousarray(audio[span[0]:span[1]])

        def decode_local_host(lo, hi):
            assert (lo, hi) == local_win
            return wb.waveform_to_tokens(eng, st, host_pcm, sr, params=params, win_begin=0, win_end=hi - lo)[1]

        def hstep():
            return shard.transcribe_sharded(decode_local_host, wb.stitch_windows, n_win, rank, world, row_stride,
                                            device=dev if world > 1 else None)

        h_steps = max(2, min(args.steps, 40))
        htok, _ = hstep()
        barrier()
        t0 = time.perf_counter()
        for _ in range(h_steps):
            htok, _ = hstep()
        barrier()
        hdt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([hdt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            hdt = float(t.item())
        assert list(htok) == list(tokens), "host-PCM path decoded different tokens"
        from_host = {"value": round(args.seconds * world * h_steps / hdt, 2), "unit": "x real-time", "steps": h_steps,
                     "ms_per_step": round(hdt / h_steps * 1e3, 3),
                     "h2d_bytes_per_step_per_gpu": int(host_pcm.nbytes),
                     "note": "identical step, but the PCM starts in pageable HOST memory and its upload is inside the timed "
                             "region (`value` above: PCM resident in HBM, as the bench contract prescribes)"}

    # ---- per-kernel roofline (profiled passes: every decode-step launch carries its own start / stop HIP events on
    # the engine's stream = the dispatch's begin -> end, the quantity `rocprofv3 --kernel-trace` reports) ----
    roofline = None
    kernels = None
    stages = None
    if args.full and rank == 0:
        n_prof = 3
        buf, kstats = profiled_passes(lib, _lib, lambda: decode_local(*local_win), n_prof)
        mel_ms, enc_ms, ckv_ms, dec_ms, n_steps, n_mel, logit_ms, n_logit = buf
        # measured HBM bytes per launch: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command,
        # corrected per MI355X_MICROARCH.md (profiles/summarize_pmc.py), keyed by kernel class; only used when the
        # file was collected on this workload (it records the command line)
        pmc = {}
        import glob
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_traffic_tiny_en_30s.json")))
        pmc_json = cands[-1] if cands else os.path.join(ROOT, "profiles", "none.json")     # the newest round's passes
        if args.model in ("tiny.en", "tiny_en") and args.dtype == "f32" and args.beam == 1 and args.seconds == 30.0 \
                and args.geometry == "reference" and os.path.exists(pmc_json):
            pmc = json.load(open(pmc_json))
        def pmc_bytes(cls_name):
            """HBM bytes per launch of the rocprof kernel(s) behind one profiler class (profiles/r02_pmc_*.json is keyed
            by the demangled kernel name)."""
            want = {"dec_persist": lambda n: "dec_persist_kernel" in n,
                    "dec_attn_fused": lambda n: "dec_attn_fused_kernel" in n,
                    "dec_mlp_fused": lambda n: "dec_mlp_fused_kernel" in n,
                    "dec_cross_attn": lambda n: "dec_cross_attn_kernel" in n,
                    "dec_cross_fused": lambda n: "dec_cross_fused_kernel" in n,
                    "dec_topk_merge": lambda n: "dec_topk_merge_kernel" in n,
                    "dec_gemv logits": lambda n: "dec_gemv_kernel" in n and "true, true" in n,
                    "dec_gemv cross-attn": lambda n: "dec_gemv_kernel" in n and "false, false, false" in n}
            for key, pred in want.items():
                if cls_name.startswith(key):
                    vals = [v for n, v in pmc.items() if pred(n)]
                    return int(max(vals)) if vals else None
            return None

        kernels = kernel_table(kstats, pmc_bytes)
        if kernels:
            roofline = roofline_of(kernels[0], os.path.relpath(pmc_json, ROOT))
        stages = {"mel_ms_per_step": round(mel_ms / n_prof, 4), "encoder_ms_per_step": round(enc_ms / n_prof, 4),
                  "cross_kv_ms_per_step": round(ckv_ms / n_prof, 4), "decode_ms_per_step": round(dec_ms / n_prof, 4),
                  "decode_steps_per_step": n_steps / n_prof,
                  "decode_launches_per_step": round(sum(k["calls"] for k in kstats) / n_prof, 2),
                  "mel_frames_per_s": round(n_frames_local / (mel_ms / n_prof * 1e-3), 1) if mel_ms > 0 else None,
                  "mel_GBps_algorithmic": round(960.0 * n_frames_local / (mel_ms / n_prof * 1e-3) / 1e9, 2) if mel_ms > 0 else None}

    enc_gemm_after = eng.encoder_gemm()     # ("f32" after "f16x3" at load: the split kernel's range guard tripped during the run)

    # ---- the frontend alone (BASELINE.json's second metric): >= 100 batched reference windows, PCM resident ----
    mel_frontend = None
    if args.full and rank == 0:
        n_mw = max(1, args.mel_windows)
        shift = int(wlen) - int(params.overlap_seconds * sr)
        n_mel = shift * (n_mw - 1) + int(wlen)
        big = pcm_dev.repeat((n_mel + n_local - 1) // n_local)[:n_mel].contiguous()
        m_starts, m_lens = wb.window_extents(n_mel, sr, wlen, params.overlap_seconds)
        Ts = eng.max_mel_frames()
        mel_out = torch.empty((len(m_starts), 80, Ts), dtype=torch.float32, device=dev)
        clip = eng.max_mel_frames() - params.padding
        wb.waveform_to_mels_dev(big.data_ptr(), n_mel, m_starts, m_lens, mel_out.data_ptr(), 80 * Ts, Ts, sr, clip,
                                params.padding, local_rank, iters=2)                       # warm-up
        iters = 20
        _, ms = wb.waveform_to_mels_dev(big.data_ptr(), n_mel, m_starts, m_lens, mel_out.data_ptr(), 80 * Ts, Ts, sr,
                                        clip, params.padding, local_rank, iters=iters)
        fr = int(sum(int(l) // 160 for l in m_lens))
        fps = fr * iters / (ms * 1e-3)
        mel_frontend = {"metric": "mel-frames/s", "value": round(fps, 1), "windows": len(m_starts), "frames_per_pass": fr,
                        "ms_per_pass": round(ms / iters, 4), "algorithmic_GBps": round(960.0 * fps / 1e9, 1),
                        "frac_of_hbm_peak": round(960.0 * fps / 1e9 / HBM_PEAK_GBS, 4),
                        "note": f"mel kernel + finalize on {n_mw} reference windows resident in HBM; 960 algorithmic "
                                "bytes per frame (640 B of PCM in, 320 B of log-mel out)"}
        del big, mel_out

    # ---- CPU baseline: the oracle (reference algorithm as written) on a bounded sample ----
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_baseline = run_cpu_baseline(weights, st, audio, sr, int(wlen), args.beam, args.max_depth, args.geometry,
                                        args.model)

    # ---- beam-5 leg: the reference's LIVE decode setting (transcribe.rs:232-233: beam_size 5, max_depth 100) on the same
    # model shape, audio and windows as the headline figure (greedy = the same code with beam_size 1).  Beam search
    # has no length normalisation (beam.rs:9-37), so on the headline checkpoint its beams end on <|endoftext|> after <= 26 tokens
    # -- a third of the greedy run's decode work (round 4's leg).  The leg therefore runs the parity workload `tiny_beam5`
    # (tests/workloads.py: the same recipe WITHOUT the EOT ramp): every window runs beam 5 to depth 100.  `value` stays greedy.
    beam5 = None
    if args.full and (args.beam5_leg == "on" or (args.beam5_leg == "auto" and args.beam == 1 and args.geometry == "reference")):
        bweights = synth.synth_preset(args.model, eot_beta=0.0)
        beng = wb.Whisper.from_tensors(bweights, device=local_rank)
        del bweights
        bparams = wb.decode_params(st, beam_size=5, max_depth=args.max_depth)

        def bdecode(lo, hi):
            assert (lo, hi) == local_win
            return wb.waveform_to_tokens(beng, st, None, sr, params=bparams, win_begin=0, win_end=hi - lo,
                                         device_ptr=pcm_dev.data_ptr(), n_samples=n_local)[1]

        def bstep():
            return shard.transcribe_sharded(bdecode, wb.stitch_windows, n_win, rank, world, row_stride,
                                            device=dev if world > 1 else None)

        b_steps, b_warm = max(2, min(10, args.steps)), min(2, args.warmup)
        for _ in range(b_warm):
            bstep()
        barrier()
        t0 = time.perf_counter()
        for _ in range(b_steps):
            btok, brows = bstep()
        barrier()
        bdt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([bdt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            bdt = float(t.item())
        bkern, bstages = None, None
        if rank == 0:
            # where the beam path's time goes: one profiled pass (attached HIP events per launch), like the other legs
            bbuf, bkstats = profiled_passes(lib, _lib, lambda: bdecode(*local_win), 1)
            bkern = kernel_table(bkstats)
            bstages = {"encoder_ms": round(bbuf[1], 3), "cross_kv_ms": round(bbuf[2], 3), "decode_ms_profiled_pass": round(bbuf[3], 3),
                       "decode_steps": bbuf[4], "decode_kernel_ms_sum": round(sum(k["total_ms"] for k in bkstats), 3),
                       "launches": int(sum(k["calls"] for k in bkstats))}
        beng.close()
        if rank == 0:
            standard = args.model in ("tiny.en", "tiny_en") and args.seconds == 30.0 and args.max_depth == 100 and args.geometry == "reference"
            bcheck = check_against_golden(brows, "tiny_beam5", world) if standard else \
                {"tokens_checked": None, "why": "no committed golden for this non-default workload"}
            beam5 = {"metric": "real-time factor (audio-sec/wall-sec)",
                     "value": round(args.seconds * world * b_steps / bdt, 2), "unit": "x real-time", "n_gpus": world,
                     "steps": b_steps, "warmup": b_warm, "ms_per_step": round(bdt / b_steps * 1e3, 3), "dtype": args.dtype,
                     "config": {"workload": f"{args.model} shape, checkpoint without the <|endoftext|> ramp (parity workload "
                                            f"tiny_beam5), {args.seconds:g} s of 16 kHz audio per GPU per step, reference windowing "
                                            f"({n_win} windows), beam_size 5, max_depth {args.max_depth} (the reference's live "
                                            f"setting, transcribe.rs:232-233)",
                                "tokens_out": len(btok), **bcheck,
                                "generated_tokens_per_window": [max(0, len(r) - 4) for r in brows],
                                "stages_profiled_pass": bstages, "kernels": bkern,
                                "path": "host-driven beam search (beam.rs restated in C++) over KV-cached session steps: fused "
                                        "sublayer kernels while <= 8 beams are live, batch mode above; the persistent kernel "
                                        "serves greedy only"}}

    # ---- large-v2 leg (BASELINE.json's multi-GPU headline config): every rank decodes --large-v2-seconds of audio ----
    large_v2 = None
    if args.full and (args.large_v2_leg == "on" or (args.large_v2_leg == "auto" and args.model in ("tiny.en", "tiny_en")
                                                    and args.geometry == "reference" and args.beam == 1)):
        eng.close()
        del pcm_dev
        # (checkpoint without the <|endoftext|> ramp: every window decodes max_depth tokens -- the leg's work does not depend
        # on where the synthetic checkpoint happens to end its rows; rounds 3 / 4 measured the same depth, mean 100.0)
        lw = synth.synth_preset("large-v2", eot_beta=0.0)
        leng = wb.Whisper.from_tensors(lw, device=local_rank)
        del lw
        leng_split = leng.encoder_gemm() == "f16x3"
        lst = wb.SpecialTokens.for_vocab(leng.dims["n_vocab"])
        lparams = wb.decode_params(lst, beam_size=1, max_depth=args.max_depth)
        ln_total = int(round(args.large_v2_seconds * sr)) * world
        laudio = synth.synth_audio(ln_total, synth.BENCH_AUDIO_SEED + 5)
        lstarts, llens = wb.window_extents(ln_total, sr, wlen, lparams.overlap_seconds)
        ln_win = len(lstarts)
        lwin = shard.partition_windows(ln_win, rank, world)
        lspan = shard.rank_pcm_span(lstarts, llens, *lwin)
        lpcm = torch.from_numpy(np.ascontiguousarray(laudio[lspan[0]:lspan[1]])).to(dev)
        del laudio

        def ldecode(lo_, hi_):
            assert (lo_, hi_) == lwin
            return wb.waveform_to_tokens(leng, lst, None, sr, params=lparams, win_begin=0, win_end=hi_ - lo_,
                                         device_ptr=lpcm.data_ptr(), n_samples=lspan[1] - lspan[0])[1]

        def lstep():
            return shard.transcribe_sharded(ldecode, wb.stitch_windows, ln_win, rank, world, row_stride,
                                            device=dev if world > 1 else None)

        # Warm-up until the step time has settled.  After an idle stretch of the GPU (this leg follows ~40 s of CPU-only work:
        # the oracle baseline) the first tens of seconds of heavy load run in a slow phase -- the encoder's MFMA GEMMs at a
        # third of their rate (599 vs 196 ms per step, identical kernels: profiles/r05_b_ab_decoder_split.txt, rep 1 vs rep 2)
        # -- which one fixed warm-up step does not outlast.  Untimed steps run until two consecutive ones agree within 3 %
        # with the fastest seen so far, at most 60 s; every warm-up step's time is listed next to the timed ones.
        l_steps, l_warm, l_warm_s = 5, 0, []
        warm_cap_s = float(os.environ.get("WHISPER_BENCH_LARGE_WARMUP_S", "60"))     # (tools/bench_dry_run.py: 0 = one warm-up step)
        tw0 = time.perf_counter()
        while True:
            t1 = time.perf_counter()
            lstep()
            torch.cuda.synchronize()
            l_warm_s.append(time.perf_counter() - t1)
            l_warm += 1
            settled = l_warm >= 3 and max(l_warm_s[-2:]) <= 1.03 * min(l_warm_s)
            stop = 1.0 if (settled or time.perf_counter() - tw0 > warm_cap_s or l_warm >= 64) else 0.0
            if world > 1:                                   # every rank leaves the warm-up together
                tflag = torch.tensor([stop], dtype=torch.float64, device=dev)
                dist.all_reduce(tflag, op=dist.ReduceOp.MIN)
                stop = float(tflag.item())
            if stop > 0.5:
                break
        barrier()
        t0 = time.perf_counter()
        l_step_s = []
        for _ in range(l_steps):
            t1 = time.perf_counter()
            ltok, lrows = lstep()
            l_step_s.append(time.perf_counter() - t1)   # (host-side per-step times: the leg's value is over the whole region)
        barrier()
        ldt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([ldt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ldt = float(t.item())
        if rank == 0:
            # the leg's own roofline: dominant batch-mode decode kernel of ONE profiled pass (attached HIP events per launch)
            lbuf, lkstats = profiled_passes(lib, _lib, lambda: ldecode(*lwin), 1)
            # measured HBM bytes per launch of the batch-mode kernels: the two --pmc passes of `bench.py --model large-v2
            # --seconds 450` (profiles/collect_r05*.sh -> profiles/r05_*_pmc_traffic_large_v2_450s.json), newest round
            import glob as _glob
            lcands = sorted(_glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_traffic_large_v2_450s.json")))
            lpmc = json.load(open(lcands[-1])) if lcands and args.large_v2_seconds == 450.0 else {}

            def lpmc_bytes(cls_name):
                want = {"batch: split-K MFMA GEMM": ("dec_skinny_f16x3_kernel", "dec_skinny_gemm_kernel"),
                        "batch: dec_resolve_ln": ("dec_resolve_ln_kernel",), "batch: dec_self_attn": ("dec_self_attn_kernel",),
                        "batch: dec_cross_attn_stream": ("dec_cross_attn_stream_kernel",),
                        "batch: dec_gelu_fold": ("dec_gelu_fold_kernel",), "batch: dec_topk_rows": ("dec_topk_rows_kernel",)}
                for key, frags in want.items():
                    if cls_name.startswith(key):
                        vals = [v for n, v in lpmc.items() if any(f in n for f in frags)]
                        # (several template instances share a class: launches differ in size, take the launch-weighted mean
                        # when the file carries it, else the largest)
                        return int(max(vals)) if vals else None
                return None

            lkern = kernel_table(lkstats, lpmc_bytes)
            lsrc = os.path.relpath(lcands[-1], ROOT) if lpmc else None
            l_enc_ms, l_ckv_ms, l_dec_ms, l_nsteps = lbuf[1], lbuf[2], lbuf[3], lbuf[4]
            lgen = [max(0, len(r) - 4) for r in lrows[lwin[0]:lwin[1]]]
            lenc_peak = "f16x3" if leng_split else args.dtype
            lrl = e2e_roofline_ms(leng.dims, llens[lwin[0]:lwin[1]], 3 + args.max_depth, args.dtype,
                                  leng.max_mel_frames() - lparams.padding, gen_lens=lgen, encoder_peak=lenc_peak)
            lwork = lrl.pop("_work")
            l_step_ms = ldt / l_steps * 1e3
            lcheck = check_against_golden(lrows, "large_leg", world, select=(0, ln_win - 1)) \
                if args.large_v2_seconds == 450.0 and args.max_depth == 100 and args.geometry == "reference" else \
                {"tokens_checked": None, "why": "no committed golden for this non-default workload"}
            l_dec_untraced = l_step_ms - l_enc_ms - l_ckv_ms - lbuf[0]
            large_v2 = {"metric": "real-time factor (audio-sec/wall-sec)",
                        "value": round(args.large_v2_seconds * world * l_steps / ldt, 2), "unit": "x real-time",
                        "n_gpus": world, "steps": l_steps, "warmup": l_warm, "ms_per_step": round(ldt / l_steps * 1e3, 2),
                        "dtype": args.dtype,
                        "config": {"workload": f"large-v2, {args.large_v2_seconds:g} s of 16 kHz audio per GPU per step, "
                                               f"reference windowing ({ln_win} windows), greedy, max_depth {args.max_depth}",
                                   "windows": ln_win, "tokens_out": len(ltok), **lcheck,
                                   "checkpoint": "large-v2 shape, synthetic, no <|endoftext|> ramp (every window runs to max_depth)",
                                   "generated_tokens_per_window_mean": round(float(np.mean([len(r) - 4 for r in lrows])), 1)},
                        "roofline": roofline_of(lkern[0], lsrc) if lkern else None,
                        "kernels": lkern,
                        "stages": {"encoder_ms_per_step": round(l_enc_ms, 2), "cross_kv_ms_per_step": round(l_ckv_ms, 2),
                                   "decode_ms_per_step_untraced": round(l_dec_untraced, 2),
                                   "decode_ms_per_step_profiled_pass": round(l_dec_ms, 2),
                                   "decode_kernel_ms_sum_profiled_pass": round(sum(k["total_ms"] for k in lkstats), 2),
                                   "decode_steps": l_nsteps,
                                   "encoder_TFLOPs_algorithmic": round(lwork["encoder_flops"] / ((l_enc_ms + l_ckv_ms) * 1e-3) / 1e12, 2) if l_enc_ms > 0 else None,
                                   "encoder_frac_of_mfma_peak": round(lwork["encoder_flops"] / ((l_enc_ms + l_ckv_ms) * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[lenc_peak], 4) if l_enc_ms > 0 else None,
                                   "decode_frac_of_hbm_peak": round(lwork["decode_bytes"] / (l_dec_untraced * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if l_dec_untraced > 0 else None,
                                   "note": "decode_ms_per_step_untraced = timed step - encoder - cross-K/V - mel (no events attached); the "
                                           "profiled pass attaches events to every launch, which inflates its wall time -- only its per-kernel "
                                           "durations are used"},
                        "e2e_roofline_ms_per_step": {k: round(v, 3) for k, v in lrl.items()},
                        "encoder_gemm": {"at_load": "f16x3" if leng_split else "f32", "after_the_leg": leng.encoder_gemm(),
                                         "note": "f16x3 -> f32 would mean the split-precision kernel's range guard tripped "
                                                 "(an activation outside fp16's range) and the encoder fell back to exact f32"},
                        "step_ms": [round(x * 1e3, 1) for x in l_step_s],
                        "warmup_step_ms": [round(x * 1e3, 1) for x in l_warm_s],
                        "target": ">= 50x real-time on 8 GPUs (BASELINE.json north_star)"}
        leng.close()

    if rank == 0:
        audio_s = args.seconds * world * args.steps
        rtf = audio_s / dt
        e2e = None
        hcheck = {"tokens_checked": None, "why": "plain run: the comparison with the committed oracle rows runs with --full"}
        if args.full:
            lo, hi = shard.partition_windows(n_win, rank, world)
            gen_lens = [max(0, len(r) - 4) for r in per_window[lo:hi]] if args.beam == 1 else None
            # (split-precision encoder: its MFMA peak is a third of the fp16 dense peak -- three instructions per product)
            enc_peak = enc_gemm if enc_gemm == "f16x3" else args.dtype
            rl = e2e_roofline_ms(eng.dims, lens[lo:hi], 3 + args.max_depth, args.dtype,
                                 eng.max_mel_frames() - params.padding, gen_lens=gen_lens, encoder_peak=enc_peak)   # per rank (weak scaling)
            work = rl.pop("_work")
            if stages:
                # achieved rates of the two big stages from their algorithmic work: encoder + cross-K/V from the profiled
                # passes (large kernels, launch mode does not matter), decode from the TIMED steps minus those stages
                enc_ms = stages["encoder_ms_per_step"] + stages["cross_kv_ms_per_step"]
                dec_ms = dt / args.steps * 1e3 - enc_ms - stages["mel_ms_per_step"]
                stages["encoder_TFLOPs_algorithmic"] = round(work["encoder_flops"] / (enc_ms * 1e-3) / 1e12, 2) if enc_ms > 0 else None
                stages["encoder_frac_of_mfma_peak"] = round(work["encoder_flops"] / (enc_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[enc_peak], 4) if enc_ms > 0 else None
                stages["decode_GBps_algorithmic"] = round(work["decode_bytes"] / (dec_ms * 1e-3) / 1e9, 1) if dec_ms > 0 else None
                stages["decode_frac_of_hbm_peak"] = round(work["decode_bytes"] / (dec_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if dec_ms > 0 else None
            hstandard = args.model in ("tiny.en", "tiny_en") and args.seconds == 30.0 and args.max_depth == 100 and args.beam == 1
            hcheck = check_against_golden(per_window, "tiny_bench" if args.geometry == "reference" else "tiny_whisper30", world) \
                if hstandard else {"tokens_checked": None, "why": "no committed golden for this non-default workload"}
            rl_rtf = args.seconds / (rl["total"] * 1e-3)
            e2e = {"roofline_rtf": round(rl_rtf, 1), "frac": round((rtf / world) / rl_rtf, 4),
                   "roofline_ms_per_step": {k: round(v, 4) for k, v in rl.items()},
                   "generated_tokens_per_window": gen_lens,
                   "note": "per-GPU roofline of the same step: algorithmic bytes over 8 TB/s (mel, decode) and FLOPs over "
                           "the dense MFMA peak of the path's dtype (encoder, cross-K/V); decode bytes are the NECESSARY ones "
                           "(weights once per step while any window is live, a window's cached K/V only while it is live); "
                           "decode is latency-bound at this size: the whole decode of a window batch is ONE persistent launch "
                           "(stages.decode_launches_per_step) whose 12 dependent roles per token hand planes over between CUs"}
        out = {
            "metric": "real-time factor (audio-sec/wall-sec)",
            "value": round(audio_s / dt, 2),
            "unit": "x real-time",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic (seeded synthetic weights at the real shapes; seeded synthetic 16 kHz audio)",
            "config": {"workload": f"{args.model}, {args.seconds:g} s of 16 kHz audio per GPU per step, "
                                   + (f"reference windowing ({n_win} windows <= 14.9 s, 3 s overlap)" if args.geometry == "reference"
                                      else f"opt-in Whisper geometry ({n_win} window(s) <= 29.9 s: T = 2990 + 10 frames, "
                                           f"C = 1500; not reference behaviour)") +
                                   f", HIP mel + encoder + "
                                   f"KV-cached decode, {'greedy (beam_size 1)' if args.beam == 1 else 'beam ' + str(args.beam)}, "
                                   f"max_depth {args.max_depth}",
                       "windows": n_win, "beam_size": args.beam, "max_depth": args.max_depth,
                       "encoder_gemm": {"f16x3": "split precision: three fp16 MFMAs per product on fp16 hi / lo pieces, f32 "
                                                 "accumulate (f32-grade results; WHISPER_HIP_ENCODER_SPLIT=0 selects exact-f32 MFMA)",
                                        "f32": "exact-f32 MFMA"}[enc_gemm],
                       "encoder_gemm_after_the_run": enc_gemm_after,
                       "tokens_out": len(tokens) if tokens is not None else 0, **hcheck,
                       "ranks_observed": ranks_observed,
                       "parallelism": f"windows sharded over {world} GPU(s), 1 token all-gather"},
            "roofline": roofline,
            "kernels": kernels,
            "cpu_baseline": cpu_baseline,
            "e2e_roofline": e2e,
            "from_host_pcm": from_host,
            "mel_frontend": mel_frontend,
            "stages": stages,
            "beam5": beam5,
            "large_v2": large_v2,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()                 # rank 0 is still printing / profiling while the others are done
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
