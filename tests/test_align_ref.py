"""CPU: the alignment restatement (tests/align_ref.py) itself -- against the independent statement of its median filter and
DTW in `transformers`, the quality of the fixtures the GPU tests use (f32 and f64 restatement agree on every token, with a
10x noise margin), and the synthetic checkpoints' ground truth (positional heads look at encoder position ~3 p)."""
import os

import numpy as np
import pytest
import torch

import align_ref as ar
import parity_util as pu
import workloads
from whisper_burn_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_outputs.npz")


def rows_of(name):
    g = np.load(GOLD)
    t, n = g[f"{name}_tokens"], g[f"{name}_lens"]
    return [t[i, :n[i]].tolist() for i in range(len(n))]


def _hf():
    from transformers.models.whisper import generation_whisper       # (a broken import is a failure, not a skip)
    return generation_whisper


def _hf_start(x):
    ti, tj = _hf()._dynamic_time_warping(x)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    return tj[jumps].astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (5, 9), (9, 5), (13, 40)])
def test_dtw_equals_the_transformers_helper(shape):
    g = np.random.default_rng(shape[0] * 100 + shape[1])
    for x in (g.standard_normal(shape).astype(np.float32), g.integers(-2, 3, shape).astype(np.float32),
              np.zeros(shape, dtype=np.float32)):
        assert np.array_equal(ar.dtw_start_positions(x), _hf_start(x))


@pytest.mark.parametrize("width", [1, 3, 7, 15])
def test_median_filter_equals_the_transformers_helper(width):
    g = np.random.default_rng(width)
    for C in (1, 3, 8, 16, 50):
        # small integers (exact ties), and with noise on top for the odd lengths; axes of C <= pad are passed through
        x = g.integers(-3, 4, (2, 5, C)).astype(np.float32) + g.standard_normal((2, 5, C)).astype(np.float32) * (C % 2)
        x = torch.from_numpy(x)
        assert torch.equal(ar.median_filter(x, width), _hf()._median_filter(x, width))


def _fixture_quality(w, rows, encs, name):
    o32, o64 = ar.AlignOracle(w), ar.AlignOracle(w, dtype=torch.float64)
    g = np.random.default_rng(0)
    for i, (row, enc) in enumerate(zip(rows, encs)):
        dl = 1 if row[-1] == len(w["decoder/token_embedding/weight"]) - 16 else 0
        m32 = ar.alignment_matrix(o32, row, enc).numpy()
        m64 = ar.alignment_matrix(o64, row, enc).numpy()
        d32 = float(np.abs(m32 - m64).max())
        p32 = ar.start_positions(m32, 4, dl)
        p64 = ar.start_positions(m64, 4, dl, dtw_dtype=np.float64)
        print(f"{name} row {i}: d32 {d32:.2e}")
        assert np.array_equal(p32, p64), (name, i)
        noisy = m64 + g.standard_normal(m64.shape) * 10 * d32
        assert np.array_equal(ar.start_positions(noisy, 4, dl, dtw_dtype=np.float64), p64), (name, i)


@pytest.mark.parametrize("name", ["tiny_bench", "base_beam5_eot", "large_window"])
def test_fixture_rows_align_identically_in_f32_and_f64(name):
    wl = workloads.WORKLOADS[name]
    w = wl.weights()
    o32 = ar.AlignOracle(w)
    encs = [o32.forward_encoder(m)[0].numpy() for m in pu.window_mels(o32, wl.audio())]
    _fixture_quality(w, rows_of(name), encs, name)


def test_micro_model_rows_align_identically_in_f32_and_f64():
    """The micro model of the GPU test (seed 77, 20 s of audio, greedy to depth 40), rows from the oracle's own decode."""
    import whisper_burn_amd as wb
    from oracle import transcribe as otr
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
    w = synth.synth_weights(dims, seed=77)
    o32 = ar.AlignOracle(w)
    audio = synth.synth_audio(16000 * 20, 4)
    _, rows = otr.waveform_to_tokens(o32, pu.ost(wb.SpecialTokens.for_vocab(1031)), audio, 16000, 1, 40, return_windows=True)
    encs = [o32.forward_encoder(m)[0].numpy() for m in pu.window_mels(o32, audio)]
    _fixture_quality(w, rows, encs, "micro")


def test_positional_heads_follow_three_positions_per_token():
    wl = workloads.WORKLOADS["tiny_bench"]
    w = wl.weights()
    o32 = ar.AlignOracle(w)
    enc = o32.forward_encoder(pu.window_mels(o32, wl.audio())[0])[0].numpy()
    D = o32.dims
    heads = [(l, h) for l in range(D.n_text_layer) for h in range(D.n_text_head // 2)]
    row = rows_of("tiny_bench")[0]
    pos = ar.start_positions(ar.alignment_matrix(o32, row, enc, heads).numpy(), 4, 0)
    # the first 80 aligned tokens: the path must end in the last position, which pulls the row's final tokens away
    idx = np.nonzero(pos >= 0)[0][:80]
    slope = float(np.polyfit(idx.astype(np.float64), pos[idx].astype(np.float64), 1)[0])
    assert abs(slope - 3.0) <= 0.1, slope


def test_constant_column_gives_zeros():
    w = torch.tensor([[0.25, 0.5], [0.25, 0.1], [0.25, 0.4]])
    mean = w.mean(0, keepdim=True)
    std = torch.sqrt(((w - mean) ** 2).mean(0, keepdim=True))
    assert std[0, 0] == 0
    z = torch.where(std > 0, (w - mean) / torch.where(std > 0, std, torch.ones_like(std)), torch.zeros_like(w))
    assert torch.equal(z[:, 0], torch.zeros(3)) and torch.isfinite(z).all()
