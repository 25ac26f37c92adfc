"""Child process of tests/test_gpu_attn_rounds.py: the d = 384 four-layer synthetic model decodes 3 windows of different lengths
under the switches the environment sets (WHISPER_HIP_PERSIST_RESIDENT, WHISPER_HIP_PERSIST), max_depth 8.  Three rows on the
full grid: the `<6,4,1>` instance of the persistent kernel, whose self-attention role holds four QKV weight rounds in registers
(resident blocks: rounds 0, 1, 4, 5; WHISPER_HIP_PERSIST_RESIDENT=0: rounds 0 - 3, then 4, 5 streamed); layers 1 - 3 fold the
MLP planes of the layer in front.  Weight seed 480 with audio seed 52: the oracle's rows generate 8, 3 and 8 tokens -- the
middle row ends on <|endoftext|> with its third token, so from then on its roles skip their loads (`known_dead`) while the
other two rows run on; the case was token-exact with the oracle on the functional model before the body was changed.
Prints one line `RESULT <json>`: the window rows."""
import json

import whisper_burn_amd as wb
from whisper_burn_amd import synth

N_STATE, N_HEAD, N_LAYER, W_SEED = 384, 6, 4, 480
N_SAMPLES, A_SEED = 40000, 52          # n_audio_ctx = 400: windows of 62559 samples, 14559 apart -> 3 windows of different lengths
N_VOCAB, DEPTH = 2053, 8


def dims():
    return synth.micro_dims(n_state=N_STATE, n_head=N_HEAD, n_layer=N_LAYER, n_vocab=N_VOCAB, n_audio_ctx=400)


def main():
    st = wb.SpecialTokens.for_vocab(N_VOCAB)
    eng = wb.Whisper.from_tensors(synth.synth_weights(dims(), seed=W_SEED))
    rows = wb.waveform_to_tokens(eng, st, synth.synth_audio(N_SAMPLES, A_SEED), 16000, 1, DEPTH)[1]
    eng.close()
    print("RESULT " + json.dumps([list(map(int, r)) for r in rows]))


if __name__ == "__main__":
    main()
