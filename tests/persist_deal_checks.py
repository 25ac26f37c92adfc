"""Child process of tests/test_gpu_persist_deal.py: the persistent decode kernel under the dealing that the environment selects
(WHISPER_HIP_PERSIST_DEAL; csrc/decode_chain.cpp: ps_deal_roles).  One engine of the d = 128 two-layer micro model decodes 3
windows, then 2 windows of other audio (another W under a reused session: the roles are dealt again); then the d = 384
four-layer model decodes 3 short windows -- the 4-row d = 384 instance on the full grid, the dealing the benchmark gets.
max_depth 8.  Prints one line `RESULT <json>`: per call the window rows."""
import json

import whisper_burn_amd as wb
from whisper_burn_amd import synth

# (model, n_state, n_head, n_layer, weight seed) and per model (call, samples, audio seed); n_audio_ctx = 400: windows of 62559
# samples, 14559 apart -- 40000 samples = 3 windows, 25000 = 2
MODELS = [("d128", 128, 2, 2, 218), ("d384", 384, 6, 4, 474)]
CALLS = {"d128": [("w3", 40000, 51), ("w2_other", 25000, 52)], "d384": [("w3", 40000, 51)]}
N_VOCAB, DEPTH = 2053, 8


def dims_of(d, n_head, n_layer):
    return synth.micro_dims(n_state=d, n_head=n_head, n_layer=n_layer, n_vocab=N_VOCAB, n_audio_ctx=400)


def main():
    out = {}
    st = wb.SpecialTokens.for_vocab(N_VOCAB)
    for name, d, n_head, n_layer, seed in MODELS:
        eng = wb.Whisper.from_tensors(synth.synth_weights(dims_of(d, n_head, n_layer), seed=seed))
        for call, n_s, aseed in CALLS[name]:
            rows = wb.waveform_to_tokens(eng, st, synth.synth_audio(n_s, aseed), 16000, 1, DEPTH)[1]
            out[f"{name}_{call}"] = [list(map(int, r)) for r in rows]
        eng.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
