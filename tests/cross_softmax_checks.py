"""Child process of tests/test_emu_cross_softmax.py and tests/test_gpu_cross_softmax.py: greedy decodes whose windows hold the
key counts at which the block-parallel softmax of the fused cross-attention body (csrc/decode_fused_bodies.h: dec_cross_body)
could lose a key, through whichever decode path the environment selects (the persistent kernel by default, the chain of one
launch per sublayer with WHISPER_HIP_PERSIST=0), token-exact against the oracle.

A case is one call: 3 - 4 windows of different audio lengths in one session.  A window of n samples has n // 160 mel frames and
C = (frames + 9) // 2 + 1 cached keys (padding 10, the stride-2 convolution), so C keys take (2 C - 11) * 160 samples; the check
reads the key count of every window back from the session (`encoder_output`) before it decodes.

`python cross_softmax_checks.py SET [MODEL ...]` runs every case of SET ("emu": the functional model's 384-key ring; "gpu": the
product's 768-key ring) on the named models (default: both) and prints `RESULT <json>`: per case the decoded rows.
`python cross_softmax_checks.py oracle SET` prints the oracle's rows instead (no engine).  The seeds below were fixed on the CPU before the body was changed: with them the functional
model of the PARENT commit (the 384-key library for "emu", the 768-key one for "gpu") is token-exact with the oracle on every
case."""
import json
import sys

import numpy as np
import torch

DEPTH, N_VOCAB, PAD = 8, 2053, 10
# model -> (n_state, n_head, n_layer, weight seed)
MODELS = {"d128": (128, 2, 2, 218), "d384": (384, 6, 4, 474)}
# set -> n_audio_ctx and the cases: name -> (frame limit x 2 -- the whisper30 geometry --, key counts per window, audio seed)
SETS = {
    "emu": (800, {
        "one_pass": (True, (383, 384, 6), 71),
        "two_pass_a": (True, (385, 511, 512, 513), 72),
        "two_pass_b": (True, (745, 768, 64), 73),
    }),
    "gpu": (1500, {
        "one_pass_a": (False, (63, 64, 65, 750), 81),
        "one_pass_b": (False, (511, 512, 513, 6), 82),
        "one_pass_w30": (True, (768, 750, 65), 83),
        "two_pass_a": (True, (769, 1023, 1024, 1025), 84),
        "two_pass_b": (True, (1500, 1025, 64), 85),
    }),
}


def samples_of(C):
    return max((2 * C - 11) * 160, 400)              # (400 samples, one FFT frame, are the shortest window: 2 frames, C = 6)


def layout(Cs):
    lens = np.array([samples_of(C) for C in Cs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return starts, lens


def main(argv):
    oracle_only = argv[0] == "oracle"
    if oracle_only:
        argv = argv[1:]
    which, only = argv[0], argv[1:]                  # (further arguments: the models to run, default all)
    n_audio_ctx, cases = SETS[which]
    from whisper_burn_amd import synth
    import parity_util as pu
    import whisper_burn_amd as wb
    st = wb.SpecialTokens.for_vocab(N_VOCAB)
    out = {}
    for model, (d, n_head, n_layer, wseed) in MODELS.items():
        if only and model not in only:
            continue
        dims = synth.micro_dims(n_state=d, n_head=n_head, n_layer=n_layer, n_vocab=N_VOCAB, n_audio_ctx=n_audio_ctx)
        w = synth.synth_weights(dims, seed=wseed)
        eng = None if oracle_only else wb.Whisper.from_tensors(w)
        limit_now = False
        for name, (limit, Cs, aseed) in cases.items():
            starts, lens = layout(Cs)
            a = synth.synth_audio(int(lens.sum()), aseed)
            if oracle_only:
                from oracle import mel as omel
                from oracle import transcribe as otr
                from oracle.model import OracleWhisper
                o = OracleWhisper(w, frame_limit_x2=limit)
                rows = []
                for s, n in zip(starts, lens):
                    mel = omel.prep_audio(torch.from_numpy(a[s:s + n])[None])
                    assert mel.shape[-1] == n // 160, (mel.shape, n)
                    rows.append(otr.mels_to_tokens(o, pu.ost(st), mel, PAD, 1, DEPTH))
            else:
                if limit != limit_now:
                    eng.set_frame_limit(limit)
                    limit_now = limit
                sess = wb.Session.begin(eng, a, starts, lens, max_beams=1, padding=PAD)
                got_C = tuple(sess.encoder_output(i).shape[0] for i in range(len(Cs)))
                assert got_C == tuple(Cs), (name, got_C, Cs)
                sess.set_special_mask(st.is_special)
                rows = sess.decode(wb.decode_params(st, 1, DEPTH, padding=PAD))
                sess.close()
            out[f"{model}_{name}"] = [list(map(int, r)) for r in rows]
        if eng is not None:
            eng.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
