"""Child process of tests/test_emu_persist_pick.py and tests/test_gpu_persist_pick.py: one synthetic model decodes one clip
greedily under the switches the environment sets (WHISPER_HIP_PERSIST_PICK, WHISPER_HIP_PERSIST_RESIDENT, WHISPER_HIP_PERSIST,
HIPEMU_CUS).  The cells (model, clip, depth):
  d384   d = 384, 4 layers, 3 windows of different lengths, max_depth 8 (weight seed 480, audio seed 52): the rows generate 8, 3
         and 8 tokens -- the middle row ends on <|endoftext|> with its third token while the others run on;
  d512   d = 512, 2 layers, 4 windows, max_depth 12 (the `persist512` model and clip of tests/emu_checks.py);
  d128   d = 128, 2 layers, ONE window, max_depth 10;
  early  d = 128, 2 layers, 3 windows, <|endoftext|> pushed up (eot_ramp) and left OUT of the special-token mask (under the
         mask no row can end before its third token): two rows end on their FIRST generated token -- the pick of the first
         step behind the prompt already takes the row-end path -- while the third runs on for six.
`python persist_pick_checks.py CELL` prints one line `RESULT <json>`: the window rows.  oracle_rows(cell) is the CPU oracle's."""
import json
import sys

import numpy as np

import whisper_burn_amd as wb
from whisper_burn_amd import synth

CELLS = {
    # name: (n_state, n_layer, n_vocab, n_audio_ctx, weight seed, weight overrides, samples, audio seed, depth, eot unmasked)
    "d384": (384, 4, 2053, 400, 480, {}, 40000, 52, 8, False),
    "d512": (512, 2, 2053, 400, 90 + 512, {}, 50000, 51, 12, False),
    "d128": (128, 2, 1031, 1500, 4242, {}, 16000 * 3, 7, 10, False),
    "early": (128, 2, 1031, 400, 4242, {"eot_ramp": (5.5, 3.5)}, 40000, 52, 6, True),
}


def setup(cell):
    d, nl, nv, ctx, ws, over, ns, aseed, depth, unmask_eot = CELLS[cell]
    dims = synth.micro_dims(n_state=d, n_head=d // 64, n_layer=nl, n_vocab=nv, n_audio_ctx=ctx)
    st = wb.SpecialTokens.for_vocab(nv)
    if unmask_eot:
        st.is_special = np.array(st.is_special, copy=True)
        st.is_special[st.end_of_text] = False
    return synth.synth_weights(dims, seed=ws, **over), st, synth.synth_audio(ns, aseed), depth


def oracle_rows(cell):
    import parity_util as pu
    from oracle import transcribe as otr
    from oracle.model import OracleWhisper
    w, st, audio, depth = setup(cell)
    rows = otr.waveform_to_tokens(OracleWhisper(w), pu.ost(st), audio, 16000, 1, depth, return_windows=True)[1]
    return [list(map(int, r)) for r in rows], int(st.end_of_text)


def main(cell):
    w, st, audio, depth = setup(cell)
    eng = wb.Whisper.from_tensors(w)
    rows = wb.waveform_to_tokens(eng, st, audio, 16000, 1, depth)[1]
    eng.close()
    print("RESULT " + json.dumps([list(map(int, r)) for r in rows]))


if __name__ == "__main__":
    main(sys.argv[1])
