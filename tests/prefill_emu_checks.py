"""Driven by tests/test_prefill_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: prefill.hip, the prefill
pass and the conditioned seek loop executed through the hipemu functional model at micro shapes, compared with
tests/prefill_ref.py and the oracle.  A check of the sources' logic on a machine without a GPU; tests/test_gpu_prefill_kernel.py
/ test_gpu_prefill.py are the parity tests proper."""
import sys

import prefill_ref as pf
import tsrules_ref as tr
import whisper_burn_amd as wb
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib


def check_store():
    for shape in pf.STORE_SHAPES:
        pf.check_store_case(shape)


def check_cache(i):
    import torch
    weights = pf.cache_weights()
    eng = wb.Whisper.from_tensors(weights)
    W, active, n = pf.CACHE_CASES[i]
    pf.check_cache_case(eng, OracleWhisper(weights), OracleWhisper(weights, dtype=torch.float64), W, active, n)
    eng.close()


def check_errors():
    eng = wb.Whisper.from_tensors(pf.cache_weights())
    pf.check_prefill_errors(eng)
    eng.close()


def check_chain(which):
    weights = tr.fixture()[0]
    eng = wb.Whisper.from_tensors(weights)
    pf.check_chain(eng, OracleWhisper(weights), which)
    eng.close()


def check_seek(beam):
    eng = pf.cond_engine()
    pf.check_conditioned_loop(eng, beam=beam)
    if not beam:
        pf.check_conditioning_off(eng)
        _, st, audio, R, sup, prompt = tr.fixture()
        p = wb.decode_params(st, 1, 6)
        tp = wb.TimestampParams(R["tb"], R["n_ts"])

        def status(**kw):
            try:
                wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=tp, suppress=sup, prompt=prompt, **kw)
            except wb.WbError as e:
                return e.status
            return 0

        lib = _lib.load()
        lib.wb_profile_enable(1)
        _lib.profile_kernels(reset=True)
        assert status(initial_prompt=[1, tr.FIX_V]) == -1 and status(initial_prompt=[-1]) == -1      # a history token out of range
        bad = wb.SpecialTokens.for_vocab(tr.FIX_V)
        bad.start_of_prev = tr.FIX_V
        try:
            wb.waveform_to_segments(eng, bad, audio, 16000, params=p, timestamps=tp, suppress=sup, prompt=prompt,
                                    condition_on_previous_text=True)
            rc = 0
        except wb.WbError as e:
            rc = e.status
        assert rc == -1
        assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
        lib.wb_profile_enable(0)
    eng.close()


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    which = sys.argv[1]
    if which == "store":
        check_store()
    elif which.startswith("cache_"):
        check_cache(int(which.split("_")[1]))
    elif which == "errors":
        check_errors()
    elif which.startswith("chain_"):
        check_chain(which[len("chain_"):])
    elif which.startswith("seek_"):
        check_seek(int(which.split("_")[1]))
    else:
        raise SystemExit(f"unknown check {which}")
    print("OK", which)
