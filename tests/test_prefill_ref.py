"""CPU: the restatements of tests/prefill_ref.py against hand cases, and the fixture's long prompt on the oracle alone.

 * store_ref on a hand case;
 * the seek loop's prompt rule (build_prompt / update_history / conditioned_loop_ref) on scripted windows against prompts
   written out by hand, and five mutants -- truncation from the front, <|startofprev|> on an empty history, timestamps
   dropped from the history, the tail behind the last pair appended, no reset at T > 0.5 -- each of which changes a scripted
   result;
 * the long prompt of the chain tests keeps the fixture inside the 5 % exclusion cap, on the oracle alone."""
import numpy as np
import pytest

import prefill_ref as pf
import tsrules_ref as tr


def test_store_restatement_on_a_hand_case():
    nA, n, S, Lmax, d = 2, 3, 4, 5, 4
    qkv = np.arange(nA * n * 3 * d, dtype=np.float32).reshape(nA * n, 3 * d)
    K, V = np.full((Lmax * S, d), -1, np.float32), np.full((Lmax * S, d), -1, np.float32)
    tabs = np.full((2, S, Lmax), -7, np.int32)
    pf.store_ref(qkv, nA, n, d, S, Lmax, K, V, tabs)
    assert K[2 * S + 1].tolist() == qkv[1 * n + 2, d:2 * d].tolist() == [64.0, 65.0, 66.0, 67.0]     # (a, p) = (1, 2): row 5 of qkv
    assert V[0 * S + 0].tolist() == [8.0, 9.0, 10.0, 11.0]
    assert tabs[0, 1, :3].tolist() == [1, 5, 9] and (tabs[1] == -7).all() and (tabs[0, 2:] == -7).all() and tabs[0, 0, 3] == -7
    assert int((K != -1).any(axis=1).sum()) == nA * n and (K[3] == -1).all()                       # slot 3 is not an active window


def test_prompt_rule_on_hand_cases():
    assert pf.history_cap(-1, 448) == 223 and pf.history_cap(-1, 64) == 31 and pf.history_cap(5, 448) == 5 and pf.history_cap(0, 64) == 0
    assert pf.build_prompt([], [90, 91, 92], 95, 6) == [90, 91, 92]
    assert pf.build_prompt([1, 2], [90, 91, 92], 95, 6) == [95, 1, 2, 90, 91, 92]
    assert pf.build_prompt([1, 2, 3, 4], [90], 95, 3) == [95, 2, 3, 4, 90]
    assert pf.build_prompt([1, 2, 3, 4], [90], 95, 0) == [90]
    # the scripted windows (prefill_ref.scripted_loop), cap 6: what each window is prompted with, written out by hand
    P = [90, 91, 92]
    w0 = [100, 5, 6, 110, 110, 7, 120]                 # covered by window 0's two segments; its tail (120, 8, 9) is not
    w1 = [100, 11, 12, 13, 125]
    w2 = [100, 21, 22]                                 # no pair: one segment over everything
    got = pf.scripted_loop()
    assert got[0] == P
    assert got[1] == [95] + w0[-6:] + P
    assert got[2] == [95] + (w0 + w1)[-6:] + P == [95, 120, 100, 11, 12, 13, 125] + P
    assert got[3] == [95] + (w1 + w2)[-6:] + P
    # conditioning off: an initial prompt reaches the first window only; on: it is the start of the history
    off = pf.scripted_loop(condition=False, initial=[1, 2])
    assert off[0] == [95, 1, 2] + P and all(p == P for p in off[1:])
    on = pf.scripted_loop(initial=[1, 2], cap=20)
    assert on[0] == [95, 1, 2] + P and on[1] == [95, 1, 2] + w0 + P
    # T > 0.5 resets after every window, T = 0.5 does not
    assert all(p == P for p in pf.scripted_loop(temperature=0.6)) and pf.scripted_loop(temperature=0.5) == got


@pytest.mark.parametrize("mut", pf.SEEK_MUTANTS)
def test_every_mutant_of_the_prompt_rule_changes_a_scripted_result(mut):
    kw = dict(temperature=0.6) if mut == "no_reset" else {}
    assert pf.scripted_loop(mut=mut, **kw) != pf.scripted_loop(**kw), mut


def test_the_long_prompt_keeps_the_fixture_inside_the_exclusion_cap():
    from oracle.model import OracleWhisper
    _, st, _, R, _, _ = tr.fixture()
    prompt = pf.long_prompt(st)
    assert len(prompt) == 24 and len(set(pf.LONG_IDS)) == 20
    assert not any(st.is_special[t] or tr.is_ts(R, t) for t in pf.LONG_IDS) and prompt[0] == st.start_of_prev
    (n, ex), (bn, bex) = pf.oracle_fixture_exclusions(OracleWhisper(tr.fixture()[0]))
    print("greedy positions / excluded:", n, ex, "beam-5 window-steps / excluded:", bn, bex)
    assert n >= 12 and ex <= 0.05 * n and bn >= 12 and bex <= 0.05 * bn


def test_cli_rejects_the_conditioning_flags_without_segments(capsys):
    from whisper_burn_amd import transcribe as cli
    for flags in (["--condition-on-previous-text"], ["--initial-prompt", "hello"], ["--segments", "s.jsonl", "--initial-prompt"]):
        assert cli.main(["transcribe", "no_such_model", "no_such.wav", "en", "no_such_out.txt"] + flags) == 1
    assert "need --segments" in capsys.readouterr().err
