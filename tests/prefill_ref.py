"""The one-pass prompt prefill and the conditioned seek loop, restated: the store kernel on caller arrays, a slot's cached K / V
from the oracle's own layer_norm / linear, the next steps against the f32 oracle, the chains behind a long prompt by the
existing teacher-forced schemes (tsrules_ref / tsbeam_ref / sample_ref), the seek loop's prompt rule with its mutants.  Shared by
tests/test_prefill_ref.py (CPU), tests/prefill_emu_checks.py (functional model) and tests/test_gpu_prefill*.py."""
import numpy as np

import sample_ref as sr
import tsbeam_ref as tb
import tsrules_ref as tr

# ---- the store kernel ------------------------------------------------------------------------------------------------------------
STORE_SHAPES = [(1, 1, 1, 8, 64, 192), (3, 5, 5, 8, 128, 384 + 8), (2, 33, 16, 40, 64, 192)]     # (nA, n, S, Lmax, d, ld)
CANARY_F = np.array([0x7FC5A5A5], dtype=np.uint32).view(np.float32)[0]       # a NaN with a payload: compared by bits
CANARY_I = np.int32(-0x5A5A5A5B)


def store_ref(qkv, nA, n, d, S, Lmax, Kc, Vc, tabs):
    """What prefill_store_kernel does to the three arrays (in place)."""
    for a in range(nA):
        for p in range(n):
            row = p * S + a
            Kc[row] = qkv[a * n + p, d:2 * d]
            Vc[row] = qkv[a * n + p, 2 * d:3 * d]
            tabs[(n - 1) & 1, a, p] = row


def check_store_case(shape, seed=0, device=0):
    """K and V rows bit-exact at p * S + a, table entries exact in parity (n - 1) & 1, every other word still its canary."""
    import whisper_burn_amd as wb
    nA, n, S, Lmax, d, ld = shape
    g = np.random.default_rng(seed)
    qkv = g.standard_normal((nA * n, ld)).astype(np.float32)
    got = [np.full((Lmax * S, d), CANARY_F, dtype=np.float32), np.full((Lmax * S, d), CANARY_F, dtype=np.float32),
           np.full((2, S, Lmax), CANARY_I, dtype=np.int32)]
    ref = [a.copy() for a in got]
    store_ref(qkv, nA, n, d, S, Lmax, *ref)
    wb.prefill_store(qkv, nA, n, d, S, Lmax, *got, device=device)
    for name, a, b in zip(("K", "V", "tabs"), got, ref):
        assert np.array_equal(tr.bits(a), tr.bits(b)), (shape, name, int((tr.bits(a) != tr.bits(b)).sum()))
    n_canary = int((tr.bits(got[2]) == tr.bits(np.array([CANARY_I]))[0]).sum())
    assert n_canary == 2 * S * Lmax - nA * n, (shape, n_canary)             # (no table entry equals the canary by accident)
    return got


# ---- the cache and the next steps --------------------------------------------------------------------------------------------------
CACHE_CASES = [(3, None, 1), (3, None, 2), (3, None, 8), (3, None, 33), (4, [1, 0, 1, 1], 7)]     # (W, active, n)
CACHE_MAX_BEAMS = 3


def cache_weights():
    from whisper_burn_amd import synth
    return synth.synth_weights(synth.micro_dims(), seed=5)


def cache_tokens(n, seed=11):
    """n prompt tokens and the one behind them: non-special ids of the micro vocabulary."""
    return [int(t) for t in np.random.default_rng(seed).integers(1, 700, n + 1)]


def oracle_self_kv(oracle, tokens, enc):
    """Per decoder layer (K, V) [n, d] of `tokens` as the self-KV cache holds them: the oracle's own layer_norm / linear, K times
    d_h^-0.25 (in the oracle's precision: qkv_attention's scale)."""
    import torch
    w, D = oracle.w, oracle.dims
    toks = torch.tensor([list(tokens)], dtype=torch.long)
    xa = torch.as_tensor(np.asarray(enc)).to(oracle.dtype)[None]
    x = w["decoder/token_embedding/weight"][toks] + w["decoder/positional_embedding"][0:len(tokens)][None]
    dh = D.n_text_state // D.n_text_head
    scale = float(np.float32(dh ** -0.25)) if oracle.dtype == torch.float32 else dh ** -0.25
    out = []
    for i in range(D.n_text_layer):
        p = f"decoder/block_{i}"
        h = oracle.layer_norm(p + "/attn_ln", x)
        out.append(((oracle.linear(p + "/attn/key", h) * scale)[0].double().numpy(), oracle.linear(p + "/attn/value", h)[0].double().numpy()))
        x = x + oracle.self_attention(p + "/attn", h, oracle.mask, D.n_text_head)
        x = x + oracle.cross_attention(p + "/cross_attn", oracle.layer_norm(p + "/cross_attn_ln", x), xa, D.n_text_head)
        x = x + oracle.mlp(p + "/mlp", oracle.layer_norm(p + "/mlp_ln", x))
    return out


def cache_session(eng, W):
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    audio = synth.synth_audio(48000, 3)
    return wb.Session.begin(eng, audio, np.array(tr.FIX_OFFSETS[:W], dtype=np.int64), np.full(W, 16000, dtype=np.int64),
                            max_beams=CACHE_MAX_BEAMS)


def step_prefill(sess, tokens, wa):
    """The n prefill steps the pass replaces."""
    nA = len(wa)
    for t, tok in enumerate(tokens):
        sess.step([tok] * nA, [-1] * nA if t == 0 else list(range(nA)), wa, k=0)


def check_cache_kv(sess, o32, o64, tokens, wa, who, record=None):
    """self_kv of every active slot and layer against the f64 oracle: max |engine - f64| <= 4 d32 + 1e-7 max |f64|, d32 the f32
    oracle's own distance from the f64 one on the same entries (DESIGN.md section 10's yardstick).  Returns the largest ratio."""
    n, NL = len(tokens), o32.dims.n_text_layer
    worst = 0.0
    for a, w in enumerate(wa):
        enc = sess.encoder_output(w)
        r32, r64 = oracle_self_kv(o32, tokens, enc), oracle_self_kv(o64, tokens, enc)
        for layer in range(NL):
            got = sess.self_kv(layer, a, n)
            for name, g, a32, a64 in zip("KV", got, r32[layer], r64[layer]):
                err, d32 = float(np.abs(g.astype(np.float64) - a64).max()), float(np.abs(a32 - a64).max())
                bound = 4 * d32 + 1e-7 * float(np.abs(a64).max())
                print(f"prefill cache {who} n={n} slot={a} layer={layer} {name}: err {err:.3e} d32 {d32:.3e} bound {bound:.3e}")
                if record is not None:
                    record(f"{who}/n{n}/slot{a}/L{layer}{name}", err / bound)
                assert err <= bound, (who, n, a, layer, name, err, d32, bound)
                worst = max(worst, err / bound)
    return worst


def _oracle_logprobs(o32, enc, row):
    import torch
    from oracle.model import log_softmax
    x = o32.forward_decoder(torch.tensor([list(row)], dtype=torch.long), torch.as_tensor(np.asarray(enc))[None])[0, -1]
    return log_softmax(x.double(), 0).numpy()


def check_step_rows(ids, lps, rows, encs, o32, who, record=None):
    """A step's k best per row against the f32 oracle: log-probs within the project's 1e-3, top-1 equal wherever the oracle's
    top-two gap exceeds 2e-3."""
    worst = 0.0
    for r, (row, enc) in enumerate(zip(rows, encs)):
        ref = _oracle_logprobs(o32, enc, row)
        err = float(np.abs(lps[r].astype(np.float64) - ref[ids[r]]).max())
        worst = max(worst, err)
        assert err <= 1e-3, (who, r, err)
        top = np.sort(ref)[::-1]
        if top[0] - top[1] > 2e-3:
            assert int(ids[r, 0]) == int(np.argmax(ref)), (who, r, int(ids[r, 0]), int(np.argmax(ref)))
    print(f"prefill step {who}: worst |log-prob - oracle| {worst:.3e} (tol 1e-3, {len(rows)} rows)")
    if record is not None:
        record(who, worst)
    return worst


def check_cache_case(eng, o32, o64, W, active, n, record_ratio=None, record_lp=None):
    """One case of CACHE_CASES: the cache behind Session.prefill and behind the n steps under the same bound, then one step and
    two forking steps behind the pass against the f32 oracle."""
    toks = cache_tokens(n)
    prompt, last = toks[:n], toks[n]
    wa = [w for w in range(W) if active is None or active[w]]
    nA = len(wa)
    name = f"W{W}{'a' if active is not None else ''}"
    ref = cache_session(eng, W)
    step_prefill(ref, prompt, wa)
    check_cache_kv(ref, o32, o64, prompt, wa, name + "/steps", record_ratio)
    ref.close()
    sess = cache_session(eng, W)
    sess.prefill(prompt, active)
    check_cache_kv(sess, o32, o64, prompt, wa, name + "/pass", record_ratio)
    encs = [sess.encoder_output(w) for w in wa]
    rows, renc, win = [prompt + [last] for _ in wa], list(encs), list(wa)
    ids, lps = sess.step([last] * nA, list(range(nA)), wa, k=5)
    check_step_rows(ids, lps, rows, renc, o32, f"{name}/n{n}/step0", record_lp)
    for s in (1, 2):                                   # forks: rows 0 and 1 both continue slot 0, row i >= 2 continues slot i - 1
        par = [0, 0] + list(range(1, len(rows)))
        tok = [int(ids[0, 0]), int(ids[0, 1])] + [int(ids[q, 0]) for q in range(1, len(rows))]
        rows = [rows[q] + [t] for q, t in zip(par, tok)]
        renc, win = [renc[q] for q in par], [win[q] for q in par]
        NL = o32.dims.n_text_layer
        before = [[sess.self_kv(layer, q, len(rows[0]) - 1) for layer in range(NL)] for q in range(len(set(par)))]
        ids, lps = sess.step(tok, par, win, k=5)
        check_step_rows(ids, lps, rows, renc, o32, f"{name}/n{n}/step{s}", record_lp)
        for q in range(len(rows)):                     # ... and the tables survived the parent copy: a row's cached positions
            for layer in range(NL):                    # in front of its new token are its parent's rows, bit for bit
                K, V = sess.self_kv(layer, q, len(rows[q]))
                assert np.isfinite(K[-1]).all() and np.isfinite(V[-1]).all()
                for got, ref in zip((K, V), before[par[q]][layer]):
                    assert np.array_equal(tr.bits(got[:-1]), tr.bits(ref)), (name, n, s, q, layer)
    sess.close()


def check_prefill_errors(eng):
    """Not fresh, n >= Lmax, a token out of range: the status, and nothing launched."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import _lib
    lib = _lib.load()
    lib.wb_profile_enable(1)

    def status(fn):
        try:
            fn()
        except wb.WbError as e:
            return e.status
        return 0

    sess = cache_session(eng, 2)
    V, L = eng.dims["n_vocab"], eng.dims["n_text_ctx"]
    sess.step([1, 1], [-1, -1], [0, 1], k=0)
    _lib.profile_kernels(reset=True)
    assert status(lambda: sess.prefill([1, 2, 3])) == -6                       # not fresh
    sess.rewind()
    assert status(lambda: sess.prefill([1, V, 3])) == -1                       # a token out of range
    assert status(lambda: sess.prefill([1, -1])) == -1
    assert status(lambda: sess.prefill([1] * min(L, 448))) == -2               # n >= Lmax
    assert status(lambda: sess.prefill([1, 2], active=[0, 0])) == -1           # no active window
    assert status(lambda: sess.set_prefill(2)) == -1
    assert status(lambda: sess.prefill([])) == 0                               # n == 0: a no-op
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status(lambda: sess.prefill([1, 2, 3])) == 0
    names = {k["name"].split(" ")[0] for k in _lib.profile_kernels(reset=True)}
    assert "prefill_store" in names and "dec_prepare" not in names, names
    assert status(lambda: sess.prefill([1, 2, 3])) == -6                       # not fresh any more
    sess.close()
    lib.wb_profile_enable(0)


# ---- the chains behind a long prompt ---------------------------------------------------------------------------------------------------
# 20 non-special, non-timestamp ids of the micro fixture (tests/test_prefill_ref.py: the oracle alone stays inside the 5 % cap)
LONG_IDS = [772, 629, 405, 36, 105, 39, 304, 524, 220, 225, 43, 18, 119, 1, 496, 368, 799, 324, 453, 633]
CHAINS = ("ts_3_1", "ts_3_5", "beam_3_5", "sample_3_5", "prompt_greedy", "greedy")


def long_prompt(st):
    return [st.start_of_prev] + LONG_IDS + [st.start_of_transcript, st.language, st.transcribe]


def oracle_fixture_exclusions(o32, depth=tr.FIX_DEPTH, W=3):
    """The oracle alone behind the long prompt on the fixture's windows: (positions, excluded) of the greedy timestamp decode
    and (window-steps, excluded) of the beam-5 search under its replay rule."""
    _, st, audio, R, sup, _ = tr.fixture()
    prompt = long_prompt(st)
    n = ex = bn = bex = 0
    for enc in tr.fixture_encs(o32, audio, W):
        row, steps = tr.oracle_decode(o32, enc, prompt, R, st.end_of_text, sup, None, depth)
        n += len(steps)
        ex += sum(1 for d in steps if tr.is_excluded(d, tr.FIX_V, 0.0, model=True))
        _, a, b = tb.oracle_search(o32, enc, prompt, R, st.end_of_text, sup, 5, 1.0, depth)
        bn, bex = bn + a, bex + b
    return (n, ex), (bn, bex)


def _ts_rows_check(sess, o32, st, R, sup, prompt, rows_sums_best, gens, T, seed, attempt, best_of, cap, who):
    rows, sums, best = rows_sums_best
    P = len(prompt)
    n = ex = bad = 0
    for w in range(sess.n_windows):
        enc = sess.encoder_output(w)
        ranks = []
        for j in range(best_of):
            gen = gens[w][j]
            tr.check_invariants(gen, R, st.end_of_text, sup)
            a, b, c, total = tr.oracle_row_check(o32, enc, prompt + gen, P, R, st.end_of_text, sup, None, T, seed, w * best_of + j, attempt)
            n, ex, bad = n + a, ex + b, bad + c
            assert abs(sums[w, j] - total) <= 1e-3 * len(gen), (who, w, j, sums[w, j], total)
            nt = sr.n_text(gen, st.end_of_text)
            ranks.append(sums[w, j] / nt if nt > 0 else -np.inf)
        assert best[w] == int(np.argmax(ranks)) and rows[w] == prompt + gens[w][best[w]], (who, w)
    print(f"prefill chain {who}: positions {n}, excluded {ex}, mismatches {bad}")
    assert bad == 0 and ex <= cap * n, (who, n, ex, bad)


def check_chain(eng, o32, which, cap=0.05):
    """One chain behind the long prompt in prefill mode 1 against the teacher-forced oracle (the chain's own scheme and cap);
    rewind + mode 1 again: identical bits; mode 0 with the same prompt: the rows of a session that never heard of the mode."""
    import whisper_burn_amd as wb
    _, st, audio, R, sup, _ = tr.fixture()
    prompt, depth, eot = long_prompt(st), tr.FIX_DEPTH, st.end_of_text
    tp0 = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])

    def run(sess):
        if which.startswith("ts_"):
            bo = int(which.split("_")[2])
            T, seed, att = (0.0, 0, 0) if bo == 1 else (1.0, 1234, 2)
            tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"], temperature=T, best_of=bo, seed=seed, attempt=att)
            out = sess.decode_timestamps(wb.decode_params(st, 1, depth), tp, prompt=prompt)
            return out, sess.last_samples(bo, depth), (T, seed, att, bo)
        if which == "beam_3_5":
            p = wb.decode_params(st, 1, depth)
            out = sess.decode_timestamps_beam(p, tp0, wb.BeamParams(5, 1.0, -1.0), prompt=prompt)
            return out[:3], (sess.last_beams(depth), sess.last_beam_trace(depth)), None
        if which == "sample_3_5":
            p = wb.decode_params(st, 1, depth, mask_until_len=0)
            out = sess.decode_sample(p, wb.SampleParams(1.0, 5, 1234, 2), prompt=prompt)
            return out, sess.last_samples(5, depth), None
        if which == "prompt_greedy":
            return sess.decode_prompt(wb.decode_params(st, 1, depth, mask_until_len=0), prompt), None, None
        return sess.decode(wb.decode_params(st, 1, depth)), None, None          # the four-token prompt: the persistent launch

    def same(a, b):
        if isinstance(a, (list, tuple)) and not (a and isinstance(a[0], (int, np.integer))):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        return a == b

    mb = 1 if which in ("ts_3_1", "prompt_greedy", "greedy") else 5
    fresh = lambda: tr.fixture_session(eng, audio, 3, mb)

    def prepared(mode):
        s = fresh()
        s.set_suppress(sup)
        s.set_special_mask(st.is_special)
        if mode is not None:
            s.set_prefill(mode)
        return s

    base = prepared(None)
    r_base = run(base)
    base.close()
    s0 = prepared(0)
    r0 = run(s0)
    s0.close()
    assert same(r0[:2], r_base[:2]), which                                     # mode 0: today's rows, bit for bit
    s1 = prepared(1)
    out, extra, draw = run(s1)
    s1.rewind()
    out2, extra2, _ = run(s1)
    assert same((out, extra), (out2, extra2)), which                           # rewind + mode 1 again: identical bits
    if which.startswith("ts_"):
        T, seed, att, bo = draw
        _ts_rows_check(s1, o32, st, R, sup, prompt, out, extra, T, seed, att, bo, cap, which)
    elif which == "beam_3_5":
        rows, score, ncand = out
        beams, trace = extra
        C = tb.max_candidates(5, 1.0)
        n = ex = 0
        for w in range(3):
            enc = s1.encoder_output(w)
            cur, n_store = [tb.new_beam()], 0
            for t, step in enumerate(trace[w]):
                x = tb.oracle_rows(o32, enc, prompt, cur)
                n += 1
                stp = tb.beam_step(cur, x, R, eot, sup, None, 5, C, n_store)
                got = [dict(gen=cur[p]["gen"] + [tok], hist=cur[p]["gen"] + [tok], score=sc, parent=p) for tok, p, sc in step["beams"]]
                if tb.replay_excluded(cur, x, R, eot, sup, None, 5):
                    ex += 1
                else:
                    assert [(b["gen"][-1], b["parent"]) for b in stp["live"]] == [(b["gen"][-1], b["parent"]) for b in got], (w, t)
                    assert len(stp["newly"]) == step["finished"], (w, t)
                    for a, b in zip(stp["live"], got):
                        assert abs(a["score"] - b["score"]) <= 1e-3, (w, t, a["score"], b["score"])
                n_store = min(C, n_store + step["finished"])
                cur = got
            for c in beams[w]:
                tr.check_invariants(c["tokens"], R, eot, sup)
                _, _, _, total = tr.oracle_row_check(o32, enc, prompt + c["tokens"], len(prompt), R, eot, sup, None, 0.0, 0, 0, 0)
                assert abs(c["score"] - total) <= 1e-3 * len(c["tokens"]), (w, c, total)
            best = int(np.argmax([c["rank"] for c in beams[w]]))
            assert rows[w] == prompt + beams[w][best]["tokens"], w
        print(f"prefill chain {which}: window-steps {n}, excluded {ex}")
        assert ex <= cap * n, (which, n, ex)
    elif which == "sample_3_5":
        rows, sums, best = out
        n = ex = bad = 0
        for w in range(3):
            enc = s1.encoder_output(w)
            for j in range(5):
                gen = extra[w][j]
                a, b, c, total = sr.oracle_row_check(o32, st.is_special, enc, prompt + gen, len(prompt), 0, 1.0, 1234, w * 5 + j, 2, eot)
                n, ex, bad = n + a, ex + b, bad + c
                assert abs(sums[w, j] - total) <= 1e-3 * len(gen), (w, j, sums[w, j], total)
            assert rows[w] == prompt + extra[w][best[w]], w
        print(f"prefill chain {which}: positions {n}, excluded {ex}, mismatches {bad}")
        assert bad == 0 and ex <= cap * n, (which, n, ex, bad)
    else:                                                                      # greedy: the oracle's argmax row, ties excluded
        import torch
        full = prompt if which == "prompt_greedy" else [st.start_of_transcript, st.language, st.transcribe, st.no_timestamps]
        mask_until = 0 if which == "prompt_greedy" else wb.decode_params(st, 1, depth).mask_until_len
        maskv = np.where(np.asarray(st.is_special).astype(bool), -np.inf, 0.0)
        n = ex = 0
        for w in range(3):
            row, enc = out[w], s1.encoder_output(w)
            assert row[:len(full)] == full and len(row) > len(full), (which, w)
            logits = o32.forward_decoder(torch.tensor([row], dtype=torch.long), torch.as_tensor(enc)[None])[0].double().numpy()
            for l in range(len(full), len(row)):
                x = logits[l - 1] + (maskv if l <= mask_until else 0.0)
                top = np.sort(x)[::-1]
                n += 1
                if top[0] - top[1] > 2e-3:
                    assert int(np.argmax(x)) == row[l], (which, w, l)
                else:
                    ex += 1
        print(f"prefill chain {which}: positions {n}, excluded {ex}")
        assert ex <= cap * n, (which, n, ex)
    # mode 1 did run the pass (and mode 0 did not): the profiled (eager) repeat names its launches and gives the same rows
    from whisper_burn_amd import _lib
    lib = _lib.load()
    for mode, sess in ((1, s1), (0, prepared(0))):
        sess.rewind()
        lib.wb_profile_enable(1)
        _lib.profile_kernels(reset=True)
        again = run(sess)
        names = {k["name"].split(" ")[0] for k in _lib.profile_kernels(reset=True)}
        lib.wb_profile_enable(0)
        assert ("prefill_store" in names) == (mode == 1), (which, mode, names)
        if mode == 1:
            assert same(again[0], out), which
        sess.close()


# ---- the conditioned seek loop -----------------------------------------------------------------------------------------------------------
SEEK_MUTANTS = ("truncate_back", "sop_on_empty", "drop_timestamps", "append_tail", "no_reset")


def history_cap(max_prompt_tokens, n_text_ctx):
    return n_text_ctx // 2 - 1 if max_prompt_tokens < 0 else max_prompt_tokens


def build_prompt(history, prompt, sot_prev, cap, mut=None):
    """[sot_prev] + the last min(cap, len) tokens of history + prompt; no history section: prompt alone."""
    k = min(cap, len(history))
    tail = (history[:k] if mut == "truncate_back" else history[len(history) - k:]) if k > 0 else []
    if not tail and mut != "sop_on_empty":
        return list(prompt)
    return [sot_prev] + list(tail) + list(prompt)


def update_history(history, body, segs, R, condition, temperature, mut=None):
    """After a window (body: its generated tokens in front of end-of-text): append the tokens its segments cover, then Whisper's
    two reset rules."""
    h = list(history)
    if segs:
        cov = list(body) if mut == "append_tail" else list(body[segs[0][0]:segs[-1][1]])
        if mut == "drop_timestamps":
            cov = [t for t in cov if not tr.is_ts(R, t)]
        h += cov
    if not condition or (temperature > 0.5 and mut != "no_reset"):
        h = []
    return h


def conditioned_loop_ref(n, wlen, rate, spt, decode, R, eot, prompt, sot_prev, cap, condition, temperature, initial=(), mut=None):
    """tr.seek_loop_ref with the history rule: decode(seek, len, window_index, window_prompt) -> generated tokens.  Returns
    (segments, text, seeks, prompt lengths, prompts)."""
    seek, segs, text, seeks, plens, prompts = 0, [], [], [], [], []
    per = float(np.float32(spt)) * rate
    history = list(initial)
    while n - seek >= 400:
        ln = min(wlen, n - seek)
        wi = int(ln / per)
        wp = build_prompt(history, prompt, sot_prev, cap, mut)
        gen = list(decode(seek, ln, wi, wp))
        seeks.append(seek); plens.append(len(wp)); prompts.append(wp)
        ss, adv = tr.segments_ref(gen, R, eot, wi)
        for b, e, i0, i1 in ss:
            tt = [t for t in gen[b:e] if not tr.is_ts(R, t)]
            segs.append((seek / rate + i0 * spt, seek / rate + i1 * spt, tt))
            text += tt
        body = gen[:gen.index(eot)] if eot in gen else gen
        history = update_history(history, body, ss, R, condition, temperature, mut)
        stepn = int(round(adv * per))
        if stepn <= 0:
            stepn = ln
        seek += min(stepn, ln)
    return segs, text, seeks, plens, prompts


def scripted_loop(mut=None, condition=True, temperature=0.0, initial=(), cap=6):
    """The rule on scripted windows (no model): timestamps 100 + i, text ids < 100, eot 99; every window is 50 units long."""
    R, eot = tr.rules(100, 51), 99
    script = [[100, 5, 6, 110, 110, 7, 120, 120, 8, 9, eot],          # two closed pairs, a tail (8, 9) behind the last one
              [100, 11, 12, 13, 125, 125, 14, eot],                   # one pair, a tail
              [100, 21, 22, eot],                                     # no pair: one segment over everything
              [100, 31, 130, 130, eot]]
    calls = []

    def decode(seek, ln, wi, wp):
        calls.append(list(wp))
        return script[min(len(calls) - 1, len(script) - 1)]

    out = conditioned_loop_ref(16000 * 4, 16000, 16000, 0.02, decode, R, eot, [90, 91, 92], 95, cap, condition, temperature, initial, mut)
    return out[4]


def cond_engine():
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    dims = synth.micro_dims(64, 1, 1, tr.FIX_V, n_audio_ctx=400, n_text_ctx=64)
    return wb.Whisper.from_tensors(synth.synth_weights(dims, seed=5))


def check_conditioned_loop(eng, beam=None, seconds=20, depth=24):
    """wb_waveform_to_segments_conditioned equals the Python seek loop driving per-window decodes (mode 1 where the prompt
    carries a history section): segments, tokens, seeks and prompt lengths outright.  At least 4 windows, at least one
    truncated history (prompt length 1 + 31 + 3): 20 s of synth_audio reach it for greedy and beam 3, 16 s stop at 29."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    _, st, _, R, sup, prompt = tr.fixture()
    audio = synth.synth_audio(16000 * seconds, 3)
    p = wb.decode_params(st, 1, depth)
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    bp = wb.BeamParams(beam, 1.0, -1.0) if beam else None
    kw = dict(params=p, timestamps=tp, suppress=sup, suppress_first=None, prompt=prompt, beam=bp)
    segs, toks, n_win, win = wb.waveform_to_segments(eng, st, audio, 16000, condition_on_previous_text=True, return_windows=True, **kw)
    cap = history_cap(-1, eng.dims["n_text_ctx"])
    assert cap == 31 and n_win >= 4 and 1 + cap + len(prompt) in win["prompt_len"], (n_win, win)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)

    def decode(seek, ln, wi, wp):
        sess = wb.Session.begin(eng, audio, np.array([seek], dtype=np.int64), np.array([ln], dtype=np.int64), max_beams=beam or 1,
                                padding=p.padding)
        sess.set_suppress(sup)
        sess.set_prefill(1 if len(wp) > len(prompt) else 0)
        wtp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], wi if (R["max_ts"] < 0 or R["max_ts"] > wi) else R["max_ts"])
        rows = (sess.decode_timestamps_beam(p, wtp, bp, prompt=wp) if beam else sess.decode_timestamps(p, wtp, prompt=wp))[0]
        sess.close()
        return rows[0][len(wp):]

    rsegs, rtoks, seeks, plens, _ = conditioned_loop_ref(len(audio), wlen, 16000, 0.02, decode, R, st.end_of_text, prompt,
                                                         st.start_of_prev, cap, True, 0.0)
    assert seeks == win["seek"] and plens == win["prompt_len"] and rtoks == toks and len(rsegs) == len(segs), (seeks, win, plens)
    for a, b in zip(rsegs, segs):
        assert abs(a[0] - b["start"]) < 1e-4 and abs(a[1] - b["end"]) < 1e-4 and a[2] == b["tokens"], (a, b)
    print(f"conditioned loop (beam {beam}): seeks {seeks}, prompt lengths {plens}, segments {len(segs)}")
    # the rule "the pass whenever a history section exists, steps otherwise": the profiled (eager) repeat gives the same result
    # with one prefill_store launch per decoder layer for every window whose prompt is longer than `prompt`, and prepare
    # launches of prefill steps (len(prompt) - 1 each) for the others only
    from whisper_burn_amd import _lib
    lib = _lib.load()
    lib.wb_profile_enable(1)
    _lib.profile_kernels(reset=True)
    again = wb.waveform_to_segments(eng, st, audio, 16000, condition_on_previous_text=True, return_windows=True, **kw)
    calls = {k["name"].split(" ")[0]: k["calls"] for k in _lib.profile_kernels(reset=True)}
    off = wb.waveform_to_segments(eng, st, audio, 16000, return_windows=True, **kw)
    calls_off = {k["name"].split(" ")[0]: k["calls"] for k in _lib.profile_kernels(reset=True)}
    lib.wb_profile_enable(0)
    assert again == (segs, toks, n_win, win), beam
    n_hist = sum(1 for pl in plens if pl > len(prompt))
    assert 0 < n_hist < n_win and calls.get("prefill_store", 0) == eng.dims["n_text_layer"] * n_hist, (calls, n_hist)
    # (every window launches dec_prepare once for its first generated step; a window on steps once more per prefill step)
    assert calls.get("dec_prepare", 0) == n_win + (n_win - n_hist) * (len(prompt) - 1), (calls, n_win, n_hist)
    assert "prefill_store" not in calls_off and calls_off.get("dec_prepare", 0) == off[2] * len(prompt), calls_off
    return segs, toks, win


def check_conditioning_off(eng, depth=24, seconds=16):
    """Conditioning off and no initial prompt: every output equals waveform_to_segments'; an initial prompt with conditioning
    off lengthens window 0's prompt only."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    _, st, _, R, sup, prompt = tr.fixture()
    audio = synth.synth_audio(16000 * seconds, 3)
    kw = dict(params=wb.decode_params(st, 1, depth), timestamps=wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"]),
              suppress=sup, suppress_first=None, prompt=prompt)
    plain = wb.waveform_to_segments(eng, st, audio, 16000, **kw)
    off = wb.waveform_to_segments(eng, st, audio, 16000, return_windows=True, **kw)
    assert off[:3] == plain and off[3]["prompt_len"] == [len(prompt)] * plain[2], off[3]
    init = LONG_IDS[:5]
    ini = wb.waveform_to_segments(eng, st, audio, 16000, initial_prompt=init, return_windows=True, **kw)
    assert ini[3]["prompt_len"] == [1 + len(init) + len(prompt)] + [len(prompt)] * (ini[2] - 1), ini[3]
    return plain, ini
