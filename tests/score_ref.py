"""Token scoring restated in NumPy (the checker side of csrc/score.hip and wb_logprob_gather), written from the contract in
csrc/kernels.h -- not from the kernel:

    logits = h E^T                      [R][V]
    own    = logits + mask on the rows with row_masked, logits elsewhere
    lse[r]      = log sum_v exp(own[r][v])
    logprob[r]  = own[r][target[r]] - lse[r]                    (NaN when target[r] = -1)
    probe_lp[p] = logits[row_p][id_p] - log sum_v exp(logits[row_p][v])      (always unmasked)

plus the error bound the comparisons use, the operator cases (shapes, targets, masks, probes) shared by the GPU test and the
functional-model test, and the NumPy mutants the bound must reject."""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
BM, BN = 32, 128          # csrc/kernels.h: SCORE_BM, SCORE_BN

# (R, d, V, splits): the smallest shapes at which the tiling can go wrong (0 = auto)
SHAPES = [(1, 64, 263, 0), (5, 1280, 263, 1), (33, 128, 1031, 3), (130, 384, 1031, 0)]


def n_splits(R, V, requested=0):
    """score_splits (score.hip): requested, or enough splits for ~512 blocks; at most one per 128-column tile."""
    tiles, row_tiles = -(-V // BN), -(-R // BM)
    vs = requested if requested > 0 else -(-512 // row_tiles)
    return max(1, min(vs, tiles))


def split_ranges(V, vs):
    """Columns [lo, hi) of every split: split s owns the 128-column tiles [s T / vs, (s + 1) T / vs)."""
    tiles = -(-V // BN)
    return [(BN * (s * tiles // vs), min(V, BN * ((s + 1) * tiles // vs))) for s in range(vs)]


def _lse(x, axis=-1):
    m = x.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0).astype(x.dtype)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True, dtype=x.dtype))).squeeze(axis)


def score_ref(h, E, mask=None, row_masked=None, target=None, probes=None, dtype=np.float64, mutant=None, vs=1, ldv=None):
    """(logprob [R], lse [R], probe_lp [n_probe]) in `dtype`.  mutant: None, or one of
    "target_shift" (the target of row r read from row r + 1), "mask_ignored", "pad_zeros" (columns [V, ldv) enter the sums
    as zero logits), "no_rescale" (the splits' sums added without rescaling to the common max)."""
    h, E = np.asarray(h, dtype=dtype), np.asarray(E, dtype=dtype)
    R, V = h.shape[0], E.shape[0]
    logits = h @ E.T
    own = logits.copy()
    if mask is not None and mutant != "mask_ignored":
        rm = np.asarray(row_masked).astype(bool)
        own[rm] = own[rm] + np.asarray(mask, dtype=dtype)[None, :]

    def lse_of(x):
        if mutant == "pad_zeros":
            x = np.concatenate([x, np.zeros((R, (ldv or -(-V // 64) * 64) - V), dtype=dtype)], axis=1)
        if mutant == "no_rescale":
            parts = [x[:, lo:hi] for lo, hi in split_ranges(V, vs)]
            ms = [p.max(axis=1) for p in parts]
            ss = [np.where(np.isfinite(m), np.exp(p - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(axis=1), 0.0)
                  for p, m in zip(parts, ms)]
            with np.errstate(divide="ignore"):
                return (np.max(ms, axis=0) + np.log(np.sum(ss, axis=0))).astype(dtype)
        return _lse(x)

    lse = lse_of(own)
    logprob = np.full(R, np.nan, dtype=dtype)
    if target is not None:
        t = np.asarray(target)
        if mutant == "target_shift":
            t = np.roll(t, -1) if R > 1 else np.where(t >= 0, (t + 1) % V, t)
        ok = t >= 0
        with np.errstate(invalid="ignore"):
            logprob[ok] = own[np.nonzero(ok)[0], t[ok]] - lse[ok]
    pr = np.asarray(probes if probes is not None else [], dtype=np.int64).reshape(-1, 2)
    lse_u = lse_of(logits)
    probe_lp = (logits[pr[:, 0], pr[:, 1]] - lse_u[pr[:, 0]]).astype(dtype)
    return logprob, lse, probe_lp


def logit_bound_rows(h, E):
    """2 (d + 4) 2^-24 max_v sum_k |h_k| |E_vk| per row: the logit error of an f32 accumulation in any order, once for the
    picked logit and once through the 1-Lipschitz log-sum-exp."""
    h, E = np.abs(np.asarray(h, dtype=np.float64)), np.abs(np.asarray(E, dtype=np.float64))
    return 2.0 * (h.shape[1] + 4) * U32 * (h @ E.T).max(axis=1)


def absdiff(a, b):
    """|a - b| with equal infinities / NaNs at the same place counting as 0 and a one-sided NaN / inf as inf."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        dlt = np.abs(a - b)
    return np.where(same, 0.0, np.where(np.isnan(dlt), np.inf, dlt))


def bounds(case):
    """(ref64 triple, bound triple) of a case: the f64 statement and the per-element bound."""
    a = dict(mask=case["mask"], row_masked=case["row_masked"], target=case["target"], probes=case["probes"])
    ref = score_ref(case["h"], case["E"], **a)
    f32 = score_ref(case["h"], case["E"], dtype=np.float32, **a)
    rows = logit_bound_rows(case["h"], case["E"])
    pr = np.asarray(case["probes"] if case["probes"] is not None else [], dtype=np.int64).reshape(-1, 2)
    base = (rows, rows, rows[pr[:, 0]])
    return ref, tuple(b + 4.0 * absdiff(x, y) for b, x, y in zip(base, f32, ref))


def worst_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the three outputs (a NaN where the reference has a number counts as inf)."""
    w = 0.0
    for g, r, b in zip(got, ref, bound):
        if len(r):
            w = max(w, float((absdiff(g, r) / b).max()))
    return w


def make_cases(shape, seed=0):
    """The calls of one shape: every mask kind the kernel distinguishes, targets at column 0, V - 1, the first and the last
    column of a split and -1, duplicate probes, a probe at V - 1, masked and unmasked rows in one call.  Logits have unit
    scale whatever d is (E ~ N(0, 1 / d), h ~ N(0, 1): a final-LayerNorm row)."""
    R, d, V, req = shape
    vs = n_splits(R, V, req)
    g = np.random.default_rng(1000 * R + d + V + seed)
    h = g.standard_normal((R, d)).astype(np.float32)
    E = (g.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)
    rng = split_ranges(V, vs)
    edge = [0, V - 1, -1] + [c for lo, hi in rng for c in (lo, hi - 1)]
    out = []
    kinds = ["none", "tail", "single"] + (["split"] if vs > 1 else [])
    for kind in kinds:
        mask = None
        keep = np.ones(V, dtype=bool)
        if kind == "tail":                       # the synthetic vocabularies' specials: the last 16 ids
            keep[V - 16:] = False
        elif kind == "split":                    # every column of the middle split (and one more id)
            lo, hi = rng[len(rng) // 2]
            keep[lo:hi] = False
            keep[3] = False
        elif kind == "single":
            keep[:] = False
            keep[V // 2 + 1] = True
        if kind != "none":
            mask = np.where(keep, 0.0, -np.inf).astype(np.float32)
        # R = 1 cannot hold every target in one call: one call per edge column there
        n_calls = len(edge) if R == 1 else 1
        for c in range(n_calls):
            row_masked = None
            if mask is not None:
                row_masked = (np.arange(R) % 2 == 0).astype(np.uint8) if R > 1 else np.ones(1, dtype=np.uint8)
            target = np.array([edge[(r + c) % len(edge)] for r in range(R)], dtype=np.int32)
            if R > len(edge):
                target[len(edge):] = g.integers(0, V, R - len(edge))
            if mask is not None:                  # a masked row's target is an id the mask keeps (a finite log-prob) ...
                kept = np.nonzero(keep)[0]
                for r in range(R):
                    if row_masked[r] and target[r] >= 0 and not keep[target[r]]:
                        target[r] = kept[(r * 7) % len(kept)]
                if kind == "tail" and R > 1:      # ... but one: a masked target is -inf exactly
                    target[2] = V - 1
            probes = [(R - 1, V - 1), (0, 5), (0, 5), (R // 2, rng[-1][0])]
            probes += [(r, int(g.integers(0, V))) for r in range(0, R, 3)]
            out.append(dict(name=f"{R}x{d}x{V}/s{req}/{kind}/{c}", h=h, E=E, V=V, vs=vs, req=req, mask=mask,
                            row_masked=row_masked, target=target, probes=probes, kind=kind))
    return out


# ---- the hook on guarded arrays ------------------------------------------------------------------------------------------------
CANARY = np.float32(-7777.25)


def run_hook(case, device=0):
    """wb_logprob_gather on the case: every input sits inside a larger NaN-poisoned array (the hook must read exactly its
    contract), every output between two canary bands (it must write exactly R / n_probe floats).  Returns the triple."""
    import ctypes as C

    from whisper_burn_amd import _lib
    lib = _lib.load()
    G = 16

    def guarded_in(a, dtype, poison):
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        big = np.full(a.size + 2 * G, poison, dtype=dtype)
        big[G:G + a.size] = a
        return big, big[G:G + a.size]

    def guarded_out(n):
        big = np.full(n + 2 * G, CANARY, dtype=np.float32)
        return big, big[G:G + n]

    def ptr(view, ty):
        return C.cast(view.ctypes.data, ty) if view is not None else None

    R, d = case["h"].shape
    V = case["V"]
    keep = []
    _, h = guarded_in(case["h"], np.float32, np.nan); keep.append(_)
    _, E = guarded_in(case["E"], np.float32, np.nan); keep.append(_)
    mask = rm = None
    if case["mask"] is not None:
        _, mask = guarded_in(case["mask"], np.float32, np.nan); keep.append(_)
        _, rm = guarded_in(case["row_masked"], np.uint8, 1); keep.append(_)
    _, tg = guarded_in(case["target"], np.int32, 2 ** 30); keep.append(_)
    pr = np.asarray(case["probes"], dtype=np.int32).reshape(-1, 2)
    _, prow = guarded_in(pr[:, 0], np.int32, 2 ** 30); keep.append(_)
    _, pid = guarded_in(pr[:, 1], np.int32, 2 ** 30); keep.append(_)
    outs = [guarded_out(R), guarded_out(R), guarded_out(len(pr))]
    rc = lib.wb_logprob_gather(device, ptr(h, _lib.c_float_p), R, d, ptr(E, _lib.c_float_p), V, ptr(mask, _lib.c_float_p),
                               ptr(rm, _lib.c_uint8_p), ptr(tg, _lib.c_int32_p), ptr(prow, _lib.c_int32_p),
                               ptr(pid, _lib.c_int32_p), len(pr), case["req"], ptr(outs[0][1], _lib.c_float_p),
                               ptr(outs[1][1], _lib.c_float_p), ptr(outs[2][1], _lib.c_float_p))
    _lib.check(rc)
    for big, view in outs:
        assert (big[:G] == CANARY).all() and (big[G + view.size:] == CANARY).all(), "the hook wrote outside an output array"
        assert not (view == CANARY).any(), "the hook left an output element unwritten"
    return tuple(view.copy() for _, view in outs)


def check_hook_case(case, record=None):
    """Run the hook on a case and hold it to the bound; returns the worst error / bound."""
    got = run_hook(case)
    ref, bound = bounds(case)
    ratio = worst_ratio(got, ref, bound)
    print(f"score kernel {case['name']}: vs {case['vs']} worst error / bound {ratio:.3f}")
    if record is not None:
        record(case["name"], ratio)
    assert ratio <= 1.0, (case["name"], ratio)
    for g in got[1:]:
        assert not np.isnan(g).any(), case["name"]                      # (lse, probes: never NaN; logprob: only without a target)
    assert np.array_equal(np.isnan(got[0]), case["target"] < 0), case["name"]
    if case["kind"] == "single":                                        # one id left: its log-prob is 0 up to the bound
        rm = case["row_masked"].astype(bool) & (case["target"] >= 0)
        assert (np.abs(got[0][rm]) <= bound[0][rm]).all() and (rm.any() or case["h"].shape[0] == 1), case["name"]
    return ratio


def check_hook_nan_row(shape=(33, 128, 1031, 3)):
    """A NaN in one row of h (a broken final-LayerNorm row) comes out as NaN in THAT row's lse, log-prob and probes -- never
    as a finite-looking number -- and leaves every other row's bits alone."""
    case = dict(make_cases(shape)[1])                    # masked and unmasked rows
    clean = run_hook(case)
    h = case["h"].copy()
    bad = (1, 4)                                         # an unmasked and a masked row
    h[1, 7] = np.nan
    h[4, h.shape[1] - 3] = np.nan
    case["h"] = h
    got = run_hook(case)
    pr = np.asarray(case["probes"]).reshape(-1, 2)
    for r in bad:
        assert np.isnan(got[1][r]) and (case["target"][r] < 0 or np.isnan(got[0][r])), r
    ok = ~np.isin(np.arange(h.shape[0]), bad)
    assert np.array_equal(got[0][ok], clean[0][ok], equal_nan=True) and np.array_equal(got[1][ok], clean[1][ok])
    pbad = np.isin(pr[:, 0], bad)
    assert np.isnan(got[2][pbad]).all() and np.array_equal(got[2][~pbad], clean[2][~pbad])


# ---- the model entries against the oracle --------------------------------------------------------------------------------------
def oracle_scores(oracle, is_special, enc, row, mask_until_len=5, probe_ids=None, probe_pos=0):
    """(token_logprobs [len] with NaN at entry 0, probe_logprobs [n_probe]) of one row from ONE stateless forward of the oracle
    (OracleWhisper.forward_decoder + oracle.model.log_softmax), in the oracle's dtype: entry l is the log-prob of row[l] at
    position l - 1, under the special mask while l <= mask_until_len (transcribe.rs:271-275); probes are unmasked."""
    import torch

    from oracle.model import log_softmax
    dt = oracle.dtype if hasattr(oracle, "dtype") else torch.float32
    toks = torch.tensor([list(row)], dtype=torch.long)
    enc_t = torch.as_tensor(np.asarray(enc)).to(dt)
    logits = oracle.forward_decoder(toks, enc_t[None])[0]
    maskv = torch.tensor(np.where(np.asarray(is_special).astype(bool), -np.inf, 0.0), dtype=logits.dtype)
    out = np.full(len(row), np.nan, dtype=np.float64)
    for l in range(1, len(row)):
        lg = logits[l - 1]
        if mask_until_len > 0 and l <= mask_until_len:
            lg = lg + maskv
        out[l] = float(log_softmax(lg, 0)[row[l]])
    probes = np.zeros(0)
    if probe_ids is not None:
        probes = log_softmax(logits[probe_pos], 0)[torch.as_tensor(np.asarray(probe_ids), dtype=torch.long)].double().numpy()
    return out, probes
