"""Operator-level cases for the fused cross-attention sublayer (csrc/decode_fused.hip: launch_dec_cross_fused, the body that
also serves the persistent kernel's cross-attention role), through `wbk_cross_fused` of the kernel test harness
(whisper-burn_amd/tools/kernel_harness.cpp).  Shared by tests/test_gpu_fused_cross.py (the product's key ring of 768) and
tests/test_emu_fused_cross.py (the functional model, whose ring holds 384 keys).

The statement, per live row r of window w (C = win_C[w] keys) and head h, restated in f64:
    x      = x_in[r] + (pbias + sum_s pend[s][r])                       -> x_out[r]
    q      = (LayerNorm(x) Wq[:, head h] + bq[head h]) * scale
    p      = softmax_j (q . K[j, head h]),  j < C                       (K is cached pre-scaled)
    P[h][r] = (p V[:, head h]) Wo[head h rows, :]

The key counts sit where the block-parallel softmax can lose a key: thread t of 512 owns keys t + 512 i, the denominator's
lanes own keys l + 64 i, and the ring holds `ring` keys per pass.  Every count comes in two data variants:
  * `uniform`: scores within +-0.3 of each other and V with mean 0.5 -- a key missing from the denominator moves every output
    by about 1 / C of its value, orders of magnitude above the bound;
  * `peak`: one score of about +100 on a boundary key (C - 1, 63, 64, 511, 512, 767, 768, ...; a different one per head and
    row), every other score near 0 -- missing from the maximum it overflows expf, missing from the probabilities or the
    denominator it takes the whole output with it.

Bound: the attention-family scheme of tests/kernel_cases.py (run_attn).  c = 4 x the largest error of the plain f32 NumPy
evaluation of the same statement against f64, in units of a (row, head)'s base, measured over the case; an element may miss the
f64 value by c base + 2^-24 max|P[h][r]|.  base = kernel_refs.attention_base(q, K, V) x 64 max|Wo[head rows]|: the scale of the
f32 error of the attention output carried through the 64-term out-projection.  x_out is a chain of KSp + 1 f32 additions:
(KSp + 1) 2^-24 (|x_in| + |pbias| + sum |pend|) elementwise.

Poison and canaries as in kernel_cases.py: cached rows outside every window, the columns past K | V in a cached row, rows of
x_in / pend past the live ones are NaN; P and x_out carry guard bands and must keep their canary outside the live rows."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_cases as kc  # noqa: E402
import kernel_refs as R  # noqa: E402

Cross = kc._struct("Cross", [
    ("x_in pend pbias x_out ln_g ln_b Wq bq ckv win_row0 win_C row_win Wo P", kc.Buf),
    ("S W d n_head KSp ldkv koff n_pass n_rows ln_inside", C.c_int64), ("ln_eps scale", C.c_double)])

PROD_RING, EMU_RING = 768, 384
# key counts per ring and pass count (the issue's lists)
KEYS = {(PROD_RING, 1): (1, 63, 64, 65, 511, 512, 513, 750, 768),
        (PROD_RING, 2): (769, 1023, 1024, 1025, 1500, 1536),
        (EMU_RING, 1): (383, 384),
        (EMU_RING, 2): (385, 511, 512, 513, 745, 768)}
BOUNDARY = (63, 64, 383, 384, 511, 512, 767, 768, 1023, 1024, 1535)
G = kc.G

_LIBS = {}


def load(path):
    if path not in _LIBS:
        lib = C.CDLL(path)
        lib.wbk_cross_fused.restype = C.c_int
        lib.wbk_cross_fused.argtypes = [C.c_void_p]
        lib.wbk_cross_fused_ring.restype = C.c_int
        lib.wbk_cross_fused_ring.argtypes = []
        _LIBS[path] = lib
    return _LIBS[path]


def cases(ring):
    """Every listed key count x d in (128, 384) x rows in (1, 3) x both variants.  With three rows, the other two rows take the
    next two key counts of the same list: different C per row, one pass count per launch."""
    out = []
    for n_pass in (1, 2):
        ks = KEYS[(ring, n_pass)]
        for i, c0 in enumerate(ks):
            for d in (128, 384):
                for rows in (1, 3):
                    cs = tuple(ks[(i + j) % len(ks)] for j in range(min(rows, len(ks))))
                    cs += tuple(c0 // 3 + 5 + j for j in range(rows - len(cs)))       # (a list shorter than the rows)
                    for variant in ("uniform", "peak"):
                        out.append(dict(id=f"ring{ring}_np{n_pass}_C{c0}_d{d}_r{rows}_{variant}", ring=ring, n_pass=n_pass, Cs=cs,
                                        d=d, rows=rows, variant=variant))
    return out


def peak_key(Cn, r, h):
    cand = [Cn - 1] + [b for b in BOUNDARY if b < Cn - 1]
    return cand[(r + h) % len(cand)]


def _ln(x, g, b, eps, inside, dtype):
    return R.layernorm_ref(x[None], g, b, eps, inside, dtype=dtype)[0].astype(dtype)


def _statement(x, g, b, eps, inside, Wq, bq, scale, K, V, Wo, H, dtype):
    """(q [H][64], out [H][d]) of one row in `dtype`."""
    f = dtype
    xn = _ln(x.astype(f), g.astype(f), b.astype(f), eps, inside, f)
    qs, outs = [], []
    for h in range(H):
        hs = slice(64 * h, 64 * h + 64)
        q = ((xn @ Wq[:, hs].astype(f) + bq[hs].astype(f)) * f(np.float32(scale))).astype(f)
        s = K[:, hs].astype(f) @ q
        p = np.exp(s - s.max())
        att = (p @ V[:, hs].astype(f)) / p.sum(dtype=f)
        qs.append(q)
        outs.append((att.astype(f) @ Wo[hs, :].astype(f)).astype(f))
    return np.stack(qs).astype(np.float64), np.stack(outs).astype(np.float64)


def run(lib, c):
    """Runs one case through the harness and compares.  Returns dict(ratio=worst error / bound, c_measured=...)."""
    assert lib.wbk_cross_fused_ring() == c["ring"], "the library's key ring is not the one this case was made for"
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 104729 + 11)
    d, rows, Cs, n_pass = c["d"], c["rows"], c["Cs"], c["n_pass"]
    H, S, W, KSp = d // 64, rows + 1, rows, H_planes(d)
    eps, inside, scale = 1e-5, 1, 0.125
    x_in = kc.nan32(S * d).reshape(S, d)
    pend = kc.nan32(KSp * S * d).reshape(KSp, S, d)
    x_in[:rows] = kc.values(rng, (rows, d), 1.0)
    pend[:, :rows] = kc.values(rng, (KSp, rows, d), 0.3)
    pbias = kc.values(rng, d, 0.1)
    g, b = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32), kc.values(rng, d, 0.1)
    Wq, bq = kc.values(rng, (d, d), 1.0 / np.sqrt(d)), kc.values(rng, d, 0.1)
    Wo = kc.values(rng, (d, d), 1.0 / np.sqrt(d))
    # cached rows: window w at row0[w], poisoned rows between the windows; K | V | 4 poisoned columns per row
    ldkv, koff = 2 * d + 4, 4
    row0, nr = [], 3
    for Cn in Cs:
        row0.append(nr)
        nr += Cn + 2 + (Cn % 2)
    ckv = kc.nan32(G + koff + nr * ldkv + G)
    body = ckv[G + koff:G + koff + nr * ldkv].reshape(nr, ldkv)
    # rows take their windows in reverse order: row r belongs to window rows - 1 - r
    row_win = np.array([rows - 1 - r for r in range(rows)], dtype=np.int32)
    xs = (x_in[:rows].astype(np.float64) + (pbias.astype(np.float64) + pend[:, :rows].astype(np.float64).sum(axis=0)))
    x32 = x_in[:rows].copy()
    acc = np.broadcast_to(pbias, (rows, d)).copy()
    for s in range(KSp):
        acc = acc + pend[s, :rows]
    x32 = x32 + acc                                                 # the kernel's own f32 order: x + (bias + planes ascending)
    Ks, Vs = {}, {}
    for w, Cn in enumerate(Cs):
        r = int(np.nonzero(row_win == w)[0][0])
        K = kc.values(rng, (Cn, d), 0.02)
        V = kc.values(rng, (Cn, d), 1.0)
        if c["variant"] == "uniform":
            V = (V + np.float32(0.5)).astype(np.float32)
        else:
            # the query of (row, head) from the f32 row the kernel normalises; the peak key's K row is q * 100 / |q|^2
            q64, _ = _statement(x32[r], g, b, eps, inside, Wq, bq, scale, K, V, Wo, H, np.float64)
            for h in range(H):
                hs = slice(64 * h, 64 * h + 64)
                K[peak_key(Cn, r, h), hs] = (q64[h] * (100.0 / float(q64[h] @ q64[h]))).astype(np.float32)
        body[row0[w]:row0[w] + Cn, :d] = K
        body[row0[w]:row0[w] + Cn, d:2 * d] = V
        Ks[w], Vs[w] = K, V
    p_total = G + H * S * d + G
    P = kc.canary32(p_total)
    xo = kc.canary32(G + S * d + G)
    r0a, wca = np.array(row0, dtype=np.int32), np.array(Cs, dtype=np.int32)
    t = Cross()
    t.x_in, t.pend, t.pbias, t.x_out = kc.buf(x_in), kc.buf(pend), kc.buf(pbias), kc.buf(xo, G)
    t.ln_g, t.ln_b, t.Wq, t.bq, t.ckv = kc.buf(g), kc.buf(b), kc.buf(Wq), kc.buf(bq), kc.buf(ckv, G)
    t.win_row0, t.win_C, t.row_win, t.Wo, t.P = kc.buf(r0a), kc.buf(wca), kc.buf(row_win), kc.buf(Wo), kc.buf(P, G)
    t.S, t.W, t.d, t.n_head, t.KSp, t.ldkv, t.koff, t.n_pass, t.n_rows, t.ln_inside = S, W, d, H, KSp, ldkv, koff, n_pass, rows, inside
    t.ln_eps, t.scale = eps, scale
    st = kc._call(lib.wbk_cross_fused, t)
    assert st == 0, f"harness status {st}"

    # ---- x_out: the folded stream
    got_x = xo[G:G + S * d].reshape(S, d)
    mag = np.abs(x_in[:rows]).astype(np.float64) + np.abs(pbias) + np.abs(pend[:, :rows]).astype(np.float64).sum(axis=0)
    errx = np.abs(got_x[:rows].astype(np.float64) - xs)
    assert np.isfinite(got_x[:rows]).all() and (errx <= (KSp + 1) * R.U32 * mag).all(), f"x_out: worst error {errx.max():.3g}"
    wx = np.zeros(xo.shape, dtype=bool)
    wx[G:G + rows * d] = True
    kc.assert_untouched(xo, wx, kc.CANARY32, "x_out")

    # ---- the planes
    got = P[G:G + H * S * d].reshape(H, S, d)
    items, measured_c = [], 0.0
    for r in range(rows):
        w = int(row_win[r])
        x_row = got_x[r]                                            # what the kernel normalises (checked above)
        q64, ref = _statement(x_row, g, b, eps, inside, Wq, bq, scale, Ks[w], Vs[w], Wo, H, np.float64)
        _, f32 = _statement(x_row, g, b, eps, inside, Wq, bq, scale, Ks[w], Vs[w], Wo, H, np.float32)
        for h in range(H):
            hs = slice(64 * h, 64 * h + 64)
            base = R.attention_base(q64[h][None], Ks[w][:, hs], Vs[w][:, hs], 1.0) * 64.0 * float(np.abs(Wo[hs]).max())
            measured_c = max(measured_c, float(np.abs(f32[h] - ref[h]).max()) / base)
            items.append((r, h, ref[h], base))
    cc = 4.0 * measured_c
    ratio, worst = 0.0, None
    for r, h, ref, base in items:
        bound = cc * base + R.U32 * float(np.abs(ref).max())
        o = got[h, r].astype(np.float64)
        assert np.isfinite(o).all(), f"non-finite output, row {r} head {h} (C = {Cs[int(row_win[r])]})"
        e = float(np.abs(o - ref).max()) / bound
        if e > ratio:
            ratio, worst = e, dict(row=r, head=h, C=Cs[int(row_win[r])], err=e * bound, bound=bound)
    wp = np.zeros(P.shape, dtype=bool)
    for h in range(H):
        wp[G + (h * S) * d:G + (h * S + rows) * d] = True
    info = dict(id=c["id"], ratio=ratio, c_measured=measured_c, worst=worst)
    assert ratio <= 1.0, f"worst error / bound {ratio:.3g} at {worst}"
    kc.assert_untouched(P, wp, kc.CANARY32, "P")
    return info


def H_planes(d):
    """Pending planes folded by the prologue: one per head of the self-attention sublayer in front."""
    return d // 64


def main(argv):
    """`python fused_cross_cases.py LIB RING [ID ...]`: runs the cases (default: all of the ring) in THIS process -- the library and
    nothing else of the engine loaded -- and prints one `KCASE <json>` line per case."""
    import json
    lib, ring = load(argv[0]), int(argv[1])
    for c in cases(ring):
        if argv[2:] and c["id"] not in argv[2:]:
            continue
        try:
            info = dict(run(lib, c), ok=True)
        except AssertionError as e:
            info = dict(id=c["id"], ok=False, msg=str(e)[:600])
        print("KCASE " + json.dumps(info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
