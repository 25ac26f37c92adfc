"""Operator-level cases for the fused self-attention sublayer at d = 384 with the count of QKV weight rounds held in registers
named (csrc/decode_fused.hip: launch_dec_attn_fused_rounds, the body that also serves the persistent kernel's self-attention
role), through `wbk_attn_fused` of the kernel test harness (whisper-burn_amd/tools/kernel_harness.cpp).  Shared by
tests/test_gpu_attn_rounds_kernel.py and tests/test_emu_attn_rounds.py (the functional model).

Every case runs TWICE on the same inputs, with 2 and with 4 register rounds.  Both sequences multiply the same operands in the
same order (rounds 0 .. 5), so the plane, the new K / V cache rows and x_out must agree bit for bit; each run is also compared
with the f64 restatement, per live row r (length len including the new token) and head h:
    x        = x_in[r] + (pbias + sum_s pend[s][r])                     -> x_out[r]
    q, k, v  = LayerNorm(x) Wqkv[:, {q, k, v} of head h] + bqkv;  q, k *= scale
    K, V     = cached rows of positions 0 .. len - 2 (through the position table) followed by (k, v) -> cache row tabs[r][len - 1]
    P[h][r]  = (softmax_j (q . K[j]) V) Wo[head h rows, :]

Lengths: 1 (no cached key), 2 (one), 100, 129 (a full first tile of 128 cached positions) -- the issue's list -- and 130 (one
position in the first tail tile), with 1 and 3 rows; with 3 rows the other two take the next lengths of the list.  V has mean
0.5, so a position missing from the sum moves every output by about 1 / len of its value.

Bounds.  Planes: the attention-family scheme of tests/kernel_cases.py as tests/fused_cross_cases.py applies it to a sublayer:
c = 4 x the largest error of the plain f32 NumPy evaluation of the statement against f64 in units of a (row, head)'s base,
base = kernel_refs.attention_base(q, K, V) x 64 max|Wo[head rows]|; an element may miss f64 by c base + 2^-24 max|P[h][r]|.
x_out: a chain of KSp + 1 f32 additions, (KSp + 1) 2^-24 (|x_in| + |pbias| + sum |pend|) elementwise.  New cache rows: a
LayerNorm followed by a d-term f32 dot product in some order -- (d + 2) 2^-24 (|xn| |W| + |b|) for the product (the a-priori
bound of a d-term sum and the bias addition) plus the LayerNorm's error carried through |W|, the LayerNorm error taken as in
kernel_cases.run_norm (4 x the f32 NumPy evaluation's error in units of kernel_refs.layernorm_base); all times scale for K.

Poison and canaries as in kernel_cases.py: rows of x_in / pend past the live ones, the columns of Wqkv past 3 d and every cache
row no position points to are NaN; table entries past a row's length point to such a NaN row; the new tokens' cache rows, P and
x_out start as canaries; P and x_out carry guard bands and must keep their canary outside the live rows."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_cases as kc  # noqa: E402
import kernel_refs as R  # noqa: E402

Attn = kc._struct("Attn", [
    ("x_in pend pbias x_out ln_g ln_b Wqkv bqkv Kc Vc tabs lens Wo P", kc.Buf),
    ("S d n_head KSp ldqkv Lmax n_slots n_rows ln_inside n_reg", C.c_int64), ("ln_eps scale", C.c_double)])

D = 384
LENS = (1, 2, 100, 129, 130)
ROWS = (1, 3)
G = kc.G

_LIBS = {}


def load(path):
    if path not in _LIBS:
        lib = C.CDLL(path)
        lib.wbk_attn_fused.restype = C.c_int
        lib.wbk_attn_fused.argtypes = [C.c_void_p]
        _LIBS[path] = lib
    return _LIBS[path]


def cases():
    out = []
    for i, l0 in enumerate(LENS):
        for rows in ROWS:
            ls = tuple(LENS[(i + j) % len(LENS)] for j in range(rows))
            out.append(dict(id=f"len{l0}_r{rows}", lens=ls, rows=rows))
    return out


def _statement(x, g, b, eps, inside, Wqkv, bqkv, scale, Kp, Vp, Wo, f):
    """One row in dtype f: (xn [d], q, k, v [H][64], planes [H][d]); Kp / Vp [npast][d] are the cached rows in position order."""
    d = x.shape[0]
    H = d // 64
    xn = R.layernorm_ref(x[None].astype(f), g, b, eps, inside, dtype=f)[0].astype(f)
    s = f(np.float32(scale))
    qs, ks, vs, outs = [], [], [], []
    for h in range(H):
        hs = slice(64 * h, 64 * h + 64)
        q, k, v = ((xn @ Wqkv[:, seg * d + 64 * h:seg * d + 64 * h + 64].astype(f) + bqkv[seg * d + 64 * h:seg * d + 64 * h + 64].astype(f)).astype(f)
                   for seg in range(3))
        q, k = (q * s).astype(f), (k * s).astype(f)
        K = np.concatenate([Kp[:, hs].astype(f), k[None]])
        V = np.concatenate([Vp[:, hs].astype(f), v[None]])
        sc = K @ q
        p = np.exp(sc - sc.max())
        att = ((p @ V) / p.sum(dtype=f)).astype(f)
        qs.append(q); ks.append(k); vs.append(v)
        outs.append((att @ Wo[hs, :].astype(f)).astype(f))
    return xn.astype(np.float64), np.stack(qs).astype(np.float64), np.stack(ks).astype(np.float64), np.stack(vs).astype(np.float64), \
        np.stack(outs).astype(np.float64)


def run(lib, c):
    """Runs one case with 2 and with 4 register rounds and compares.  Returns dict(id, ratio = worst error / bound over both)."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 7919 + 5)
    d, rows, lens = D, c["rows"], c["lens"]
    H, S, KSp = d // 64, rows + 1, 4 * d // 64                      # the pending planes of an MLP sublayer in front
    eps, inside, scale = 1e-5, 1, 0.35355339059327373               # 64 ** -0.25
    Lmax = max(LENS) + 6
    x_in = kc.nan32(S * d).reshape(S, d)
    pend = kc.nan32(KSp * S * d).reshape(KSp, S, d)
    x_in[:rows] = kc.values(rng, (rows, d), 1.0)
    pend[:, :rows] = kc.values(rng, (KSp, rows, d), 0.1)
    pbias = kc.values(rng, d, 0.1)
    g, b = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32), kc.values(rng, d, 0.1)
    ldqkv = 3 * d + 8
    Wqkv = kc.nan32(d * ldqkv).reshape(d, ldqkv)
    Wqkv[:, :3 * d] = kc.values(rng, (d, 3 * d), 1.0 / np.sqrt(d))
    bqkv = kc.values(rng, 3 * d, 0.1)
    Wo = kc.values(rng, (d, d), 1.0 / np.sqrt(d))
    # cache: every position of every row gets its own row, in a shuffled order; the last row stays NaN and takes the table's
    # entries past each length; rows no position points to stay NaN
    n_pos = sum(lens)
    NS = n_pos + 5
    order = rng.permutation(NS - 1)[:n_pos]
    Kc0, Vc0 = kc.nan32(NS * d).reshape(NS, d), kc.nan32(NS * d).reshape(NS, d)
    tabs = np.full((S, Lmax), NS - 1, dtype=np.int32)
    Kp, Vp, new_slot, o = [], [], [], 0
    for r in range(rows):
        sl = order[o:o + lens[r]]
        o += lens[r]
        tabs[r, :lens[r]] = sl
        K = kc.values(rng, (lens[r] - 1, d), 0.3)
        V = (kc.values(rng, (lens[r] - 1, d), 1.0) + np.float32(0.5)).astype(np.float32)
        Kc0[sl[:-1]], Vc0[sl[:-1]] = K, V
        Kc0[sl[-1]], Vc0[sl[-1]] = kc.canary32(d), kc.canary32(d)
        Kp.append(K); Vp.append(V); new_slot.append(int(sl[-1]))
    lens_a = np.array(lens, dtype=np.int32)

    runs = {}
    for n_reg in (2, 4):
        Kc, Vc = Kc0.copy(), Vc0.copy()
        P = kc.canary32(G + H * S * d + G)
        xo = kc.canary32(G + S * d + G)
        t = Attn()
        t.x_in, t.pend, t.pbias, t.x_out = kc.buf(x_in), kc.buf(pend), kc.buf(pbias), kc.buf(xo, G)
        t.ln_g, t.ln_b, t.Wqkv, t.bqkv = kc.buf(g), kc.buf(b), kc.buf(Wqkv), kc.buf(bqkv)
        t.Kc, t.Vc, t.tabs, t.lens, t.Wo, t.P = kc.buf(Kc), kc.buf(Vc), kc.buf(tabs), kc.buf(lens_a), kc.buf(Wo), kc.buf(P, G)
        t.S, t.d, t.n_head, t.KSp, t.ldqkv, t.Lmax, t.n_slots, t.n_rows, t.ln_inside, t.n_reg = S, d, H, KSp, ldqkv, Lmax, NS, rows, inside, n_reg
        t.ln_eps, t.scale = eps, scale
        st = kc._call(lib.wbk_attn_fused, t)
        assert st == 0, f"harness status {st} (register rounds {n_reg})"
        runs[n_reg] = (P, xo, Kc, Vc)

    # ---- 2 against 4 register rounds: the same bits everywhere (canaries, NaN rows and all)
    for name, a2, a4 in zip(("P", "x_out", "Kc", "Vc"), runs[2], runs[4]):
        diff = np.nonzero(a2.view(np.uint32).ravel() != a4.view(np.uint32).ravel())[0]
        assert diff.size == 0, f"{name}: {diff.size} words differ between 2 and 4 register rounds, first at {int(diff[0])}"

    # ---- each against the f64 restatement (the arrays are bit-equal, but a failure names its run)
    xs = x_in[:rows].astype(np.float64) + (pbias.astype(np.float64) + pend[:, :rows].astype(np.float64).sum(axis=0))
    mag = np.abs(x_in[:rows]).astype(np.float64) + np.abs(pbias) + np.abs(pend[:, :rows]).astype(np.float64).sum(axis=0)
    W3 = Wqkv[:, :3 * d]
    ratio, worst = 0.0, None
    for n_reg, (P, xo, Kc, Vc) in runs.items():
        got_x = xo[G:G + S * d].reshape(S, d)
        errx = np.abs(got_x[:rows].astype(np.float64) - xs)
        assert np.isfinite(got_x[:rows]).all() and (errx <= (KSp + 1) * R.U32 * mag).all(), f"x_out ({n_reg} rounds): worst error {errx.max():.3g}"
        wx = np.zeros(xo.shape, dtype=bool)
        wx[G:G + rows * d] = True
        kc.assert_untouched(xo, wx, kc.CANARY32, "x_out")
        # the cache: nothing but the new tokens' rows changed
        keep = np.ones(NS, dtype=bool)
        keep[new_slot] = False
        for nm, now, was in (("Kc", Kc, Kc0), ("Vc", Vc, Vc0)):
            assert (now[keep].view(np.uint32) == was[keep].view(np.uint32)).all(), f"{nm} ({n_reg} rounds): a cache row other than the new tokens' changed"
        got = P[G:G + H * S * d].reshape(H, S, d)
        items, measured_c = [], 0.0
        for r in range(rows):
            x_row = got_x[r]                                            # what the kernel normalises (checked above)
            xn, q64, k64, v64, ref = _statement(x_row, g, b, eps, inside, W3, bqkv, scale, Kp[r], Vp[r], Wo, np.float64)
            xn32, _, _, _, f32 = _statement(x_row, g, b, eps, inside, W3, bqkv, scale, Kp[r], Vp[r], Wo, np.float32)
            # new cache rows
            ln_base = R.layernorm_base(x_row[None], g, b, float(np.float32(eps)), inside)[0]
            c_ln = 4.0 * float((np.abs(xn32 - xn) / ln_base).max())
            aW = np.abs(W3).astype(np.float64)
            for nm, arr, ref_hv, seg, s_ in (("Kc", Kc, k64, 1, scale), ("Vc", Vc, v64, 2, 1.0)):
                cols = slice(seg * d, seg * d + d)
                bound = s_ * ((d + 2) * R.U32 * (np.abs(xn) @ aW[:, cols] + np.abs(bqkv[cols])) + (c_ln * ln_base) @ aW[:, cols])
                row = arr[new_slot[r]].astype(np.float64)
                assert np.isfinite(row).all(), f"{nm} ({n_reg} rounds): the new row of row {r} is not finite"
                e = float((np.abs(row - ref_hv.reshape(d)) / bound).max())
                if e > ratio:
                    ratio, worst = e, dict(what=nm, n_reg=n_reg, row=r, len=lens[r])
            for h in range(H):
                hs = slice(64 * h, 64 * h + 64)
                Kf = np.concatenate([Kp[r][:, hs].astype(np.float64), k64[h][None]])
                Vf = np.concatenate([Vp[r][:, hs].astype(np.float64), v64[h][None]])
                base = R.attention_base(q64[h][None], Kf, Vf, 1.0) * 64.0 * float(np.abs(Wo[hs]).max())
                measured_c = max(measured_c, float(np.abs(f32[h] - ref[h]).max()) / base)
                items.append((r, h, ref[h], base))
        cc = 4.0 * measured_c
        for r, h, ref, base in items:
            bound = cc * base + R.U32 * float(np.abs(ref).max())
            o_ = got[h, r].astype(np.float64)
            assert np.isfinite(o_).all(), f"non-finite plane ({n_reg} rounds), row {r} head {h} (len = {lens[r]})"
            e = float(np.abs(o_ - ref).max()) / bound
            if e > ratio:
                ratio, worst = e, dict(what="P", n_reg=n_reg, row=r, head=h, len=lens[r], err=e * bound, bound=bound)
        wp = np.zeros(P.shape, dtype=bool)
        for h in range(H):
            wp[G + (h * S) * d:G + (h * S + rows) * d] = True
        kc.assert_untouched(P, wp, kc.CANARY32, "P")
    info = dict(id=c["id"], ratio=ratio, worst=worst)
    assert ratio <= 1.0, f"worst error / bound {ratio:.3g} at {worst}"
    return info


def main(argv):
    """`python attn_rounds_cases.py LIB [ID ...]`: runs the cases (default: all) in THIS process -- the library and nothing else of
    the engine loaded -- and prints one `KCASE <json>` line per case."""
    import json
    lib = load(argv[0])
    for c in cases():
        if argv[1:] and c["id"] not in argv[1:]:
            continue
        try:
            info = dict(run(lib, c), ok=True)
        except AssertionError as e:
            info = dict(id=c["id"], ok=False, msg=str(e)[:600])
        print("KCASE " + json.dumps(info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
