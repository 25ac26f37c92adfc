"""Operator-level cases for the kernel test harness (whisper-burn_amd/tools/kernel_harness.cpp): the case lists, the builders
that lay inputs out with poison and canaries, and the comparison against tests/kernel_refs.py.  Shared by
tests/test_gpu_kernels.py (every case, on the GPU) and tests/test_kernel_harness_emu.py (the cases marked emu, through the
functional model).  Also a small command line: `python kernel_cases.py LIB ID [ID ...]` runs cases in THIS process and prints
one JSON line per case -- the way the tests run cases under another environment (the launchers read their switches once).

Poison: every input element outside the contract (rows >= M, columns in [K, lda), masked k, keys >= kv_len, other segments'
padding) is NaN -- a kernel that reads and USES one produces NaN and fails the comparison.  Canaries: every output array is
larger than the contract (guard band before and after, ldc > N, extra rows) and pre-filled with a bit pattern; after the launch
every element outside the contract must still hold it.  All of it lives inside the arrays the harness copies, so a wrong kernel
is a failed assertion, not a memory fault."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "whisper-burn_amd", "lib")
GPU_LIB = os.path.join(LIB_DIR, "libwhisper_hip_ktest.so")
EMU_LIB = os.path.join(LIB_DIR, "libwhisper_hip_ktest_emu.so")

G = 64                                   # guard band, elements (a multiple of 16 bytes for every element size)
CANARY32 = np.uint32(0xC3C3C3C3)         # as f32: -391.5..., finite
CANARY16 = np.uint16(0xC3C3)
NAN16 = np.uint16(0x7E00)
EARG = -2


# ---- ctypes mirror of the harness structs (every field 8 bytes wide) --------------------------------------------------------------
class Buf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("bytes", C.c_int64), ("off", C.c_int64)]


def _struct(name, spec):
    fields = []
    for group, typ in spec:
        fields += [(f, typ) for f in group.split()]
    return type(name, (C.Structure,), {"_fields_": fields})


Gemm = _struct("Gemm", [
    ("variant", C.c_int64), ("A Ah Al desc B W Wh Wl C Ch Cl bias residual aux aux_idx", Buf), ("residual_is_c", C.c_int64),
    ("lda a_mask_align conv1_tstride ldb ldc ldr ld_aux n_aux_rows", C.c_int64),
    ("col_scale_period col_scale_width M N K act ksplit c_split_stride c_block_cols c_block_stride ldwt", C.c_int64),
    ("use_range_flag range_flag_out", C.c_int64), ("col_scale", C.c_double)])
Attn = _struct("Attn", [
    ("which", C.c_int64), ("X", Buf), ("q_off k_off v_off", C.c_int64), ("O Oh Ol segs", Buf),
    ("ldq ldkv ldo n_segs max_q_len n_head causal split wrote_pieces", C.c_int64), ("scale", C.c_double)])
Norm = _struct("Norm", [
    ("which", C.c_int64), ("x g b y yh yl", Buf), ("M d eps_inside_sqrt L n_vocab", C.c_int64), ("eps", C.c_double)])
Skinny = _struct("Skinny", [
    ("A B th tl P", Buf), ("lda M N K ksplit plane use_range_flag range_flag_out", C.c_int64)])

_LIBS = {}


def load(path):
    if path not in _LIBS:
        lib = C.CDLL(path)
        for f in ("wbk_gemm", "wbk_attention", "wbk_norm", "wbk_skinny"):
            getattr(lib, f).restype = C.c_int
            getattr(lib, f).argtypes = [C.c_void_p]
        lib.wbk_skinny_ksplit.restype = C.c_int
        lib.wbk_skinny_ksplit.argtypes = [C.c_int] * 4
        _LIBS[path] = lib
    return _LIBS[path]


def buf(arr, off_elems=0):
    """arr must stay alive for the call (the caller keeps the reference)."""
    if arr is None:
        return Buf(None, 0, 0)
    assert arr.flags["C_CONTIGUOUS"]
    return Buf(arr.ctypes.data, arr.nbytes, off_elems * arr.itemsize)


def nan32(n):
    return np.full(n, np.nan, dtype=np.float32)


def canary32(n):
    return np.full(n, CANARY32, dtype=np.uint32).view(np.float32)


def canary16(n):
    return np.full(n, CANARY16, dtype=np.uint16)


def values(rng, shape, scale):
    """Normal values of the given scale with |x| >= 1e-3: no fp16-subnormal high pieces (the split's relative bound holds)."""
    x = rng.standard_normal(shape) * scale
    x = np.where(np.abs(x) < 1e-3, np.copysign(1e-3, x), x)
    return x.astype(np.float32)


STASH = None                             # diagnostics: a dict collects the raw attention outputs per case id
HIP_ERROR = [0]                          # the first HIP error any call of this process returned


def _call(fn, struct):
    """One harness call.  After a HIP error nothing more is launched by this process: every later case fails here instead."""
    assert HIP_ERROR[0] == 0, f"not launched: an earlier call returned the HIP error {HIP_ERROR[0]}"
    st = fn(C.addressof(struct))
    if st <= -1000:
        HIP_ERROR[0] = st
    return st


def assert_untouched(arr_after, mask_written, canary, what):
    bits = arr_after.view(np.uint32 if arr_after.itemsize == 4 else np.uint16)
    bad = (bits != canary) & ~mask_written
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the contract were overwritten (first at {int(np.argmax(bad))})"


# ---- the dispatchers, mirrored (csrc/gemm.hip launch_gemm_f32, csrc/gemm_f16x3.hip launch_gemm_f16x3, csrc/attention.hip) -------
# These name the branch a shape takes so that the case lists can be ASSERTED to cover every branch.  They cannot notice a retune of
# the C++ thresholds by themselves: the `if` ladders carry a comment pointing here, and profiles/ktest_kernel_names.txt is the
# kernel-name table of one traced run of tests/test_gpu_kernels.py (every template instance present).
def _blocks(M, N, bm, bn):
    return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)


def gemm_f32_branch(M, N, K, ksplit=1, conv1=False):
    if conv1:
        return "conv1_128x128" if _blocks(M, N, 128, 128) >= 384 else "conv1_64x64"
    if ksplit > 1:
        return "splitk_32x128" if M <= 32 else "splitk_64x64"
    if K % 32 != 0:
        return "k16_32x128" if M <= 32 else "k16_64x64"
    if _blocks(M, N, 128, 128) >= 768:
        return "rows_128x128"
    return "rows_32x128"


GEMM_F32_BRANCHES = {"conv1_128x128", "conv1_64x64", "splitk_32x128", "splitk_64x64", "k16_32x128", "k16_64x64", "rows_128x128",
                     "rows_32x128"}


def gemm_f16x3_branch(M, N, K, ksplit=1):
    if M <= 32:
        return "splitk_32x128" if ksplit > 1 else "m32_32x128"
    if ksplit > 1:
        return "splitk_64x64"
    return "64x64" if _blocks(M, N, 128, 128) < 384 else "128x128"


GEMM_F16X3_BRANCHES = {"m32_32x128", "64x64", "128x128", "splitk_32x128", "splitk_64x64"}


def attn_branch(which, split, causal, max_q_len, n_head, n_segs, kvsplit_on=True, f16_on=True):
    blocks128 = ((max_q_len + 127) // 128) * n_head * n_segs
    kvsplit = (not causal) and max_q_len >= 256 and blocks128 < 384 and kvsplit_on
    if which == 1 and split and f16_on and not kvsplit and max_q_len > 64:
        return "f16x3"
    if kvsplit:
        return "f32_kvsplit"
    return "f32_nw2" if max_q_len <= 64 else "f32_nw4"


ATTN_BRANCHES = {"f32_nw2", "f32_nw4", "f32_kvsplit", "f16x3"}


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------
def _g(id, variant, M, N, K, emu=False, **kw):
    d = dict(id=f"{variant}-{id}", family="gemm_" + variant, variant=variant, M=M, N=N, K=K, emu=emu, lda_pad=0, ldc_pad=4,
             mode="rows", bias=False, gelu=False, cs=None, residual=None, ldr_pad=4, aux=0, cblocks=0, pieces_out=False, ksplit=1,
             ldb_pad=0, mask_align=0, refuse=None, overflow=False, w_scale=0.1)
    d.update(kw)
    return d


def gemm_cases():
    out = []
    for v in ("f32", "f16x3"):
        k16 = v == "f32"                                           # the split-precision kernel needs K % 32 == 0
        # edges of M against the tile heights, N against the tile widths
        for i, M in enumerate((1, 31, 32, 33, 63, 65, 127, 129)):
            N = (4, 60, 64, 68, 1031, 131, 260, 37)[i]
            K = (32, 96, 32, 96, 32, 96, 32, 96)[i]
            out.append(_g(f"edge-M{M}-N{N}-K{K}", v, M, N, K, emu=M in (1, 33), lda_pad=(0, 4, 8)[i % 3] if v == "f32" else (0, 8)[i % 2],
                          ldc_pad=(4, 1, 0, 7)[i % 4]))
        out.append(_g("K1536", v, 65, 68, 1536, lda_pad=8))
        if k16:
            out.append(_g("K16-M31", v, 31, 60, 16, emu=True, lda_pad=4))
            out.append(_g("K48-M32", v, 32, 132, 48, lda_pad=4))
            out.append(_g("K48-M33", v, 33, 68, 48, emu=True))
            out.append(_g("K16-M129", v, 129, 64, 16, bias=True, gelu=True))
            out.append(_g("ldb-gt-N", v, 33, 60, 32, ldb_pad=8))
        # the large tiles: single launches
        out.append(_g("tile128", v, *((4033, 3012, 32) if v == "f32" else (2000, 3012, 64)), bias=True))
        # epilogues: each switch alone
        out.append(_g("bias", v, 33, 68, 64, emu=True, bias=True))
        out.append(_g("gelu", v, 65, 132, 64, gelu=True))
        out.append(_g("colscale", v, 33, 96, 32, cs=(0.125, 48, 16)))
        out.append(_g("residual", v, 65, 60, 64, residual="sep", ldr_pad=12))
        out.append(_g("residual-alias", v, 63, 68, 32, emu=True, residual="alias"))
        out.append(_g("aux", v, 65, 64, 32, aux=5, emu=True))
        out.append(_g("cblocks2", v, 33, 128, 32, cblocks=2, emu=True))
        out.append(_g("cblocks4", v, 65, 256, 64, cblocks=4))
        out.append(_g("desc", v, 65, 68, 96, mode="desc", mask_align=8, emu=True))
        if k16:
            out.append(_g("desc-align1", v, 33, 60, 48, mode="desc", mask_align=1, emu=True))
        # the engine's combinations (d = 64: fused QKV with the scale on Q and K, Q only, cross-Q; MLP; out-projection; conv; logits)
        d = 64
        out.append(_g("qkv-3d-2d", v, 65, 3 * d, d, bias=True, cs=(0.35355339, 3 * d, 2 * d)))
        out.append(_g("kv-2d-d", v, 63, 2 * d, d, bias=True, cs=(0.35355339, 2 * d, d), cblocks=2))
        out.append(_g("q-d-d", v, 33, d, d, bias=True, cs=(0.35355339, d, d), emu=True))
        out.append(_g("mlp1", v, 129, 4 * d, d, bias=True, gelu=True, emu=False))
        out.append(_g("mlp2-residual", v, 129, d, 4 * d, bias=True, residual="alias"))
        out.append(_g("bias-gelu-aux", v, 65, 68, 96, bias=True, gelu=True, aux=7))
        out.append(_g("splitk-M9", v, 9, 132, 384, ksplit=4, emu=True))
        out.append(_g("splitk-M65", v, 65, 68, 352, ksplit=3, emu=True))          # 352 / 3 -> slices of 128, 128, 96
        out.append(_g("splitk-M32-uneven", v, 32, 1028, 160, ksplit=4))           # slices of 64, 64, 32, 0
    # split precision only: pieces in, pieces out, the range flag
    out.append(_g("pieces-out", "f16x3", 65, 68, 64, bias=True, gelu=True, pieces_out=True, emu=True))
    out.append(_g("pieces-out-M31", "f16x3", 31, 132, 32, bias=True, pieces_out=True))
    out.append(_g("pieces-in", "f16x3", 65, 68, 96, mode="pre", lda_pad=8, bias=True, emu=True))
    out.append(_g("pieces-in-M9", "f16x3", 9, 64, 32, mode="pre", residual="sep"))
    out.append(_g("pieces-in-tile128", "f16x3", 2000, 3012, 64, mode="pre", pieces_out=False))
    out.append(_g("range-flag", "f16x3", 33, 68, 64, overflow=True, emu=True))
    # exact f32 only: the conv stem's gather
    out.append(_g("conv1-64x64", "f32", 203, 68, 48, mode="conv1", bias=True, gelu=True, emu=False))
    out.append(_g("conv1-64x64-M33", "f32", 33, 64, 48, mode="conv1", emu=True))
    out.append(_g("conv1-K240", "f32", 129, 132, 240, mode="conv1", bias=True, gelu=True, aux=9, w_scale=0.03))
    out.append(_g("conv1-128x128", "f32", 6100, 1028, 48, mode="conv1", bias=True, gelu=True))
    # refusals: the launcher returns -1 before any launch, C stays untouched
    out.append(_g("refuse-K24", "f32", 9, 64, 24, refuse="k", emu=True))
    out.append(_g("refuse-ldb", "f32", 9, 62, 32, refuse="ldb", ldb_pad=0, emu=True))
    out.append(_g("refuse-splitk-bias", "f32", 9, 64, 64, refuse="splitk_epilogue", ksplit=2, bias=True, emu=True))
    out.append(_g("refuse-splitk-K48", "f32", 9, 64, 48, refuse="splitk_k", ksplit=2, emu=True))
    out.append(_g("refuse-K48", "f16x3", 9, 64, 48, refuse="k", emu=True))
    out.append(_g("refuse-ldwt", "f16x3", 9, 64, 32, refuse="ldwt", emu=True))
    out.append(_g("refuse-Ah-without-Al", "f16x3", 9, 64, 32, refuse="ah_no_al", mode="pre", emu=True))
    out.append(_g("refuse-splitk-gelu", "f16x3", 9, 64, 64, refuse="splitk_epilogue", ksplit=2, gelu=True, emu=True))
    return out


def gelu_ulps_for(pre):
    """The GELU term of the bound: 4x the worst error, in ulps of max(1, |v|), of torch's exact-form f32 GELU on the CPU against
    the f64 reference on the same f32 pre-activations; floor 4 ulp.  Returns (ulps used, worst torch error in ulps)."""
    import torch
    p32 = np.ascontiguousarray(pre.astype(np.float32))
    t = torch.nn.functional.gelu(torch.from_numpy(p32), approximate="none").numpy().astype(np.float64)
    ref = R.gelu_erf(p32.astype(np.float64))
    worst = float((np.abs(t - ref) / (R.U32 * np.maximum(1.0, np.abs(p32.astype(np.float64))))).max())
    return max(4.0, 4.0 * worst), worst


def run_gemm(lib, c, scheme=None):
    """scheme = None: the harness.  Otherwise a NumPy statement of the arithmetic, (matmul(A, W) -> f64, gelu(v) -> f64), takes the
    kernel's place (tests/test_kernel_harness_emu.py: the correct schemes must pass, mutated ones must miss by a decade); the
    function then returns error / bound without asserting it."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 7919 + 13)
    M, N, K, v = c["M"], c["N"], c["K"], c["variant"]
    f16 = v == "f16x3"
    g = Gemm()
    keep = []                                                       # arrays the struct points into
    g.variant = 1 if f16 else 0
    g.M, g.N, g.K, g.ksplit = M, N, K, c["ksplit"]
    g.act = 1 if c["gelu"] else 0
    g.col_scale = 1.0
    g.a_mask_align = 1
    Kp = (K + 31) // 32 * 32                                        # refusal cases: arrays sized for the padded K
    # ---- A ----
    mode = c["mode"]
    desc = None
    if mode in ("rows", "desc"):
        lda = Kp + c["lda_pad"]
        flat = nan32(2 * G + (M + 3) * lda)
        base = G
        if mode == "rows":
            for m in range(M):
                flat[base + m * lda: base + m * lda + K] = values(rng, K, 1.0)
            if c["overflow"]:
                flat[base + (M // 2) * lda + K // 2] = 70000.0
        else:
            al = c["mask_align"]
            base = G + 8                                            # off may be negative: masked k is never read
            desc = np.zeros((M, 3), dtype=np.int64)
            for m in range(M):
                klo = (0, al, 2 * al, 8 if al == 8 else 9)[m % 4]
                khi = K - (0, al, 0, 3 * al)[(m // 2) % 4]
                off = m * lda - (8 if klo >= 8 else 0)              # row 0 .. 3: off < 0 for the klo >= 8 rows
                desc[m] = (off, klo, khi)
                flat[base + off + klo: base + off + khi] = values(rng, khi - klo, 1.0)
            g.a_mask_align = al
        A = R.rows_effective(flat, base, M, K, lda, desc)
        g.A, g.lda = buf(flat, base), lda
        keep.append(flat)
    elif mode == "pre":
        lda = Kp + c["lda_pad"]
        a32 = values(rng, (M, K), 1.0)
        hb, lb = R.split_f16_bits(a32)
        ph = np.full(2 * G + (M + 3) * lda, NAN16, dtype=np.uint16)
        pl = ph.copy()
        for m in range(M):
            ph[G + m * lda: G + m * lda + K] = hb[m]
            pl[G + m * lda: G + m * lda + K] = lb[m]
        A = R.join_f16(hb, lb)
        g.Ah, g.lda = buf(ph, G), lda
        if c["refuse"] != "ah_no_al":
            g.Al = buf(pl, G)
        keep += [ph, pl]
    else:                                                           # conv1: [Cin][T] planes, windows separated by a NaN column
        cin = K // 3
        wins = []
        left, col = M, 1
        for f in (1, 2, 37, 10 ** 9):                               # window lengths: 1 frame, 2 frames, mid, the rest
            f = min(f, left)
            if f <= 0:
                break
            wins.append((col, f))
            col += f + 1
            left -= f
        T = (col + 3) // 4 * 4
        plane = nan32(G + cin * T + G)
        desc = np.zeros((M, 3), dtype=np.int64)
        m = 0
        for c0, f in wins:
            for ci in range(cin):
                plane[G + ci * T + c0: G + ci * T + c0 + f] = values(rng, f, 1.0)
            for t in range(f):
                desc[m] = (c0 + t, 1 if t == 0 else 0, 1 if t == f - 1 else 0)
                m += 1
        A = R.conv1_effective(plane, G, M, K, T, desc)
        g.A, g.conv1_tstride = buf(plane, G), T
        keep.append(plane)
    if desc is not None:
        dd = np.zeros(M, dtype=np.dtype([("off", "<i4"), ("klo", "<i2"), ("khi", "<i2")]))
        dd["off"], dd["klo"], dd["khi"] = desc[:, 0], desc[:, 1], desc[:, 2]
        g.desc = buf(dd)
        keep.append(dd)
    # ---- B ----
    W = values(rng, (K, N), c["w_scale"])
    if f16:
        Wd = np.ascontiguousarray(W)
        ldwt = K
        if c["refuse"] == "ldwt":
            ldwt = K + 4
        wh = canary16(N * max(ldwt, Kp) + G)
        wl = canary16(N * max(ldwt, Kp) + G)
        g.W, g.Wh, g.Wl, g.ldwt = buf(Wd), buf(wh), buf(wl), ldwt
        keep += [Wd, wh, wl]
    else:
        ldb = (N + 3) // 4 * 4 + c["ldb_pad"]
        if c["refuse"] == "ldb":
            ldb = N                                                 # 62: not a multiple of 4
        bflat = nan32(G + (Kp + 2) * ldb + G)
        for k in range(K):
            bflat[G + k * ldb: G + k * ldb + N] = W[k]
        g.B, g.ldb = buf(bflat, G), ldb
        keep.append(bflat)
    # ---- epilogue operands ----
    bias = res = aux = aux_idx = None
    if c["bias"]:
        bias = values(rng, N, 0.5)
        bb = nan32(G + N + G)
        bb[G: G + N] = bias
        g.bias = buf(bb, G)
        keep.append(bb)
    cs = c["cs"]
    if cs:
        g.col_scale, g.col_scale_period, g.col_scale_width = cs
    ldc = N + c["ldc_pad"]
    cb_cols = cb_stride = 0
    if c["cblocks"]:
        cb_cols = N // c["cblocks"]
        ldc = cb_cols + c["ldc_pad"]
        cb_stride = (M + 2) * ldc + 4
    nsplit = max(1, c["ksplit"])
    split_stride = (M + 1) * ldc + 8 if c["ksplit"] > 1 else 0
    total = G + (nsplit - 1) * split_stride + (max(1, c["cblocks"]) - 1) * cb_stride + (M + 2) * ldc + G
    pos = G + R.c_positions(M, N, ldc, cb_cols, cb_stride)
    if c["residual"] == "sep":
        res = values(rng, (M, N), 1.0)
        ldr = N + c["ldr_pad"]
        rr = nan32(G + (M + 1) * ldr + G)
        for m in range(M):
            rr[G + m * ldr: G + m * ldr + N] = res[m]
        g.residual, g.ldr = buf(rr, G), ldr
        keep.append(rr)
    if c["aux"]:
        n_aux = c["aux"]
        auxv = values(rng, (n_aux, N), 1.0)
        ld_aux = N + 4
        aa = nan32(G + n_aux * ld_aux + G)
        for r in range(n_aux):
            aa[G + r * ld_aux: G + r * ld_aux + N] = auxv[r]
        aux_idx = (np.arange(M) % n_aux).astype(np.int32)          # repeating indices
        aux_idx[0] = n_aux - 1
        g.aux, g.aux_idx, g.ld_aux, g.n_aux_rows = buf(aa, G), buf(aux_idx), ld_aux, n_aux
        aux = auxv
        keep += [aa, aux_idx]
    if c["pieces_out"]:
        ch, cl = canary16(total), canary16(total)
        g.Ch, g.Cl = buf(ch, G), buf(cl, G)
        keep += [ch, cl]
    cbuf = canary32(total)
    if c["residual"] == "alias":
        res = values(rng, (M, N), 1.0)
        cbuf[pos] = res
        g.residual_is_c, g.ldr = 1, ldc
    g.C, g.ldc = buf(cbuf, G), ldc
    g.c_split_stride, g.c_block_cols, g.c_block_stride = split_stride, cb_cols, cb_stride
    g.use_range_flag = 1 if f16 else 0
    c_before = cbuf.copy()
    # ---- the reference, before the launch ----
    ulps_used = worst_torch = None
    if c["refuse"] is None and not c["overflow"] and c["ksplit"] <= 1:
        gul = 4.0
        if c["gelu"]:
            _, pre0, _ = R.gemm_ref(A, W, bias)
            gul, worst_torch = gelu_ulps_for(pre0)
            ulps_used = gul
        ref, pre, bound = R.gemm_ref(A, W, bias, c["gelu"], cs[0] if cs else 1.0, cs[1] if cs else 0, cs[2] if cs else 0, res, aux,
                                     aux_idx, variant=v, gelu_ulps=gul,
                                     acc_cap=4.0 * float(np.abs(R.matmul_f32(A, W) - A @ W.astype(np.float64)).max()) if f16 else None)

    info = dict(id=c["id"], family=c["family"], branch=None)
    if scheme is not None:
        mm, gl = scheme
        if c["refuse"] is not None or c["overflow"]:
            return info
        if c["ksplit"] > 1:
            ratio = 0.0
            planes = R.gemm_splitk_ref(A, W, c["ksplit"])
            for z, (ka, kb) in enumerate(R.splitk_slices(K, c["ksplit"])):
                if kb > ka:
                    absdot = np.abs(A[:, ka:kb]) @ np.abs(W[ka:kb].astype(np.float64))
                    bnd = ((kb - ka) + 4) * R.U32 * absdot + (R.REP16 * absdot if f16 else 0.0)
                    ratio = max(ratio, float((np.abs(mm(A[:, ka:kb], W[ka:kb]) - planes[z]) / bnd).max()))
            info["ratio"] = ratio
            return info
        got = R.gemm_epilogue(mm(A, W), bias, c["gelu"], cs[0] if cs else 1.0, cs[1] if cs else 0, cs[2] if cs else 0, res, aux,
                              aux_idx, gelu=gl)
        info["ratio"] = float((np.abs(got - ref) / bound).max())
        return info
    st = _call(lib.wbk_gemm, g)
    if c["refuse"] is not None:
        assert st == -1, f"launcher returned {st}, expected the refusal -1"
        assert (cbuf.view(np.uint32) == c_before.view(np.uint32)).all(), "a refused launch changed C"
        return info
    assert st == 0, f"harness status {st}"
    written = np.zeros(total, dtype=bool)
    if f16:
        hb, lb = R.split_f16_bits(W)
        assert (wh[:N * K].reshape(N, K) == hb.T).all() and (wl[:N * K].reshape(N, K) == lb.T).all(), \
            "launch_split_weight_f16 != split_f16(W).T"
        assert (wh[N * K:] == CANARY16).all() and (wl[N * K:] == CANARY16).all(), "launch_split_weight_f16 wrote past [N][K]"
        info["branch"] = gemm_f16x3_branch(M, N, K, c["ksplit"])
    else:
        info["branch"] = gemm_f32_branch(M, N, K, c["ksplit"], mode == "conv1")
    if c["overflow"]:
        assert g.range_flag_out == 1, "an operand of 70000 did not raise range_flag"
        written[pos] = True
        assert_untouched(cbuf, written, CANARY32, "C")
        return info
    if f16:
        assert g.range_flag_out == 0, "range_flag raised on in-range inputs"
    if c["ksplit"] > 1:
        planes = R.gemm_splitk_ref(A, W, c["ksplit"])
        ratio = 0.0
        for z, (ka, kb) in enumerate(R.splitk_slices(K, c["ksplit"])):
            got = cbuf[pos + z * split_stride].astype(np.float64)
            absdot = np.abs(A[:, ka:kb]) @ np.abs(W[ka:kb].astype(np.float64))
            bnd = ((kb - ka) + 4) * R.U32 * absdot + (R.REP16 * absdot if f16 else 0.0)
            err = np.abs(got - planes[z])
            assert np.isfinite(got).all(), f"plane {z}: non-finite output (poison read?)"
            if kb == ka:
                assert (got == 0).all(), f"plane {z} of an empty K-slice is not zero"
            else:
                assert (err <= bnd).all(), f"plane {z}: worst error / bound {float((err / bnd).max()):.3g}"
                ratio = max(ratio, float((err / bnd).max()))
            written[pos + z * split_stride] = True
        assert_untouched(cbuf, written, CANARY32, "C")
        info["ratio"] = ratio
        return info
    if c["pieces_out"]:
        # the same launch with f32 output: the pieces must be split_f16 of it, bit for bit
        assert (cbuf.view(np.uint32) == c_before.view(np.uint32)).all(), "piece output also wrote the f32 C"
        g.Ch, g.Cl = Buf(None, 0, 0), Buf(None, 0, 0)
        assert _call(lib.wbk_gemm, g) == 0
        eh, el = R.split_f16_bits(cbuf[pos])
        assert (ch[pos] == eh).all() and (cl[pos] == el).all(), "piece output != split_f16(f32 output)"
        written[pos] = True
        assert_untouched(ch, written, CANARY16, "Ch")
        assert_untouched(cl, written, CANARY16, "Cl")
    got = cbuf[pos].astype(np.float64)
    assert np.isfinite(got).all(), "non-finite output (a poisoned element was read and used?)"
    err = np.abs(got - ref)
    ratio = float((err / bound).max())
    info.update(ratio=ratio, worst=float(err.max()))
    if ulps_used is not None:
        info.update(gelu_ulps=ulps_used, gelu_torch_worst_ulps=worst_torch)
    assert (err <= bound).all(), f"worst error / bound {ratio:.3g} (worst error {float(err.max()):.3g})"
    written[pos] = True
    assert_untouched(cbuf, written, CANARY32, "C")
    return info


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _a(id, which, segs, n_head, emu=False, **kw):
    """segs: list of (q_len, kv_len)."""
    d = dict(id=f"attn-{id}", family="attention", which=which, segs=segs, n_head=n_head, emu=emu, split=0, pieces=False, causal=0,
             scale=1.0, layout="fused", stress=False, env=None)
    d.update(kw)
    return d


S025 = float(np.float32(64 ** -0.25))


def attn_cases():
    out = []
    mixed64 = [(1, 1), (63, 31), (64, 32), (5, 33), (33, 63), (17, 65)]
    mixed129 = [(129, 65), (1, 300), (127, 1), (65, 33), (63, 63)]
    for which, split, tag in ((0, 0, "f32api"), (1, 0, "exact"), (1, 1, "split")):
        out.append(_a(f"{tag}-nw2-mixed", which, mixed64, 2, split=split, scale=S025, emu=(tag == "f32api")))
        out.append(_a(f"{tag}-nw2-causal", which, [(64, 64), (33, 65), (1, 1), (7, 31)], 1, split=split, causal=1, scale=0.125 * 4,
                      layout="cross"))
        out.append(_a(f"{tag}-q129-mixed", which, mixed129, 2, split=split, scale=S025, layout="cross", emu=(tag == "split")))
        out.append(_a(f"{tag}-q129-causal", which, [(129, 129), (65, 300), (127, 127), (1, 5)], 2, split=split, causal=1, scale=0.125 * 4))
        out.append(_a(f"{tag}-q300-kvsplit", which, [(300, 300), (1, 31), (257, 65)], 6, split=split, scale=1.0, layout="cross"))
        out.append(_a(f"{tag}-q300-causal", which, [(300, 300), (129, 300)], 1, split=split, causal=1, scale=S025))
        out.append(_a(f"{tag}-stress-q129", which, [(129, 97), (40, 33)], 1, split=split, stress=True, scale=1.0))
        out.append(_a(f"{tag}-scale-0.125", which, [(65, 63), (64, 32)], 2, split=split, scale=0.125, layout="cross"))
    out.append(_a("f32api-stress-nw2", 0, [(64, 97), (3, 33)], 1, stress=True, emu=True))
    out.append(_a("f32api-stress-kvsplit", 0, [(260, 161)], 1, stress=True))
    out.append(_a("f32api-kvsplit-emu", 0, [(257, 33)], 1, scale=S025, emu=True))
    # >= 384 blocks of 128 queries: the LDS-tiled kernels at a non-causal shape the key-split kernel would otherwise take
    big = [(300, 65)] * 21 + [(260, 33)]
    out.append(_a("exact-q300-many", 1, big, 6, split=0, scale=S025))
    out.append(_a("split-q300-many", 1, big, 6, split=1, scale=S025, pieces=True))
    out.append(_a("split-pieces-q129", 1, mixed129, 2, split=1, pieces=True, scale=S025, layout="cross", emu=True))
    out.append(_a("split-pieces-causal", 1, [(129, 129), (65, 300)], 6, split=1, pieces=True, causal=1, scale=0.125))
    out.append(_a("split-pieces-nw2", 1, mixed64, 2, split=1, pieces=True))           # exact-f32 kernel: pieces NOT written
    out.append(_a("exact-pieces-q129", 1, mixed129, 1, split=0, pieces=True))           # split off: pieces NOT written
    # the switches, read once per process: one child process per value
    for which, split, tag in ((0, 0, "f32api"), (1, 1, "split")):
        out.append(_a(f"{tag}-q300-kvsplit-off", which, [(300, 300), (1, 31), (257, 65)], 2, split=split, scale=S025,
                      env=("WHISPER_HIP_ATTN_KVSPLIT", "0")))
    out.append(_a("split-q129-f16-off", 1, mixed129, 2, split=1, pieces=True, scale=S025, env=("WHISPER_HIP_ATTN_F16", "0")))
    out.append(_a("refuse-ldq-not-x4", 0, [(5, 7)], 1, bad_ld=True, emu=True))      # the harness refuses what kernels.h rules out
    out.append(_a("split-causal-f16-off", 1, [(129, 129), (65, 300)], 1, split=1, causal=1, env=("WHISPER_HIP_ATTN_F16", "0")))
    return out


def attn_case_branch(c):
    env = c["env"] or ("", "")
    return attn_branch(c["which"], c["split"], c["causal"], max(q for q, _ in c["segs"]), c["n_head"], len(c["segs"]),
                       kvsplit_on=env != ("WHISPER_HIP_ATTN_KVSPLIT", "0"), f16_on=env != ("WHISPER_HIP_ATTN_F16", "0"))


def run_attn(lib, c, scheme=None):
    """scheme: None (the harness) or a function (Q, K, V, scale, causal) -> O in f64 that takes the kernel's place (see run_gemm)."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 104729 + 7)
    H, segs = c["n_head"], c["segs"]
    d = 64 * H
    # rows: segment i's queries and keys start at rows that are multiples of nothing, with poisoned rows between segments
    q_rows, kv_rows, rq, rk = [], [], 3, 5
    for ql, kl in segs:
        q_rows.append(rq)
        kv_rows.append(rk)
        rq += ql + 1 + (ql % 3)
        rk += kl + 2 + (kl % 2)
    if c["layout"] == "fused":                                      # one [rows][3d] array: Q | K | V (the encoder's fused view)
        ldq = ldkv = 3 * d
        rows = max(rq, rk) + 2
        X = nan32(G + rows * 3 * d + G)
        q_off, k_off, v_off = G, G + d, G + 2 * d
    else:                                                           # Q [rows][d + 4], K | V [rows][2d] (the cross view)
        ldq, ldkv = d + 4, 2 * d
        X = nan32(G + (rq + 1) * ldq + G + (rk + 1) * ldkv + G)
        q_off = G
        k_off = G + (rq + 1) * ldq + G
        v_off = k_off + d
    sc = float(np.float32(c["scale"]))
    for i, (ql, kl) in enumerate(segs):
        for r in range(ql):
            o = q_off + (q_rows[i] + r) * ldq
            X[o: o + d] = values(rng, d, 1.0)
        for r in range(kl):
            o = k_off + (kv_rows[i] + r) * ldkv
            X[o: o + d] = values(rng, d, 1.0)
            o = v_off + (kv_rows[i] + r) * ldkv
            X[o: o + d] = values(rng, d, 1.0)
        if c["stress"]:
            # scores that span +-80 and stay finite: queries along one axis, keys along the same one.  Query 0: the dominant key
            # sits in the LAST key tile; query 1: in the first; query 2: all scores equal.
            kmat = np.zeros((kl, 64), dtype=np.float32)
            kmat[:, 0] = np.linspace(-1.0, 1.0, kl, dtype=np.float32)
            qmat = values(rng, (ql, 64), 0.05)
            qmat[:, 0] = (rng.uniform(-80.0, 80.0, ql) / sc / sc).astype(np.float32)
            qmat[0] = 0
            qmat[0, 0] = 80.0 / sc / sc
            if ql > 1:
                qmat[1] = 0
                qmat[1, 0] = -80.0 / sc / sc
            if ql > 2:
                qmat[2] = 0
            for h in range(H):
                for r in range(ql):
                    o = q_off + (q_rows[i] + r) * ldq + 64 * h
                    X[o: o + 64] = qmat[r]
                for r in range(kl):
                    o = k_off + (kv_rows[i] + r) * ldkv + 64 * h
                    X[o: o + 64] = kmat[r]
    ldo = d + 4
    o_total = G + (rq + 2) * ldo + G
    O = canary32(o_total)
    Oh = Ol = None
    sg = np.zeros((len(segs), 4), dtype=np.int32)
    for i, (ql, kl) in enumerate(segs):
        sg[i] = (q_rows[i], ql, kv_rows[i], kl)
    t = Attn()
    t.which, t.X, t.q_off, t.k_off, t.v_off = c["which"], buf(X), q_off, k_off, v_off
    t.O, t.segs = buf(O, G), buf(sg)
    if c["pieces"]:
        Oh, Ol = canary16(o_total), canary16(o_total)
        t.Oh, t.Ol = buf(Oh, G), buf(Ol, G)
    t.ldq, t.ldkv, t.ldo, t.n_segs, t.max_q_len, t.n_head = ldq, ldkv, ldo, len(segs), max(q for q, _ in segs), H
    t.causal, t.split, t.scale = c["causal"], c["split"], c["scale"]
    branch = attn_case_branch(c)
    info = dict(id=c["id"], family="attention", branch=branch)
    if c.get("bad_ld"):
        if scheme is None:
            t.ldq += 2
            assert _call(lib.wbk_attention, t) == EARG, "ldq % 4 != 0 must be refused before the launch"
            assert (O.view(np.uint32) == CANARY32).all()
        return info
    if scheme is None:
        st = _call(lib.wbk_attention, t)
        assert st == 0, f"harness status {st}"
    else:
        t.wrote_pieces = 0
        c = dict(c, pieces=False)
        for i, (ql, kl) in enumerate(segs):
            for h in range(H):
                Q = np.stack([X[q_off + (q_rows[i] + r) * ldq + 64 * h:][:64] for r in range(ql)])
                Km = np.stack([X[k_off + (kv_rows[i] + r) * ldkv + 64 * h:][:64] for r in range(kl)])
                Vm = np.stack([X[v_off + (kv_rows[i] + r) * ldkv + 64 * h:][:64] for r in range(kl)])
                oi = G + (q_rows[i] + np.arange(ql))[:, None] * ldo + 64 * h + np.arange(64)[None, :]
                O[oi] = scheme(Q, Km, Vm, c["scale"], c["causal"])
    wrote = branch == "f16x3" and c["pieces"]
    assert int(t.wrote_pieces) == int(wrote), f"launch_attention returned {t.wrote_pieces}, the {branch} kernel was expected"
    got_f32 = O
    if wrote:
        assert (O.view(np.uint32) == CANARY32).all(), "pieces were written AND the f32 output touched"
        # the same launch with f32 output: the pieces join to it within the split's bound
        t.Oh, t.Ol = Buf(None, 0, 0), Buf(None, 0, 0)
        assert _call(lib.wbk_attention, t) == 0 and t.wrote_pieces == 0
    elif c["pieces"]:
        assert (Oh == CANARY16).all() and (Ol == CANARY16).all(), "an exact-f32 kernel wrote the piece arrays"
    written = np.zeros(o_total, dtype=bool)
    ratio = 0.0
    worst_at = None
    measured_c = 0.0
    results = []
    for i, (ql, kl) in enumerate(segs):
        for h in range(H):
            Q = np.stack([X[q_off + (q_rows[i] + r) * ldq + 64 * h:][:64] for r in range(ql)])
            Km = np.stack([X[k_off + (kv_rows[i] + r) * ldkv + 64 * h:][:64] for r in range(kl)])
            Vm = np.stack([X[v_off + (kv_rows[i] + r) * ldkv + 64 * h:][:64] for r in range(kl)])
            ref, _ = R.attention_ref(Q, Km, Vm, c["scale"], c["causal"])
            f32, _ = R.attention_ref(Q, Km, Vm, c["scale"], c["causal"], dtype=np.float32)
            base = R.attention_base(Q, Km, Vm, c["scale"])
            measured_c = max(measured_c, float(np.abs(f32 - ref).max()) / base)
            idx = (G + (q_rows[i] + np.arange(ql))[:, None] * ldo + 64 * h + np.arange(64)[None, :])
            written[idx] = True
            rep = R.attention_split_bound(Q, Km, Vm, c["scale"], c["causal"]) if branch == "f16x3" else 0.0
            results.append((idx, ref, base, rep, float(np.abs(Vm).max())))
    # c: 4x the error of the plain f32 NumPy evaluation of the same statement, in units of the (segment, head)'s base;
    # floor 1 / max-base ulp of the output scale so that a case whose f32 evaluation happens to be exact keeps one rounding
    cc = 4.0 * measured_c
    for idx, ref, base, rep, vmax in results:
        bound = cc * base + R.U32 * vmax + rep                      # rep: the split operands' share (kernel_refs.attention_split_bound)
        got = got_f32[idx].astype(np.float64)
        assert scheme is not None or np.isfinite(got).all(), "non-finite output (a poisoned element was read and used?)"
        err = np.nan_to_num(np.abs(got - ref), nan=np.inf)
        if float((err / bound).max()) > ratio:
            ratio = float((err / bound).max())
            w = np.unravel_index(int(np.argmax(err / bound)), err.shape)
            worst_at = dict(flat=int(idx[w]), row_in_seg=int(w[0]), col=int(w[1]), err=float(err[w]),
                            bound=float(np.broadcast_to(bound, err.shape)[w]))
        if wrote:
            j = R.join_f16(Oh[idx], Ol[idx])
            assert (np.abs(j - got) <= 2.0 ** -21 * np.abs(got) + 2.0 ** -35).all(), "join_f16(Oh, Ol) is not the f32 result"
    info.update(ratio=ratio, c_measured=measured_c)
    if scheme is not None:
        return info
    if STASH is not None:
        STASH[c["id"]] = got_f32.copy()
    assert ratio <= 1.0, f"worst error / bound {ratio:.3g} at {worst_at}"
    if wrote:
        assert_untouched(Oh, written, CANARY16, "Oh")
        assert_untouched(Ol, written, CANARY16, "Ol")
    assert_untouched(got_f32, written, CANARY32, "O")
    return info


# ---- LayerNorm / embed -------------------------------------------------------------------------------------------------------------
def norm_cases():
    out = []
    Ms = (1, 3, 4, 5, 1001)
    for i, d in enumerate((64, 128, 384, 1280, 260)):
        for j, M in enumerate(Ms):
            if M == 1001 and d not in (64, 260):
                continue
            for inside in (0, 1):
                out.append(dict(id=f"ln-d{d}-M{M}-eps{inside}", family="layernorm", kind="ln", d=d, M=M, inside=inside, data="normal",
                                emu=(d in (64, 260) and M in (1, 5))))
        out.append(dict(id=f"ln-const-d{d}", family="layernorm", kind="ln", d=d, M=5, inside=i % 2, data="const", emu=d == 260))
        out.append(dict(id=f"ln-const-d{d}-other-eps", family="layernorm", kind="ln", d=d, M=3, inside=1 - i % 2, data="const",
                        emu=False))
        out.append(dict(id=f"ln-cancel-d{d}", family="layernorm_cancel", kind="ln", d=d, M=4, inside=i % 2, data="cancel", emu=d == 64))
        out.append(dict(id=f"embed-d{d}", family="embed", kind="embed", d=d, M=Ms[i], emu=d in (64, 260)))
    out.append(dict(id="embed-d128-M1001", family="embed", kind="embed", d=128, M=1001, emu=False))
    out.append(dict(id="refuse-ln-d66", family="layernorm", kind="refuse", d=66, M=3, inside=0, data="normal", emu=True))
    return out


def run_norm(lib, c, scheme=None):
    """scheme: None (the harness) or a function (x, g, b, eps, inside) -> y in f64 that takes the kernel's place (see run_gemm)."""
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 15485863 + 3)
    d, M = c["d"], c["M"]
    info = dict(id=c["id"], family=c["family"], branch=None)
    t = Norm()
    t.M, t.d = M, d
    if c["kind"] == "embed":
        n_vocab, L = 37, 7
        E = nan32(G + n_vocab * d + G)
        E[G: G + n_vocab * d] = values(rng, n_vocab * d, 1.0)
        pos = nan32(G + L * d + G)
        pos[G: G + L * d] = values(rng, L * d, 1.0)
        tok = rng.integers(0, n_vocab, M).astype(np.int32)
        tok[0] = n_vocab - 1
        tok[-1] = 0
        y = canary32(G + (M + 1) * d + G)
        t.which, t.x, t.g, t.b, t.y, t.L, t.n_vocab = 2, buf(E, G), buf(pos, G), buf(tok), buf(y, G), L, n_vocab
        if scheme is not None:
            return info
        st = _call(lib.wbk_norm, t)
        assert st == 0, f"harness status {st}"
        ref = R.embed_ref(tok, E[G: G + n_vocab * d].reshape(n_vocab, d), pos[G: G + L * d].reshape(L, d), L)
        assert (y[G: G + M * d].reshape(M, d).view(np.uint32) == ref.view(np.uint32)).all(), "embed is not E[tok] + pos[r % L] exactly"
        written = np.zeros(y.size, dtype=bool)
        written[G: G + M * d] = True
        assert_untouched(y, written, CANARY32, "x")
        info["ratio"] = 0.0
        return info
    x = nan32(G + (M + 2) * d + G)
    if c["data"] == "cancel":
        xv = (1.0e4 + rng.standard_normal((M, d))).astype(np.float32)                  # mean 1e4, spread 1
    else:
        xv = (rng.standard_normal((M, d)) * 2.0 + 0.3).astype(np.float32)
        if c["data"] == "const":
            xv[0] = 0.5                                              # variance 0; every sum is exact in f32, so is the mean
            xv[M - 1] = -2.0
    x[G: G + M * d] = xv.ravel()
    g = nan32(G + d + G)
    b = nan32(G + d + G)
    gv = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    bv = values(rng, d, 0.1)
    g[G: G + d], b[G: G + d] = gv, bv
    y = canary32(G + (M + 1) * d + G)
    yh, yl = canary16(y.size), canary16(y.size)
    eps = 1e-5
    t.which, t.x, t.g, t.b, t.y, t.eps, t.eps_inside_sqrt = 0, buf(x, G), buf(g, G), buf(b, G), buf(y, G), eps, c.get("inside", 0)
    if c["kind"] == "refuse":
        if scheme is not None:
            return info
        assert _call(lib.wbk_norm, t) == EARG, "d % 4 != 0 must be refused before the launch"
        assert (y.view(np.uint32) == CANARY32).all()
        return info
    if scheme is None:
        st = _call(lib.wbk_norm, t)
        assert st == 0, f"harness status {st}"
    else:
        y[G: G + M * d] = scheme(xv, gv, bv, eps, c["inside"]).astype(np.float32).ravel()
    written = np.zeros(y.size, dtype=bool)
    written[G: G + M * d] = True
    assert_untouched(y, written, CANARY32, "y")
    got32 = y[G: G + M * d].reshape(M, d)
    got = got32.astype(np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    ref = R.layernorm_ref(xv, gv, bv, eps, c["inside"])
    f32 = R.layernorm_ref(xv, gv, bv, eps, c["inside"], dtype=np.float32)
    base = R.layernorm_base(xv, gv, bv, float(np.float32(eps)), c["inside"])
    cm = float((np.abs(f32 - ref) / base).max())
    bound = 4.0 * cm * base                                          # c = 4x the f32 NumPy evaluation's own error on THESE inputs
    err = np.abs(got - ref)
    if c["data"] == "const":
        rows = [0, M - 1]
        assert (got32[rows] == bv[None, :]).all(), "a constant row (variance 0) must give b exactly"
        keep = np.ones(M, dtype=bool)
        keep[rows] = False
        err, bound = err[keep], bound[keep]
    ratio = float((err / bound).max()) if err.size else 0.0
    info.update(ratio=ratio, c_measured=cm)
    if scheme is not None:
        return info
    assert (err <= bound).all(), f"worst error / bound {ratio:.3g} (c measured {cm:.3g})"
    # the pieces variant: split_f16 of the f32 output, bit for bit
    t.which, t.yh, t.yl = 1, buf(yh, G), buf(yl, G)
    y_before = y.copy()
    st = _call(lib.wbk_norm, t)
    assert st == 0, f"harness status {st} (pieces)"
    assert (y.view(np.uint32) == y_before.view(np.uint32)).all()
    eh, el = R.split_f16_bits(got32)
    assert (yh[G: G + M * d].reshape(M, d) == eh).all() and (yl[G: G + M * d].reshape(M, d) == el).all(), \
        "layernorm_pieces != split_f16(layernorm)"
    assert_untouched(yh, written, CANARY16, "yh")
    assert_untouched(yl, written, CANARY16, "yl")
    return info


# ---- skinny split-K GEMM -----------------------------------------------------------------------------------------------------------
PRESET_D = (384, 512, 768, 1024, 1280)          # whisper_burn_amd/synth.py PRESETS: tiny.en, base.en, small, medium, large-v2
SKINNY_M = (1, 9, 16, 17, 64)


def skinny_cases():
    """Every (K, N) a preset's decoder layer produces (QKV d x 3d, out d x d, MLP d x 4d and 4d x d); whether the skinny kernel
    serves it (skinny_ksplit > 0) is asked of the library at run time -- an unserved shape must be refused.  M: all five values at
    d = 384, one value per shape (rotating) at the larger presets, both weight variants everywhere."""
    out = []
    n = 0
    for d in PRESET_D:
        for K, N in ((d, 3 * d), (d, d), (d, 4 * d), (4 * d, d)):
            for M in (SKINNY_M if d == 384 else (SKINNY_M[n % 5],)):
                for pieces in (False, True):
                    out.append(dict(id=f"skinny-K{K}-N{N}-M{M}-{'f16x3' if pieces else 'f32'}", family="skinny", K=K, N=N, M=M,
                                    pieces=pieces, emu=False))
            n += 1
    for pieces in (False, True):                                    # M = 40: the three-row-tile instances (M in 33 .. 48)
        out.append(dict(id=f"skinny-K384-N1152-M40-{'f16x3' if pieces else 'f32'}", family="skinny", K=384, N=1152, M=40,
                        pieces=pieces, emu=False))
    out.append(dict(id="skinny-K128-N128-M9-f32", family="skinny", K=128, N=128, M=9, pieces=False, emu=True))
    out.append(dict(id="skinny-K128-N128-M17-f16x3", family="skinny", K=128, N=128, M=17, pieces=True, emu=True))
    return out


def run_skinny(lib, c):
    rng = np.random.default_rng(sum(map(ord, c["id"])) * 32452843 + 11)
    K, N, M = c["K"], c["N"], c["M"]
    info = dict(id=c["id"], family="skinny", branch=None)
    ks = lib.wbk_skinny_ksplit(K, N, 16, M)
    lda = K + 4
    A = nan32(G + 64 * lda + G)                                       # rows >= M: poison (st == nullptr: all M rows live)
    av = values(rng, (M, K), 1.0)
    for m in range(M):
        A[G + m * lda: G + m * lda + K] = av[m]
    W = values(rng, (K, N), 0.05)
    t = Skinny()
    t.A, t.B, t.lda, t.M, t.N, t.K = buf(A, G), buf(W), lda, M, N, K
    t.ksplit = max(ks, 1)
    plane = M * N + 8
    P = canary32(G + max(ks, 1) * plane + G)
    t.P, t.plane, t.use_range_flag = buf(P, G), plane, 1
    th = tl = None
    if c["pieces"]:
        th, tl = canary16(K * N), canary16(K * N)
        t.th, t.tl = buf(th), buf(tl)
    if ks == 0:
        # not served: the session keeps the tiled GEMM; the launcher must refuse the smallest ksplit outright
        st = _call(lib.wbk_skinny, t)
        assert st == -1, f"unserved shape: launcher returned {st}"
        assert (P.view(np.uint32) == CANARY32).all()
        info["served"] = False
        return info
    st = _call(lib.wbk_skinny, t)
    assert st == 0, f"harness status {st}"
    assert t.range_flag_out == 0, "range_flag raised on in-range inputs"
    if c["pieces"]:
        eh, el = R.tile_layout_ref(W)
        assert (th == eh.ravel()).all() and (tl == el.ravel()).all(), "launch_split_weight_f16_tiles != tile_layout_ref"
    written = np.zeros(P.size, dtype=bool)
    total = np.zeros((M, N), dtype=np.float64)
    for z in range(ks):
        sl = slice(G + z * plane, G + z * plane + M * N)
        written[sl] = True
        total += P[sl].reshape(M, N).astype(np.float64)
    assert np.isfinite(total).all(), "non-finite output (a poisoned element was read and used?)"
    ref = av.astype(np.float64) @ W.astype(np.float64)
    absdot = np.abs(av.astype(np.float64)) @ np.abs(W.astype(np.float64))
    bound = (K + 4) * R.U32 * absdot + (R.REP16 * absdot if c["pieces"] else 0.0)       # (the planes' sum is done in f64 here)
    err = np.abs(total - ref)
    ratio = float((err / bound).max())
    info.update(ratio=ratio, ksplit=ks, served=True)
    assert (err <= bound).all(), f"worst error / bound {ratio:.3g}"
    assert_untouched(P, written, CANARY32, "P")
    return info


# ---- running -----------------------------------------------------------------------------------------------------------------------
def all_cases():
    cases = {}
    for lst, fn in ((gemm_cases(), run_gemm), (attn_cases(), run_attn), (norm_cases(), run_norm), (skinny_cases(), run_skinny)):
        for c in lst:
            assert c["id"] not in cases, c["id"]
            cases[c["id"]] = (c, fn)
    return cases


def run_case(lib, cid):
    c, fn = all_cases()[cid]
    return fn(lib, c)


def main(argv):
    lib = load(argv[1])
    cases = all_cases()
    for cid in argv[2:]:
        c, fn = cases[cid]
        try:
            info = fn(lib, c)
            info["ok"] = True
        except AssertionError as e:
            info = dict(id=cid, family=c["family"], ok=False, msg=str(e))
        print("KCASE " + json.dumps(info), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
