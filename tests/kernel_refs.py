"""Plain float64 restatements of the operators behind the host-callable launchers (whisper-burn_amd/csrc/kernels.h, decode.h),
written from the contracts stated there -- not from the kernels.  NumPy only, one function per operator, no cleverness:
tests/test_gpu_kernels.py and tests/test_kernel_harness_emu.py compare the HIP kernels with these.

Also here: the fp16 piece representation (split_f16 / join_f16: hi = fp16(x), lo = fp16((x - hi) 2^11)), the error bounds the
comparisons use (derived, see each function) and the NumPy statements of the two arithmetic schemes that the mutation tests
perturb."""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24            # unit roundoff of f32
REP16 = 3 * 2.0 ** -21      # split operands: each reconstructs to 2^-21 relative (2 operands) + the dropped lo.lo term (2^-22)
SQRT1_2 = 0.70710678118654752440


# ---- fp16 pieces ---------------------------------------------------------------------------------------------------------------
def split_f16(x):
    """x (f32) -> (hi, lo) as f32 arrays holding fp16 values: hi = fp16(x), lo = fp16((x - hi) * 2^11)."""
    x = np.asarray(x, dtype=np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    lo = ((x - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return hi, lo


def split_f16_bits(x):
    """The same pieces as the uint16 bit patterns the kernels store."""
    hi, lo = split_f16(x)
    return hi.astype(np.float16).view(np.uint16), lo.astype(np.float16).view(np.uint16)


def join_f16(hi_bits, lo_bits):
    """uint16 piece planes -> float64 value hi + lo / 2^11."""
    return (np.asarray(hi_bits, dtype=np.uint16).view(np.float16).astype(np.float64)
            + np.asarray(lo_bits, dtype=np.uint16).view(np.float16).astype(np.float64) / 2048.0)


def tile_layout_ref(W):
    """launch_split_weight_f16_tiles: W [K][N] f32 -> (hi, lo) uint16 [N/16][K/32][4][16][8]: tile (n / 16, k / 32), then
    octet (k % 32) / 8, column n % 16, element k % 8."""
    W = np.asarray(W, dtype=np.float32)
    K, N = W.shape
    assert K % 32 == 0 and N % 16 == 0
    hi, lo = split_f16_bits(W)
    out = []
    for p in (hi, lo):
        t = p.reshape(K // 32, 4, 8, N // 16, 16)           # [tk][oct][k8][tn][n16]
        out.append(np.ascontiguousarray(t.transpose(3, 0, 1, 4, 2)))
    return out[0], out[1]


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------
def _erf(x):
    try:                                                      # (vectorised; the same function as math.erf in f64)
        from scipy.special import erf
        return erf(x)
    except ImportError:
        return np.vectorize(math.erf, otypes=[np.float64])(x)


def gelu_erf(v):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + _erf(v * SQRT1_2))


def gelu_tanh(v):                                             # (a mutant: NOT what the kernels compute)
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def rows_effective(flat, base, M, K, lda, desc=None):
    """ROWS mode: the [M][K] matrix the GEMM multiplies.  flat: the whole f32 array, base: element index of the A pointer.
    desc: None, or [M] rows of (off, klo, khi): A[m][k] = flat[base + off + k] inside [klo, khi), 0 outside (never read)."""
    A = np.zeros((M, K), dtype=np.float64)
    for m in range(M):
        if desc is None:
            A[m] = flat[base + m * lda: base + m * lda + K]
        else:
            off, klo, khi = (int(v) for v in desc[m])
            A[m, klo:khi] = flat[base + off + klo: base + off + khi]
    return A


def conv1_effective(flat, base, M, K, tstride, desc):
    """CONV1 gather: A[m][ci * 3 + kk] = flat[base + off + ci * tstride + kk - 1]; kk = 0 is zero for the first frame of a
    window (klo = 1), kk = 2 for the last (khi = 1)."""
    A = np.zeros((M, K), dtype=np.float64)
    for m in range(M):
        off, first, last = (int(v) for v in desc[m])
        for ci in range(K // 3):
            for kk in range(3):
                if (kk == 0 and first) or (kk == 2 and last):
                    continue
                A[m, ci * 3 + kk] = flat[base + off + ci * tstride + kk - 1]
    return A


def gemm_ref(A, B, bias=None, act_gelu=False, col_scale=1.0, period=0, width=0, residual=None, aux=None, aux_idx=None,
             gelu=gelu_erf, variant="f32", gelu_ulps=4.0, acc_cap=None):
    """C = (act(A B + bias) * col_scale where n % period < width) + residual + aux[aux_idx[m]], in that order, in f64.
    Returns (C, pre, bound): pre = A B + bias (the activation's argument), bound = the elementwise bound on |C_kernel - C|:
    linear part (K + 4) 2^-24 (|A| |B|) -- any summation order with f32 accumulation; split precision ("f16x3") adds the
    representation term 3 * 2^-21 (|A| |B|) (operands >= 1e-3 in magnitude or exactly 0: no fp16-subnormal high pieces).
    bias / col_scale / residual / aux: one ulp of the value after each step (the bound so far scales with col_scale).
    GELU: 1.13 (its Lipschitz constant) times the bound of its argument + gelu_ulps ulps of max(1, |v|) for the device erff.
    acc_cap (split precision): caps the ACCUMULATION term only.  The worst-case term grows with K while a whole dropped cross
    term is at most 2^-12 (|A| |B|): from K ~ 200 on the worst-case bound alone cannot tell the two apart, so the caller caps it
    with 4x the error of a plain f32 NumPy matmul on the same inputs (never wider than the worst case; the representation term,
    which a correct kernel hardly uses, stays whole)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    K = A.shape[1]
    v = A @ B
    absdot = np.abs(A) @ np.abs(B)
    bound = (K + 4) * U32 * absdot
    if acc_cap is not None:
        bound = np.minimum(bound, acc_cap)
    if variant == "f16x3":
        bound = bound + REP16 * absdot
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)[None, :]
        bound = bound + U32 * np.abs(v)
    pre = v
    if act_gelu:
        bound = 1.13 * bound + gelu_ulps * U32 * np.maximum(1.0, np.abs(v))
        v = gelu(v)
    if period > 0:
        n = np.arange(B.shape[1])
        cs = np.where((n % period) < width, float(np.float32(col_scale)), 1.0)[None, :]
        v = v * cs
        bound = bound * np.abs(cs) + U32 * np.abs(v)
    if residual is not None:
        v = np.asarray(residual, dtype=np.float64) + v
        bound = bound + U32 * np.abs(v)
    if aux is not None:
        v = v + np.asarray(aux, dtype=np.float64)[np.asarray(aux_idx)]
        bound = bound + U32 * np.abs(v)
    return v, pre, bound


def gemm_epilogue(lin, bias=None, act_gelu=False, col_scale=1.0, period=0, width=0, residual=None, aux=None, aux_idx=None,
                  gelu=gelu_erf):
    """The epilogue of gemm_ref applied (in f64) to a given linear part -- for NumPy statements of the kernels' arithmetic."""
    v = np.asarray(lin, dtype=np.float64)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)[None, :]
    if act_gelu:
        v = gelu(v)
    if period > 0:
        n = np.arange(v.shape[1])
        v = v * np.where((n % period) < width, float(np.float32(col_scale)), 1.0)[None, :]
    if residual is not None:
        v = np.asarray(residual, dtype=np.float64) + v
    if aux is not None:
        v = v + np.asarray(aux, dtype=np.float64)[np.asarray(aux_idx)]
    return v


def splitk_slices(K, ksplit, tile=32):
    """The documented K-slice split of the tiled GEMMs: slice z covers [z * kchunk, min(K, (z + 1) * kchunk)) with
    kchunk = ceil(K / ksplit) rounded up to the k-tile."""
    kchunk = ((K + ksplit - 1) // ksplit + tile - 1) // tile * tile
    return [(min(K, z * kchunk), min(K, (z + 1) * kchunk)) for z in range(ksplit)]


def gemm_splitk_ref(A, B, ksplit):
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    return np.stack([A[:, a:b] @ B[a:b] for a, b in splitk_slices(A.shape[1], ksplit)])


def c_positions(M, N, ldc, c_block_cols=0, c_block_stride=0):
    """Element offsets (from the C pointer) of output (m, n): plain rows, or the column-block layout."""
    m = np.arange(M)[:, None]
    n = np.arange(N)[None, :]
    if c_block_cols > 0:
        return (n // c_block_cols) * c_block_stride + m * ldc + n % c_block_cols
    return m * ldc + n + 0 * m


# ---- the two arithmetic schemes (NumPy statements; the mutation tests perturb them) ------------------------------------------------
def matmul_f32(A, B):
    return (np.asarray(A, dtype=np.float32) @ np.asarray(B, dtype=np.float32)).astype(np.float64)


def matmul_f16x3(A, B, drop_cross=False, lo_unscale=1.0 / 2048.0):
    """hi.hi in one f32 accumulator, hi.lo + lo.hi in a second one that is scaled by 2^-11 at the end.
    Mutants: drop_cross = "a_lo" / "b_lo" (True = "a_lo") leaves that operand's low piece out; lo_unscale = 1 forgets the 2^-11."""
    ah, al = split_f16(A)
    bh, bl = split_f16(B)
    low = {False: lambda: ah @ bl + al @ bh, True: lambda: ah @ bl, "a_lo": lambda: ah @ bl, "b_lo": lambda: al @ bh}[drop_cross]()
    return (ah @ bh + low * np.float32(lo_unscale)).astype(np.float64)


# ---- attention -----------------------------------------------------------------------------------------------------------------
def attention_ref(Q, K, V, scale, causal, dtype=np.float64, strict_causal=False):
    """One segment, one head: softmax((Q s)(K s)^T [+ mask kv <= q]) V.  Q [q_len][64], K, V [kv_len][64].
    dtype = np.float32 evaluates the same statement in f32 (the yardstick of the tolerance).  Returns (O, max |Qs| |Ks|^T)."""
    s = dtype(np.float32(scale))
    Qs = np.asarray(Q, dtype=dtype) * s
    Ks = np.asarray(K, dtype=dtype) * s
    S = Qs @ Ks.T
    if causal:
        q = np.arange(S.shape[0])[:, None]
        kv = np.arange(S.shape[1])[None, :]
        S = np.where((kv < q) if strict_causal else (kv <= q), S, dtype(-np.inf))
    with np.errstate(invalid="ignore"):
        P = np.exp(S - S.max(axis=1, keepdims=True))
    P = np.nan_to_num(P, nan=0.0) if strict_causal else P
    with np.errstate(invalid="ignore", divide="ignore"):
        O = (P @ np.asarray(V, dtype=dtype)) / P.sum(axis=1, keepdims=True)
    sabs = float((np.abs(Qs.astype(np.float64)) @ np.abs(Ks.astype(np.float64)).T).max())
    return O.astype(np.float64), sabs


def attention_f16x3(Q, K, V, scale, causal, drop_cross=False, lo_unscale=1.0 / 2048.0, strict_causal=False):
    """The split-precision attention as a NumPy statement: the SCALED Q and K are split, both products are three-term."""
    s = np.float32(scale)
    Qs = np.asarray(Q, dtype=np.float32) * s
    Ks = np.asarray(K, dtype=np.float32) * s
    S = matmul_f16x3(Qs, Ks.T, drop_cross, lo_unscale).astype(np.float32)
    if causal:
        q = np.arange(S.shape[0])[:, None]
        kv = np.arange(S.shape[1])[None, :]
        S = np.where((kv < q) if strict_causal else (kv <= q), S, np.float32(-np.inf))
    with np.errstate(invalid="ignore"):
        P = np.exp(S - S.max(axis=1, keepdims=True)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return matmul_f16x3(P, V, drop_cross, lo_unscale) / P.sum(axis=1, keepdims=True, dtype=np.float32).astype(np.float64)


def attention_split_bound(Q, K, V, scale, causal):
    """Elementwise first-order bound on what the split representation adds to the error of O (on top of the f32 term):
    scores: |dS_ij| <= 3 * 2^-21 A_ij with A = |Qs| |Ks|^T;  softmax: dP_ij = P_ij (dS_ij - sum_l P_il dS_il);
    dO = dP V  =>  |dO| <= 3 * 2^-21 ((P A) |V| + rowsum(P A) (P |V|));  the P V product itself: 3 * 2^-21 (P |V|)."""
    s = float(np.float32(scale))
    Qs = np.asarray(Q, dtype=np.float64) * s
    Ks = np.asarray(K, dtype=np.float64) * s
    S = Qs @ Ks.T
    A = np.abs(Qs) @ np.abs(Ks).T
    if causal:
        q = np.arange(S.shape[0])[:, None]
        kv = np.arange(S.shape[1])[None, :]
        S = np.where(kv <= q, S, -np.inf)
    P = np.exp(S - S.max(axis=1, keepdims=True))
    P = P / P.sum(axis=1, keepdims=True)
    absV = np.abs(np.asarray(V, dtype=np.float64))
    PA = P * A
    return REP16 * (PA @ absV + PA.sum(axis=1, keepdims=True) * (P @ absV) + P @ absV)


def attention_base(Q, K, V, scale):
    """2^-24 (64 max|Qs| max|Ks| + kv_len) max|V|: the scale of the f32 error of one (segment, head)."""
    s = float(np.float32(scale))
    return U32 * (64.0 * float(np.abs(Q).max()) * s * float(np.abs(K).max()) * s + K.shape[0]) * float(np.abs(V).max())


# ---- LayerNorm / embed ---------------------------------------------------------------------------------------------------------
def layernorm_ref(x, g, b, eps, eps_inside_sqrt, dtype=np.float64, unbiased=False):
    """(x - mu) / (sqrt(var) + eps) * g + b, or (x - mu) / sqrt(var + eps) * g + b; biased variance."""
    x = np.asarray(x, dtype=dtype)
    d = x.shape[1]
    mu = x.sum(axis=1, keepdims=True, dtype=dtype) / dtype(d)
    var = ((x - mu) ** 2).sum(axis=1, keepdims=True, dtype=dtype) / dtype(d - 1 if unbiased else d)
    e = dtype(np.float32(eps))
    den = np.sqrt(var + e) if eps_inside_sqrt else np.sqrt(var) + e
    return ((x - mu) / den * np.asarray(g, dtype=dtype) + np.asarray(b, dtype=dtype)).astype(np.float64)


def layernorm_base(x, g, b, eps, eps_inside_sqrt):
    """2^-24 (|x - mu| / den |g| + |b| + 1) elementwise: the scale of the f32 error."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    den = np.sqrt(var + eps) if eps_inside_sqrt else np.sqrt(var) + eps
    return U32 * (np.abs(x - mu) / den * np.abs(g) + np.abs(b) + 1.0)


def embed_ref(tok, E, pos, L):
    """x[r] = E[tok[r]] + pos[r % L], one f32 addition per element: exact in f32."""
    tok = np.asarray(tok)
    r = np.arange(tok.shape[0])
    return (np.asarray(E, dtype=np.float32)[tok] + np.asarray(pos, dtype=np.float32)[r % L]).astype(np.float32)
