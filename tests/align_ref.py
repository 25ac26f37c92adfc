"""Token alignment restated in torch / NumPy on top of the oracle (the checker side of wb_align_tokens):

  1. one teacher-forced decoder pass, recording the cross-attention weights softmax((q s)(k s)^T) of the alignment heads
  2. z-score over the token axis per (head, encoder position), biased variance; a column with std == 0 gives zeros
  3. median filter of width `filter_width` along the positions, reflect padding (skipped when C <= filter_width // 2)
  4. M = mean over the heads; X = -M[n_prefix : len - drop_last]
  5. DTW in f32 (strict comparisons: diagonal, then up, then left), backtrace; a token's start position is the column
     of the first path cell of its row.

`dtype=torch.float64` gives the f64 statement of steps 1 - 4 (the DTW always runs on the f32 cast of its input when
`dtw_dtype` is float32, on f64 otherwise)."""
from __future__ import annotations

import numpy as np
import torch

from oracle.model import OracleWhisper, softmax


def default_heads(n_layer: int, n_head: int):
    return [(l, h) for l in range(n_layer // 2, n_layer) for h in range(n_head)]


class AlignOracle(OracleWhisper):
    """OracleWhisper that keeps the cross-attention weights of every layer of the last forward_decoder call."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cross_weights = {}

    def cross_attention(self, p: str, x, xa, n_head):
        q = self.linear(p + "/query", x)
        k = self.linear(p + "/key", xa)
        v = self.linear(p + "/value", xa)
        n_batch, n_qctx, n_state = q.shape
        n_ctx = k.shape[1]
        scale = float(np.float32((n_state / n_head) ** -0.25)) if q.dtype == torch.float32 \
            else (n_state / n_head) ** -0.25
        dh = n_state // n_head
        qh = q.reshape(n_batch, n_qctx, n_head, dh).transpose(1, 2) * scale
        kh = k.reshape(n_batch, n_ctx, n_head, dh).transpose(1, 2).transpose(2, 3) * scale
        vh = v.reshape(n_batch, n_ctx, n_head, dh).transpose(1, 2)
        w = softmax(qh.matmul(kh), 3)                       # [n, H, L, C]
        layer = int(p.split("block_")[1].split("/")[0])
        self.cross_weights[layer] = w
        return self.linear(p + "/out", w.matmul(vh).transpose(1, 2).flatten(2, 3))


def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    """Median of `width` (odd) neighbours along the last axis, reflect padding; unchanged when the axis is too short."""
    hw = width // 2
    if x.shape[-1] <= hw:
        return x
    idx = torch.arange(-hw, x.shape[-1] + hw)
    idx = idx.abs()
    C = x.shape[-1]
    idx = torch.where(idx >= C, 2 * (C - 1) - idx, idx)
    xp = x[..., idx]
    return xp.unfold(-1, width, 1).sort(-1).values[..., hw]


def dtw_start_positions(x: np.ndarray) -> np.ndarray:
    """Step 5 on x [N, C] in x's own dtype; returns the start position of every row."""
    x = np.asarray(x)
    N, C = x.shape
    inf = x.dtype.type(np.inf)
    cost = np.full((N + 1, C + 1), inf, dtype=x.dtype)
    trace = np.full((N + 1, C + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for i in range(1, N + 1):
        ci, cp, xi, ti = cost[i], cost[i - 1], x[i - 1], trace[i]
        for j in range(1, C + 1):
            c0, c1, c2 = cp[j - 1], cp[j], ci[j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            ci[j] = xi[j - 1] + c
            ti[j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, C
    start = np.full(N, -1, dtype=np.int32)
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            start[i - 1] = j - 1
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return start


def alignment_matrix(model: AlignOracle, tokens, xa, heads=None, filter_width: int = 7) -> torch.Tensor:
    """Steps 1 - 4 for ONE row: tokens [len], xa [C, d] -> M [len, C] in the model's dtype."""
    D = model.dims
    heads = default_heads(D.n_text_layer, D.n_text_head) if heads is None else [tuple(h) for h in heads]
    heads = sorted(heads, key=lambda lh: lh[0])             # (stable: the pass meets the layers in order)
    tok = torch.as_tensor(np.asarray(tokens, dtype=np.int64))[None]
    model.forward_decoder(tok, torch.as_tensor(np.asarray(xa)).to(model.dtype)[None])
    acc = None
    for (l, h) in heads:
        w = model.cross_weights[l][0, h]                    # [len, C]
        mean = w.mean(0, keepdim=True)
        std = torch.sqrt(((w - mean) ** 2).mean(0, keepdim=True))
        z = torch.where(std > 0, (w - mean) / torch.where(std > 0, std, torch.ones_like(std)), torch.zeros_like(w))
        z = median_filter(z, filter_width)
        acc = z if acc is None else acc + z
    return acc / len(heads)


def start_positions(M, n_prefix: int = 4, drop_last: int = 1, dtw_dtype=np.float32) -> np.ndarray:
    """Step 5 over M [len, C]: [len] int32, -1 outside the DTW rows."""
    M = np.asarray(M)
    L = M.shape[0]
    out = np.full(L, -1, dtype=np.int32)
    x = (-M[n_prefix:L - drop_last]).astype(dtw_dtype)
    out[n_prefix:L - drop_last] = dtw_start_positions(x)
    return out


def stitch_with_times(rows, times, max_n_offsets: int = 40, min_n_overlaps: int = 3):
    """oracle.transcribe.stitch carrying a (token, time) tuple: a token keeps the time of the window it came from."""
    from oracle.transcribe import find_chunk_overlap
    toks, tms = [], []
    for r, t in zip(rows, times):
        r, t = list(r), list(t)
        ov = find_chunk_overlap(toks, r, max_n_offsets, min_n_overlaps)
        if ov is not None:
            pi, ci = ov
            toks, tms = toks[:pi] + r[ci:], tms[:pi] + t[ci:]
        else:
            toks, tms = toks + r, tms + t
    return toks, tms
