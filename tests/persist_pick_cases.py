"""The token pick of the persistent kernel's first-layer self-attention role in isolation (csrc/decode_fused_bodies.h:
ps_pick_token, through `wbk_persist_pick` of the kernel-harness library): one row's tile records {tag, value, tag, id} in, the
picked id out, compared with a numpy restatement of `better()` (value descending, id ascending; NaN never compares; no record
that compares -> 0x7fffffff, which the role treats as end-of-text).  Integers: compared with ==.

Cases: n_tiles 1, 2, 406 (the real vocabulary's tile count: one record per thread) and 513 (a thread owns two records); the best
value tied between two tiles (the lowest id wins); the best value in the last tile; a row of only -inf (the lowest id); a row
holding NaN next to finite values (the NaN is passed over); a row of only NaN (nothing compares).
Shared by tests/test_emu_persist_pick.py (functional model) and tests/test_gpu_persist_pick_kernel.py (GPU)."""
import ctypes
import json
import sys

import numpy as np

NONE = 0x7FFFFFFF
TAG = 0x00A70013
CT = 128


class WbkBuf(ctypes.Structure):
    _fields_ = [("host", ctypes.c_void_p), ("bytes", ctypes.c_int64), ("off", ctypes.c_int64)]


class WbkPick(ctypes.Structure):
    _fields_ = [("rec", WbkBuf), ("n_tiles", ctypes.c_int64), ("tag", ctypes.c_int64), ("out_id", ctypes.c_int64)]


def ref_pick(vals, ids):
    """`better()` folded over the records: strictly greater value, or equal value and lower id; NaN compares with nothing."""
    bv, bi = -np.inf, NONE
    for v, i in zip(vals.tolist(), ids.tolist()):
        if v > bv or (v == bv and i < bi):
            bv, bi = v, i
    return bi


def cases():
    out = []

    def add(name, vals, ids):
        out.append({"id": name, "vals": np.asarray(vals, np.float32), "ids": np.asarray(ids, np.int32)})

    for n in (1, 2, 406, 513):
        rng = np.random.Generator(np.random.PCG64(1000 + n))
        # every tile's best id lies inside the tile, as the logits role writes it
        ids = np.arange(n) * CT + rng.integers(0, CT, n)
        add(f"random-{n}", rng.standard_normal(n) * 4.0, ids)
        v = rng.standard_normal(n).astype(np.float32)
        v[n - 1] = 9.0
        add(f"best-in-last-tile-{n}", v, ids)
        if n >= 2:
            v = rng.standard_normal(n).astype(np.float32)
            a, b = (0, n - 1) if n == 2 else (n // 3, n - 2)
            v[a] = v[b] = 7.5
            add(f"tie-{n}", v, ids)
            # ... and with the higher id in the EARLIER record (ids need not ascend with the record index)
            ids2 = ids.copy()
            ids2[a], ids2[b] = ids[b], ids[a]
            add(f"tie-swapped-{n}", v, ids2)
        add(f"all-neg-inf-{n}", np.full(n, -np.inf), ids)
        v = rng.standard_normal(n).astype(np.float32)
        v[::3] = np.nan
        add(f"nan-among-finite-{n}", v, ids)
        add(f"all-nan-{n}", np.full(n, np.nan), ids)
    return out


def run_case(lib, c, pad=3):
    """The records sit `pad` records into a larger array whose other records carry a foreign tag and a huge value: a pick that
    reads outside its n_tiles records would be refused by the harness or return a foreign id."""
    n = len(c["vals"])
    buf = np.zeros((n + 2 * pad, 4), np.uint32)
    buf[:, 0] = buf[:, 2] = TAG + 1
    buf[:, 1] = np.float32(1e30).view(np.uint32)
    buf[:, 3] = 0x0BADBAD
    body = buf[pad:pad + n]
    body[:, 0] = body[:, 2] = TAG
    body[:, 1] = c["vals"].view(np.uint32)
    body[:, 3] = c["ids"].view(np.uint32)
    t = WbkPick()
    t.rec = WbkBuf(buf.ctypes.data, buf.nbytes, pad * 16)
    t.n_tiles, t.tag, t.out_id = n, TAG, -7
    st = lib.wbk_persist_pick(ctypes.byref(t))
    return st, int(t.out_id)


def check(lib, c):
    st, got = run_case(lib, c)
    want = ref_pick(c["vals"], c["ids"])
    ok = st == 0 and got == want
    return {"id": c["id"], "ok": bool(ok), "msg": f"status {st}, picked {got}, numpy {want}"}


def load(path):
    lib = ctypes.CDLL(path)
    lib.wbk_persist_pick.argtypes = [ctypes.POINTER(WbkPick)]
    lib.wbk_persist_pick.restype = ctypes.c_int
    return lib


def main(path):
    lib = load(path)
    for c in cases():
        print("KCASE " + json.dumps(check(lib, c)))


if __name__ == "__main__":
    main(sys.argv[1])
