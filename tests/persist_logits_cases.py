"""One logits role of the persistent decode kernel with the final LayerNorm inside it (csrc/decode_persist.hip: ps_logits_role,
a.mlp2 = 1) against the old pair, the final-LN role of every row followed by the logits role on its rows (a.mlp2 = 0), on the
same seeded rows, through `wbk_persist_logits` of the kernel-harness library.  Both leave one 16-byte record {tag, best value,
tag, best id} per (row, tile); the records must be IDENTICAL: value bits, id and both tags (compared as uint32).  A masked row
gets no record in either form.  A float64 restatement (LayerNorm, row . E^T, columns past V excluded) guards against both forms
being wrong together: the id must be its argmax and the value within 1e-4 relative.

Cases: d = 128 and 384; 1 and 3 rows; with 3 rows also one row masked dead; one tile (V = 100 of 128 columns: the tail past V is
-inf), and two tiles (V = 200) at d = 384.
Shared by tests/test_emu_persist_logits_kernel.py (functional model) and tests/test_gpu_persist_logits_kernel.py (GPU)."""
import ctypes
import json
import sys

import numpy as np

TAG = 0x00C50017
EPS = 1e-5


class WbkBuf(ctypes.Structure):
    _fields_ = [("host", ctypes.c_void_p), ("bytes", ctypes.c_int64), ("off", ctypes.c_int64)]


_BUFS = ["x", "ln_g", "ln_b", "Et", "dead", "rec"]


class WbkLogits(ctypes.Structure):
    _fields_ = [(n, WbkBuf) for n in _BUFS] + \
               [(n, ctypes.c_int64) for n in ("S", "d", "V", "vocab_ld", "n_t", "ln_inside", "tag", "mlp2")] + [("ln_eps", ctypes.c_double)]


def cases():
    out = []
    for d in (128, 384):
        for rows, dead in ((1, ()), (3, ()), (3, (1,))):
            out.append({"id": f"d{d}-rows{rows}" + "".join(f"-dead{r}" for r in dead) + "-1tile", "d": d, "rows": rows, "dead": dead, "V": 100})
    out.append({"id": "d384-rows3-2tiles", "d": 384, "rows": 3, "dead": (), "V": 200})
    out.append({"id": "d384-rows3-dead2-2tiles", "d": 384, "rows": 3, "dead": (2,), "V": 200})
    return out


def load(path):
    lib = ctypes.CDLL(path)
    lib.wbk_persist_logits.argtypes = [ctypes.POINTER(WbkLogits)]
    lib.wbk_persist_logits.restype = ctypes.c_int
    return lib


def _run(lib, a, c, mlp2):
    S, d, V = c["rows"], c["d"], c["V"]
    n_t = (V + 127) // 128
    rec = np.zeros((S, n_t, 4), np.uint32)
    bufs = dict(a, rec=rec)
    t = WbkLogits()
    for n in _BUFS:
        setattr(t, n, WbkBuf(bufs[n].ctypes.data, bufs[n].nbytes, 0))
    t.S, t.d, t.V, t.vocab_ld, t.n_t, t.ln_inside, t.tag, t.mlp2, t.ln_eps = S, d, V, 128 * n_t, n_t, 1, TAG, mlp2, EPS
    return lib.wbk_persist_logits(ctypes.byref(t)), rec


def check(lib, c):
    S, d, V = c["rows"], c["d"], c["V"]
    n_t = (V + 127) // 128
    rng = np.random.Generator(np.random.PCG64(9000 + d + 10 * S + V + sum(c["dead"])))
    f = lambda *shape, s=1.0: (rng.standard_normal(shape) * s).astype(np.float32)
    a = {"x": f(S, d, s=2.0) + f(S, 1), "ln_g": 1.0 + f(d, s=0.2), "ln_b": f(d, s=0.2), "Et": f(d, 128 * n_t, s=d ** -0.5),
         "dead": np.array([1 if r in c["dead"] else 0 for r in range(S)], np.int32)}
    rc1, new = _run(lib, a, c, 1)
    rc0, old = _run(lib, a, c, 0)
    if rc1 != 0 or rc0 != 0:
        return {"id": c["id"], "ok": False, "msg": f"wbk_persist_logits returned {rc1} (own LN) / {rc0} (final-LN role)"}
    msgs = []
    for r in range(S):
        if r in c["dead"]:
            if new[r].any() or old[r].any():
                msgs.append(f"row {r} is masked but has a record")
            continue
        if not (new[r] == old[r]).all():
            msgs.append(f"row {r}: records differ: own LN {new[r].tolist()} / final-LN role {old[r].tolist()}")
        if not ((new[r][:, 0] == TAG).all() and (new[r][:, 2] == TAG).all()):
            msgs.append(f"row {r}: a record without the tag")
        x = a["x"][r].astype(np.float64)
        xn = (x - x.mean()) / np.sqrt(x.var() + EPS) * a["ln_g"] + a["ln_b"]
        lg = xn @ a["Et"].astype(np.float64)
        for k in range(n_t):
            cols = lg[128 * k:min(128 * k + 128, V)]
            want_id, want_v = 128 * k + int(cols.argmax()), float(cols.max())
            got_v, got_id = float(new[r][k, 1:2].view(np.float32)[0]), int(new[r][k, 3])
            if got_id != want_id or abs(got_v - want_v) > 1e-4 * max(1.0, abs(want_v)):
                msgs.append(f"row {r} tile {k}: ({got_v}, {got_id}) against the float64 restatement ({want_v}, {want_id})")
    return {"id": c["id"], "ok": not msgs, "msg": "; ".join(msgs)}


if __name__ == "__main__":          # every case in this process: python persist_logits_cases.py <library>
    lib_ = load(sys.argv[1])
    for c_ in cases():
        print("KCASE " + json.dumps(check(lib_, c_)), flush=True)
