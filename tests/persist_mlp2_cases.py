"""One layer's MLP of the persistent decode kernel in the two-phase form (csrc/decode_fused_bodies.h: dec_mlp_body, "two
phases"; 4 d / 64 co-resident blocks through `wbk_persist_mlp2` of the kernel-harness library) against dec_mlp_fused_kernel on
the same seeded inputs.  The one-launch kernel leaves the planes P [4 d / 64][S][d] and the folded stream x_out; its consumers
compute x_out + (b2 + sum_j P[j]), j ascending -- restated here in float32, one add at a time.  The two-phase roles leave that
row themselves and must leave the SAME BITS (compared as uint32), with their granule tag on every element of a live row and no
store at all for a masked row.

Cases: d = 128 and 384; 1 and 3 rows; with 3 rows also one row masked dead (the middle one, and the last one).
Shared by tests/test_emu_persist_mlp2_kernel.py (functional model) and tests/test_gpu_persist_mlp2_kernel.py (GPU)."""
import ctypes
import json
import sys

import numpy as np

TAG_IN = 0x00B30041


class WbkBuf(ctypes.Structure):
    _fields_ = [("host", ctypes.c_void_p), ("bytes", ctypes.c_int64), ("off", ctypes.c_int64)]


_BUFS = ["x_in", "pend", "pbias", "ln_g", "ln_b", "W1", "b1", "W2", "b2", "dead", "rows2", "tags2", "P", "x_out"]


class WbkMlp2(ctypes.Structure):
    _fields_ = [(n, WbkBuf) for n in _BUFS] + [(n, ctypes.c_int64) for n in ("S", "d", "KSp", "ld1", "ln_inside", "tag_in")] + \
               [("ln_eps", ctypes.c_double)]


def cases():
    out = []
    for d in (128, 384):
        for rows, dead in ((1, ()), (3, ()), (3, (1,)), (3, (2,))):
            out.append({"id": f"d{d}-rows{rows}" + ("".join(f"-dead{r}" for r in dead)), "d": d, "rows": rows, "dead": dead})
    return out


def load(path):
    lib = ctypes.CDLL(path)
    lib.wbk_persist_mlp2.argtypes = [ctypes.POINTER(WbkMlp2)]
    lib.wbk_persist_mlp2.restype = ctypes.c_int
    return lib


def check(lib, c):
    d, S, H = c["d"], c["rows"], c["d"] // 64
    rng = np.random.Generator(np.random.PCG64(7000 + d + 10 * S + sum(c["dead"])))
    f = lambda *shape, s=1.0: (rng.standard_normal(shape) * s).astype(np.float32)
    a = {"x_in": f(S, d), "pend": f(H, S, d, s=0.3), "pbias": f(d, s=0.1), "ln_g": 1.0 + f(d, s=0.1), "ln_b": f(d, s=0.1),
         "W1": f(d, 4 * d, s=d ** -0.5), "b1": f(4 * d, s=0.1), "W2": f(4 * d, d, s=(4 * d) ** -0.5), "b2": f(d, s=0.1),
         "dead": np.array([1 if r in c["dead"] else 0 for r in range(S)], np.int32),
         "rows2": np.zeros((S, d), np.uint32), "tags2": np.zeros((S, d), np.uint32),
         "P": np.zeros((4 * d // 64, S, d), np.float32), "x_out": np.zeros((S, d), np.float32)}
    t = WbkMlp2()
    for n in _BUFS:
        setattr(t, n, WbkBuf(a[n].ctypes.data, a[n].nbytes, 0))
    t.S, t.d, t.KSp, t.ld1, t.ln_inside, t.tag_in, t.ln_eps = S, d, H, 4 * d, 1, TAG_IN, 1e-5
    rc = lib.wbk_persist_mlp2(ctypes.byref(t))
    if rc != 0:
        return {"id": c["id"], "ok": False, "msg": f"wbk_persist_mlp2 returned {rc}"}
    msgs = []
    n_diff = 0
    for r in range(S):
        if r in c["dead"]:
            if (a["tags2"][r] == TAG_IN + 1).any():
                msgs.append(f"row {r} is masked but carries the stage's tag")
            continue
        acc = a["b2"].copy()
        for j in range(a["P"].shape[0]):
            acc = acc + a["P"][j, r]                    # float32, j ascending
        want = (a["x_out"][r] + acc).astype(np.float32)
        if not (a["tags2"][r] == TAG_IN + 1).all():
            msgs.append(f"row {r}: {int((a['tags2'][r] != TAG_IN + 1).sum())} elements without the stage's tag")
        bad = int((a["rows2"][r] != want.view(np.uint32)).sum())
        n_diff += bad
        if bad:
            msgs.append(f"row {r}: {bad} of {d} elements differ in bits, max |diff| "
                        f"{float(np.abs(a['rows2'][r].view(np.float32) - want).max()):.3e}")
        if not np.isfinite(want).all() or float(np.abs(want - a["x_out"][r]).max()) < 1e-3:
            msgs.append(f"row {r}: the reference row is degenerate")
    return {"id": c["id"], "ok": not msgs, "msg": "; ".join(msgs), "bits_differ": n_diff}


if __name__ == "__main__":          # every case in this process: python persist_mlp2_cases.py <library>
    lib_ = load(sys.argv[1])
    for c_ in cases():
        print("KCASE " + json.dumps(check(lib_, c_)), flush=True)
