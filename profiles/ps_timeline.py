#!/usr/bin/env python3
"""Role timeline of the persistent decode kernel (WHISPER_HIP_PS_STAMPS=<file> python bench.py ...).
Per role kind and layer, over the roles of LIVE rows only (a row whose window has ended skips its attention roles): the
time from role start to the wait being passed, the phases after the wait, and the arrive; per step, the critical chain.
Stamp slots: 0 role start, 1 wait passed, 2-5 phases inside the role, 6 done, 7 arrived.  Clock: 100 MHz (10 ns ticks).
Below the table, for the attn, cross, mlp, finln and merge rows: min / median / max OVER THE ROLES of the kind (each role's mean over
the steps) of "wait passed @" and "done @" relative to the step start -- a stage whose roles fall in two groups shows here and
not in a mean -- and, when the file carries role_off behind the stamps (files written since R15), each role's block.
Then the MLP edges: from the last MLP role's "done" of layer l to "x folded" (p2) of the next layer's self-attention roles (the
last layer: of the final-LN roles, or of the logits roles where the deal has no final-LN role), the spread of a layer's MLP
roles' "done" inside a step, and the step time separately for the steps with one, two, three ... live rows.
    python profiles/ps_timeline.py stamps.bin [first_step last_step] [row]"""
import sys

import numpy as np

raw = np.fromfile(sys.argv[1], dtype=np.uint8)
n_steps, n_roles, grid, ns = [int(x) for x in raw[:16].view(np.int32)]
kinds = raw[16:16 + 4 * n_roles].view(np.int32)
n_st = 8 * n_steps * n_roles * ns
st = raw[16 + 4 * n_roles:16 + 4 * n_roles + n_st].view(np.uint64).reshape(n_steps, n_roles, ns).astype(np.float64)
tail = raw[16 + 4 * n_roles + n_st:]                # optional: marker "ROff", then role_off [grid + 1]
block = None
if len(tail) >= 4 * (grid + 2) and int(tail[:4].view(np.int32)[0]) == 0x66664f52:
    role_off = tail[4:4 * (grid + 2)].view(np.int32)
    block = np.searchsorted(role_off, np.arange(n_roles), side="right") - 1
st[st == 0] = np.nan
names = {0: "attn", 1: "cross", 2: "mlp", 3: "logits", 4: "merge", 5: "finln"}
kind, layer, row = kinds & 0xff, (kinds >> 8) & 0xff, kinds >> 16
ran = ~np.isnan(st[:, :, 6])
last = int(np.nonzero(ran.any(1))[0].max()) + 1 if ran.any() else 0
lo = int(sys.argv[2]) if len(sys.argv) > 2 else min(8, max(last - 1, 0))
hi = int(sys.argv[3]) if len(sys.argv) > 3 else last
live_row = int(sys.argv[4]) if len(sys.argv) > 4 else 0
tick = 0.01
print(f"steps stamped {last} of {n_steps}, roles/step {n_roles}, grid {grid}; statistics over steps [{lo}, {hi}), attention roles of row {live_row}")
sel = st[lo:hi]
merge_done = sel[:, kind == 4, 7]
step_end = np.nanmax(merge_done, axis=1)
step_start = np.concatenate([[np.nan], step_end[:-1]])
hdr = f"{'role':<10}{'n':>4}{'wait':>8}{'w->p2':>8}{'p2->p3':>8}{'p3->p4':>8}{'p4->p5':>8}{'p5->done':>9}{'arrive':>8}{'run':>8}{'done@':>9}{'arrived@':>9}"
print(hdr)
spread = []
for k in (0, 1, 2, 5, 3, 4):
    for l in sorted(set(layer[kind == k])):
        cols = (kind == k) & (layer == l)
        if k in (0, 1, 5):
            cols &= row == live_row
        if not cols.any():
            continue
        s = sel[:, cols, :]
        def d(a, b):
            x = (s[:, :, b] - s[:, :, a]) * tick
            return np.nanmean(x) if np.isfinite(x).any() else float("nan")
        rel_done = np.nanmean((np.nanmax(s[:, :, 6], axis=1) - step_start) * tick)
        rel_arr = np.nanmean((np.nanmax(s[:, :, 7], axis=1) - step_start) * tick)
        nm = names[k] + (f" L{l}" if k < 3 else "")
        if k in (0, 1, 2, 3, 4, 5):                 # per role: mean over the steps of (stamp - step start)
            wp = np.nanmean((s[:, :, 1] - step_start[:, None]) * tick, axis=0)
            dn = np.nanmean((s[:, :, 6] - step_start[:, None]) * tick, axis=0)
            spread.append((nm, wp, dn, block[cols] if block is not None else None))
        print(f"{nm:<10}{int(cols.sum()):>4}{d(0,1):>8.2f}{d(1,2):>8.2f}{d(2,3):>8.2f}{d(3,4):>8.2f}{d(4,5):>8.2f}{d(5,6):>9.2f}{d(6,7):>8.2f}{d(1,6):>8.2f}{rel_done:>9.2f}{rel_arr:>9.2f}")
dd = np.diff(step_end) * tick
print(f"step time (merge arrived -> next merge arrived): mean {np.nanmean(dd):.2f} us, median {np.nanmedian(dd):.2f}, min {np.nanmin(dd):.2f}, max {np.nanmax(dd):.2f}")
# the step boundary: from the last logits role's "done" of step s to "x folded" (p2) of the attn L0 roles of step s + 1
a0 = (kind == 0) & (layer == 0) & (row == live_row)
if a0.any() and (kind == 3).any() and hi - lo > 1:
    lg_done = np.nanmax(st[lo:hi - 1][:, kind == 3, 6], axis=1)
    for nm, red in (("first", np.nanmin), ("last", np.nanmax)):
        edge = (red(st[lo + 1:hi][:, a0, 2], axis=1) - lg_done) * tick
        print(f"last logits done -> attn L0 p2 ({nm} block of row {live_row}): mean {np.nanmean(edge):.2f} us, median {np.nanmedian(edge):.2f}, min {np.nanmin(edge):.2f}, max {np.nanmax(edge):.2f}")
print("over the roles of a kind (each role: mean over the steps), us after the step start (merge: of its own step's start):")
print(f"{'role':<10}{'n':>4}  {'wait passed @  min / median / max':<36}{'done @  min / median / max':<34}")
for nm, wp, dn, blk in spread:
    f3 = lambda v: f"{np.nanmin(v):8.2f} /{np.nanmedian(v):8.2f} /{np.nanmax(v):8.2f}"
    print(f"{nm:<10}{len(wp):>4}  {f3(wp):<36}{f3(dn):<34}")
    if nm == "logits" and blk is not None:          # the last to finish, and what else their blocks hold
        late = np.argsort(-np.nan_to_num(dn))[:12]
        def held(b):
            o = [names[kind[i]] + f" L{layer[i]}" for i in np.nonzero(block == b)[0] if kind[i] < 3]
            return "+".join(o) if o else "-"
        print(f"{'':<10}last to finish (block [its layer roles]: wait passed @ / done @)  " +
              "  ".join(f"b{blk[i]}[{held(blk[i])}]:{wp[i]:.2f}/{dn[i]:.2f}" for i in late))
        behind = np.array([held(b) != "-" for b in blk])
        for lab, m in (("behind a layer role", behind), ("on blocks without one", ~behind)):
            if m.any():
                print(f"{'':<10}{lab}: n {int(m.sum())}, done @ min / median / max {np.nanmin(dn[m]):.2f} / {np.nanmedian(dn[m]):.2f} / {np.nanmax(dn[m]):.2f}")
    if nm in ("attn L0", "merge", "finln"):
        per = "  ".join((f"b{blk[i]}:" if blk is not None else f"#{i}:") + f"{wp[i]:.2f}/{dn[i]:.2f}" for i in range(len(wp)))
        print(f"{'':<10}per role (block: wait passed @ / done @)  {per}")
# the MLP edges: last mlp(l) done -> p2 of the consumers; spread of the MLP roles' done inside a step
def stats(v):
    return f"mean {np.nanmean(v):.2f} us, median {np.nanmedian(v):.2f}, min {np.nanmin(v):.2f}, max {np.nanmax(v):.2f}"
n_layer = int(layer[kind == 2].max()) + 1 if (kind == 2).any() else 0
for l in range(n_layer):
    m = (kind == 2) & (layer == l)
    mdone = sel[:, m, 6]
    if not np.isfinite(mdone).any():
        continue
    last_done = np.nanmax(mdone, axis=1)
    print(f"mlp L{l} done, last - first role inside a step ({int(m.sum())} roles): {stats((last_done - np.nanmin(mdone, axis=1)) * tick)}")
    if l + 1 < n_layer:
        cons, cn = (kind == 0) & (layer == l + 1) & (row == live_row), f"attn L{l + 1} p2"
    elif (kind == 5).any():
        cons, cn = (kind == 5) & (row == live_row), "finln p2"
    else:
        cons, cn = kind == 3, "logits p2"
    if cons.any() and np.isfinite(sel[:, cons, 2]).any():
        for nm, red in (("first", np.nanmin), ("last", np.nanmax)):
            print(f"last mlp L{l} done -> {cn} ({nm} block): {stats((red(sel[:, cons, 2], axis=1) - last_done) * tick)}")
# step time by the number of live rows (a row is live in a step when a first-layer self-attention role of it folded its x row)
a0all = (kind == 0) & (layer == 0)
if a0all.any() and hi - lo > 1:
    rows = sorted(set(row[a0all]))
    n_live = np.zeros(hi - lo, dtype=int)
    for r in rows:
        n_live += np.isfinite(sel[:, a0all & (row == r), 2]).any(axis=1)
    for n in sorted(set(n_live[1:]), reverse=True):
        v = dd[n_live[1:] == n]
        if len(v) and np.isfinite(v).any():
            print(f"step time with {n} live row(s) ({len(v)} steps): {stats(v)}")
