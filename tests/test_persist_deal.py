"""CPU: how one step's roles of the persistent decode kernel are dealt to the blocks (csrc/decode_chain.cpp: ps_deal_roles,
WHISPER_HIP_PERSIST_DEAL), through wb_persist_role_plan -- no device.

A block that holds a first-layer self- or cross-attention role is needed first in the next step; a merge or final-LN role on it
keeps it from requesting its operands until the step has ended.  The old dealing ("least loaded blocks") put merge(0..2) of
the bench shape on blocks 0, 1, 2 -- self-attention L0 of row 0, heads 0 - 2.  For both policies: every role once, every
block's list in the global dependency order, layer role i on block i % grid, the same logits split and the same blocks with
exactly one attention-type layer role (what the resident-operand counts rest on).  For the new one: the step's tail stays off
the first-layer attention blocks wherever W other blocks exist."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ATTN, CROSS, MLP, LOGITS, MERGE, FINLN = range(6)
# (n_layer, n_head, n_state, rows, n_vocab, grid)
BENCH = (4, 6, 384, 3, 51864, 256)
SHAPES = [BENCH, (2, 2, 128, 3, 2053, 256), (4, 6, 384, 3, 2053, 169), (2, 6, 384, 4, 2053, 40), (2, 6, 384, 4, 2053, 100),
          (2, 6, 384, 7, 2053, 40), (4, 8, 512, 3, 51864, 256)]
_CACHE = {}


def plan(shape, legacy):
    """[(kind, layer, row, block)] in the order the blocks hold them, and the grid after clamping"""
    if (shape, legacy) not in _CACHE:
        from whisper_burn_amd import _lib
        cap = 4096
        kinds, block = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        n = _lib.load(_lib.LIB_PATH).wb_persist_role_plan(*shape, int(legacy), kinds, block, cap)
        assert n > 0, n
        _CACHE[(shape, legacy)] = [(kinds[i] & 0xff, (kinds[i] >> 8) & 0xff, kinds[i] >> 16, block[i]) for i in range(n)]
    return _CACHE[(shape, legacy)]


def grid_of(shape):
    n_layer, n_head, d, rows, vocab, grid = shape
    return min(grid, n_layer * (2 * rows * n_head + 4 * d // 64) + (vocab + 127) // 128 + 2 * rows)


def per_block(roles, grid):
    out = [[] for _ in range(grid)]
    for k, l, r, b in roles:
        out[b].append((k, l, r))
    return out


def early_blocks(roles):
    return {b for k, l, r, b in roles if l == 0 and k in (ATTN, CROSS)}


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_role_once_in_dependency_order_layer_roles_in_place(shape, legacy):
    n_layer, n_head, d, rows, vocab, _ = shape
    grid, nb, roles = grid_of(shape), 4 * d // 64, plan(shape, legacy)
    blocks = [b for *_, b in roles]
    assert blocks == sorted(blocks) and 0 <= blocks[0] and blocks[-1] < grid          # grouped by block
    # every role of the step exactly once
    per_kind = {k: sorted((l, r) for kk, l, r, _ in roles if kk == k) for k in range(6)}
    heads = sorted((l, r) for l in range(n_layer) for r in range(rows) for _ in range(n_head))
    assert per_kind[ATTN] == heads and per_kind[CROSS] == heads
    assert per_kind[MLP] == sorted((l, 0) for l in range(n_layer) for _ in range(nb))
    assert per_kind[FINLN] == per_kind[MERGE] == [(0, r) for r in range(rows)]
    assert 1 <= len(per_kind[LOGITS]) <= (vocab + 127) // 128
    # layer role i (layer, then self-attention / cross-attention / MLP, then row) on block i % grid
    want = []
    for l in range(n_layer):
        want += [(ATTN, l, r) for r in range(rows) for _ in range(n_head)]
        want += [(CROSS, l, r) for r in range(rows) for _ in range(n_head)]
        want += [(MLP, l, 0)] * nb
    lists = per_block(roles, grid)
    got = [[x for x in lst if x[0] <= MLP] for lst in lists]
    assert got == [[want[i] for i in range(b, len(want), grid)] for b in range(grid)]
    # every block's list is a subsequence of the global order: layer roles by (layer, sublayer), finln, logits, merge
    rank = {FINLN: 1, LOGITS: 2, MERGE: 3}
    for lst in lists:
        keys = [(0, l, k) if k <= MLP else (rank[k], 0, 0) for k, l, _ in lst]
        assert keys == sorted(keys), lst


@pytest.mark.parametrize("shape", SHAPES)
def test_logits_split_and_single_attention_blocks_are_the_legacy_ones(shape):
    grid = grid_of(shape)
    new, old = plan(shape, False), plan(shape, True)

    def single(roles):
        return [b for b, lst in enumerate(per_block(roles, grid))
                if len([x for x in lst if x[0] <= MLP]) == 1 and [x for x in lst if x[0] <= MLP][0][0] != MLP]
    assert sum(k == LOGITS for k, *_ in new) == sum(k == LOGITS for k, *_ in old)
    assert single(new) == single(old)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_tail_of_the_step_stays_off_the_first_layer_attention_blocks(shape):
    rows, grid, roles = shape[3], grid_of(shape), plan(shape, False)
    early = early_blocks(roles)
    if grid - len(early) >= rows:
        assert not [(k, r, b) for k, _, r, b in roles if k in (MERGE, FINLN, LOGITS) and b in early]
    else:                # every block holds a first-layer attention role at this grid: the least loaded blocks, as before
        assert len(early) == grid and shape[5] == 40 and roles == plan(shape, True)


def test_bench_shape_merge_shares_the_block_of_its_final_layernorm():
    roles = plan(BENCH, False)
    fin = {r: b for k, _, r, b in roles if k == FINLN}
    mrg = {r: b for k, _, r, b in roles if k == MERGE}
    assert fin == mrg == {0: 240, 1: 241, 2: 242}
    for b in fin.values():
        assert [k for k, *_, bb in roles if bb == b] == [FINLN, MERGE]


def test_bench_shape_legacy_puts_the_merge_roles_on_blocks_0_1_2():
    roles = plan(BENCH, True)
    assert {r: b for k, _, r, b in roles if k == MERGE} == {0: 0, 1: 1, 2: 2}
    assert [[(k, l, r) for k, l, r, bb in roles if bb == b] for b in range(3)] == \
        [[(ATTN, 0, 0), (MERGE, 0, b)] for b in range(3)]
    assert {r: b for k, _, r, b in roles if k == FINLN} == {0: 240, 1: 241, 2: 242}


def test_a_shape_without_an_instance_is_an_error():
    from whisper_burn_amd import _lib
    kinds, block = (C.c_int32 * 4096)(), (C.c_int32 * 4096)()
    assert _lib.load(_lib.LIB_PATH).wb_persist_role_plan(4, 6, 384, 9, 51864, 256, 0, kinds, block, 4096) < 0
    assert _lib.load(_lib.LIB_PATH).wb_persist_role_plan(4, 6, 384, 3, 51864, 256, 0, kinds, block, 16) < 0   # no room
